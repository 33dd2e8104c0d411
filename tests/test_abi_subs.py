"""CPU: the ABI of hvws_subs_update -- exported, bound with argument types, the
header's constants equal to the binding's and the oracle's, the event's size
(tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd
import wssubs as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_subs_update", "hvws_subs_count", "hvws_get_subs_counts")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def _defines():
    return {n: int(v) for n, v in re.findall(r"^#define\s+(HVWS_\w+)\s+(\d+)u\b", _header(), re.M)}


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    res, args = libhv_amd._SIGS["hvws_subs_update"]
    assert res is ctypes.c_int and len(args) == 14
    assert args[3] is ctypes.c_uint32 and args[4] is ctypes.c_uint64 and args[5] is ctypes.c_uint32
    assert args[7] is ctypes.c_uint64 and args[9] is ctypes.c_uint32 and args[12] is ctypes.c_uint64
    assert args[13] == ctypes.POINTER(ctypes.c_uint64)
    assert libhv_amd._SIGS["hvws_subs_count"] == (ctypes.c_int64, [ctypes.c_void_p])
    assert libhv_amd._SIGS["hvws_get_subs_counts"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)])
    for m in ("subs_update", "subs_counts"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_constants_agree():
    d = _defines()
    want = {"HVWS_SUB_JOIN": 1, "HVWS_SUB_LEAVE": 2, "HVWS_SUB_DROP": 3, "HVWS_SUBS_UNIQUE": 1, "HVWS_RF_CLOSED": 1}
    for k, v in want.items():
        assert d.get(k) == v, (k, d.get(k))
    assert (libhv_amd.SUB_JOIN, libhv_amd.SUB_LEAVE, libhv_amd.SUB_DROP) == (U.JOIN, U.LEAVE, U.DROP) == (1, 2, 3)
    assert libhv_amd.SUBS_UNIQUE == U.UNIQUE == 1 and libhv_amd.RF_CLOSED == U.RF_CLOSED


def test_the_event_is_three_words():
    m = re.search(r"typedef struct hvws_sub_event \{([^}]*)\} hvws_sub_event;", _header())
    assert m and [w.strip() for w in m.group(1).replace("uint32_t", "").strip(" ;").split(",")] == ["op", "topic", "dest"]
    assert libhv_amd.SUB_EVENT_DTYPE.itemsize == 12 and libhv_amd.SUB_EVENT_DTYPE.names == ("op", "topic", "dest")
    assert [libhv_amd.SUB_EVENT_DTYPE.fields[n][1] for n in ("op", "topic", "dest")] == [0, 4, 8]


def test_null_context_is_refused():
    L = libhv_amd.lib()
    n = ctypes.c_uint64(7)
    assert L.hvws_subs_update(None, None, None, 0, 0, 1, None, 0, None, 0, None, None, 0, ctypes.byref(n)) == -2
    assert L.hvws_subs_count(None) == -1
    out = (ctypes.c_uint64 * 4)()
    assert L.hvws_get_subs_counts(None, out) == -2
