"""CPU: the ABI of hvws_retain -- exported, bound with argument types, the
declarations' argument counts, hvws_retained's size, a NULL context refused
(tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_retain", "hvws_retain_device", "hvws_retain_count_device", "hvws_retain_count", "hvws_get_retain",
         "hvws_get_segment_retain", "hvws_get_retain_totals", "hvws_retain_tile")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    S = libhv_amd._SIGS
    assert S["hvws_retain"] == (ctypes.c_int, [V, V, U64, V, U32])
    assert S["hvws_retain_device"] == (V, [V]) and S["hvws_retain_count_device"] == (V, [V])
    assert S["hvws_retain_count"] == (ctypes.c_int64, [V])
    assert S["hvws_get_retain"] == (ctypes.c_int, [V, V, V, V, U64, U64])
    assert S["hvws_get_segment_retain"] == (ctypes.c_int, [V, V, V])
    assert S["hvws_get_retain_totals"] == (ctypes.c_int, [V, ctypes.POINTER(U64)])
    assert S["hvws_retain_tile"] == (U64, [])
    for m in ("retain", "retain_table", "segment_retain", "retain_totals"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_the_header_declares_what_is_bound():
    """Argument counts of the declarations in include/hvws.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(libhv_amd._SIGS[n][1]), n


def test_the_entry_is_16_bytes():
    m = re.search(r"typedef struct hvws_retained \{(.*?)\} hvws_retained;", _header(), re.S)
    assert m
    fields = re.findall(r"\b(uint64_t|uint32_t)\s+(\w+);", m.group(1))
    assert fields == [("uint64_t", "len"), ("uint32_t", "flags"), ("uint32_t", "set")]
    assert libhv_amd.RETAINED_DTYPE.itemsize == 16 == sum(8 if t == "uint64_t" else 4 for t, _ in fields)
    assert libhv_amd.RETAINED_DTYPE.names == tuple(n for _, n in fields)
    tile = libhv_amd.lib().hvws_retain_tile()
    assert tile > 0 and tile % 16 == 0


def test_null_context_is_refused():
    L = libhv_amd.lib()
    assert L.hvws_retain(None, None, 16, None, 0) == -2
    assert not L.hvws_retain_device(None) and not L.hvws_retain_count_device(None)
    assert L.hvws_retain_count(None) == -1
    assert L.hvws_get_retain(None, None, None, None, 0, 0) == -2
    assert L.hvws_get_segment_retain(None, None, None) == -2
    out = (ctypes.c_uint64 * 5)()
    assert L.hvws_get_retain_totals(None, out) == -2
