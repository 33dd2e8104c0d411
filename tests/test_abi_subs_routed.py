"""CPU: the ABI of hvws_subs_update_routed and its getters -- exported, bound
with argument types, the header's constant equal to the binding's and the
oracle's (tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd
import wsturn as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_subs_update_routed", "hvws_get_subs_merged", "hvws_get_subs_events")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    S = libhv_amd._SIGS
    assert S["hvws_subs_update_routed"] == (ctypes.c_int, [V, V, V, U64, V, U64, U32, V, V, U64, ctypes.POINTER(U64)])
    assert S["hvws_get_subs_merged"] == (ctypes.c_int, [V, ctypes.POINTER(U64)])
    assert S["hvws_get_subs_events"] == (ctypes.c_int, [V, V, U64, U64])
    for m in ("subs_update_routed", "subs_merged", "subs_events"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_the_header_declares_what_is_bound():
    """Argument counts of the declarations in include/hvws.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        assert len(m.group(1).split(",")) == len(libhv_amd._SIGS[n][1]), n


def test_constants_agree():
    d = {n: int(v) for n, v in re.findall(r"^#define\s+(HVWS_\w+)\s+(\d+)u\b", _header(), re.M)}
    assert d.get("HVWS_SUBS_OVER") == 2 and d.get("HVWS_SUBS_UNIQUE") == 1
    assert libhv_amd.SUBS_OVER == N.OVER == 2 and libhv_amd.SUBS_UNIQUE == N.UNIQUE == 1
    assert (libhv_amd.SUB_JOIN, libhv_amd.SUB_LEAVE, libhv_amd.SUB_DROP) == (N.JOIN, N.LEAVE, N.DROP)
    assert (libhv_amd.RF_CLOSED, libhv_amd.RT_BAD, libhv_amd.BF_OVER) == (N.RF_CLOSED, N.RT_BAD, N.BF_OVER)


def test_null_context_is_refused():
    L = libhv_amd.lib()
    n = ctypes.c_uint64(7)
    assert L.hvws_subs_update_routed(None, None, None, 0, None, 0, 0, None, None, 0, ctypes.byref(n)) == -2
    out = (ctypes.c_uint64 * 4)()
    assert L.hvws_get_subs_merged(None, out) == -2
    assert L.hvws_get_subs_events(None, None, 0, 0) == -2
