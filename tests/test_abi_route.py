"""CPU: the ABI of hvws_route / hvws_fanout_routed -- exported, bound with
argument types, the header's constants equal to the binding's and the oracle's
(tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd
import wsroute as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_route", "hvws_route_device", "hvws_route_topics_device", "hvws_route_events_device",
         "hvws_route_event_count_device", "hvws_get_route", "hvws_route_event_count", "hvws_get_route_events",
         "hvws_get_route_flags", "hvws_get_route_totals", "hvws_fanout_routed")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def _defines():
    return {n: int(v) for n, v in re.findall(r"^#define\s+(HVWS_\w+)\s+(\d+)u\b", _header(), re.M)}


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    S = libhv_amd._SIGS
    assert S["hvws_route"] == (ctypes.c_int, [V, U32, U32, V])
    for n in NAMES[1:5]:
        assert S[n] == (V, [V]), n
    assert S["hvws_get_route"] == (ctypes.c_int, [V, V, V, V, U64, U64])
    assert S["hvws_route_event_count"] == (ctypes.c_int64, [V])
    assert S["hvws_get_route_events"] == (ctypes.c_int, [V, V, U64, U64])
    assert S["hvws_get_route_flags"] == (ctypes.c_int, [V, V, V])
    assert S["hvws_get_route_totals"] == (ctypes.c_int, [V, ctypes.POINTER(U64)])
    assert S["hvws_fanout_routed"] == (ctypes.c_int, [V, V, V, U64, U32, U64, ctypes.POINTER(U64)])
    for m in ("route", "route_table", "route_events", "route_flags", "route_totals", "fanout_routed"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_the_header_declares_what_is_bound():
    """Argument counts of the declarations in include/hvws.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        assert len(m.group(1).split(",")) == len(libhv_amd._SIGS[n][1]), n


def test_constants_agree():
    d = _defines()
    want = {"HVWS_ROUTE_HDR_MAX": 12, "HVWS_RK_OTHER": 0, "HVWS_RK_PUB": 1, "HVWS_RK_SUB": 2, "HVWS_RK_UNSUB": 3,
            "HVWS_RK_BAD": 4, "HVWS_RK_STOPPED": 5, "HVWS_RT_BAD": 1, "HVWS_SUB_JOIN": 1, "HVWS_SUB_LEAVE": 2}
    for k, v in want.items():
        assert d.get(k) == v, (k, d.get(k))
    assert re.search(r"^#define\s+HVWS_ROUTE_NONE\s+UINT64_MAX\b", _header(), re.M)
    A = libhv_amd
    assert (A.RK_OTHER, A.RK_PUB, A.RK_SUB, A.RK_UNSUB, A.RK_BAD, A.RK_STOPPED) == (
        T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED) == (0, 1, 2, 3, 4, 5)
    assert A.ROUTE_HDR_MAX == T.HDR_MAX == 12 and A.RT_BAD == T.RT_BAD == 1
    assert A.ROUTE_NONE == T.ROUTE_NONE == (1 << 64) - 1
    assert (A.SUB_JOIN, A.SUB_LEAVE) == (T.JOIN, T.LEAVE) and A.FAN_NONE == T.FAN_NONE and A.FAN_SELF == T.FAN_SELF


def test_null_context_is_refused():
    L = libhv_amd.lib()
    n = ctypes.c_uint64(7)
    assert L.hvws_route(None, 1, 1, None) == -2
    assert L.hvws_fanout_routed(None, None, None, 0, 0, 0, ctypes.byref(n)) == -2
    for name in NAMES[1:5]:
        assert not getattr(L, name)(None), name
    assert L.hvws_get_route(None, None, None, None, 0, 0) == -2
    assert L.hvws_route_event_count(None) == -1
    assert L.hvws_get_route_events(None, None, 0, 0) == -2
    assert L.hvws_get_route_flags(None, None, None) == -2
    out = (ctypes.c_uint64 * 4)()
    assert L.hvws_get_route_totals(None, out) == -2
