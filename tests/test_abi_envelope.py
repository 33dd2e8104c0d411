"""CPU: the ABI of hvws_envelope -- exported, bound with argument types, the
declarations' argument counts, the constants, a NULL context refused
(tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_envelope_bound", "hvws_envelope_tile", "hvws_envelope", "hvws_envelope_device", "hvws_get_envelope",
         "hvws_get_envelope_totals", "hvws_fanout_enveloped", "hvws_retain_enveloped")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    S = libhv_amd._SIGS
    assert S["hvws_envelope_bound"] == (U64, [V]) and S["hvws_envelope_tile"] == (U32, [])
    assert S["hvws_envelope"] == (ctypes.c_int, [V, V, U64, U32])
    assert S["hvws_envelope_device"] == (V, [V])
    assert S["hvws_get_envelope"] == (ctypes.c_int, [V, V, U64, U64])
    assert S["hvws_get_envelope_totals"] == (ctypes.c_int, [V, ctypes.POINTER(U64)])
    assert S["hvws_fanout_enveloped"] == S["hvws_fanout_routed"]
    assert S["hvws_retain_enveloped"] == S["hvws_retain"]
    for m in ("envelope_bound", "envelope", "envelope_table", "envelope_totals", "fanout_enveloped", "retain_enveloped"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_the_header_declares_what_is_bound():
    """Argument counts of the declarations in include/hvws.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(libhv_amd._SIGS[n][1]), n


def test_the_constants():
    src = _header()
    assert re.search(r"#define\s+HVWS_ENV_SENDER\s+1u\b", src) and re.search(r"#define\s+HVWS_ENV_HDR_MAX\s+23u\b", src)
    assert libhv_amd.ENV_SENDER == 1 and libhv_amd.ENV_HDR_MAX == 23 == len(b"M4294967295 4294967295\n")
    tile = libhv_amd.lib().hvws_envelope_tile()
    assert tile > 0 and tile % 16 == 0


def test_null_context_is_refused():
    L = libhv_amd.lib()
    assert L.hvws_envelope_bound(None) == 0
    assert L.hvws_envelope(None, None, 0, 0) == -2
    assert not L.hvws_envelope_device(None)
    assert L.hvws_get_envelope(None, None, 0, 0) == -2
    out = (ctypes.c_uint64 * 4)()
    assert L.hvws_get_envelope_totals(None, out) == -2
    n = ctypes.c_uint64(7)
    assert L.hvws_fanout_enveloped(None, None, None, 0, 0, 0, ctypes.byref(n)) == -2
    assert L.hvws_retain_enveloped(None, None, 16, None, 0) == -2
