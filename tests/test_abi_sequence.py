"""CPU: the ABI of hvws_sequence and hvws_envelope_sequenced -- exported, bound
with argument types, the declarations' argument counts, the constant, a NULL
context refused (tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_sequence", "hvws_sequence_device", "hvws_get_sequence", "hvws_get_sequence_totals",
         "hvws_envelope_sequenced_bound", "hvws_envelope_sequenced")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "hvws.h")).read()


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    V, U32, U64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    S = libhv_amd._SIGS
    assert S["hvws_sequence"] == (ctypes.c_int, [V, V, U32])
    assert S["hvws_sequence_device"] == (V, [V])
    assert S["hvws_get_sequence"] == (ctypes.c_int, [V, V, U64, U64])
    assert S["hvws_get_sequence_totals"] == (ctypes.c_int, [V, ctypes.POINTER(U64)])
    assert S["hvws_envelope_sequenced_bound"] == S["hvws_envelope_bound"]
    assert S["hvws_envelope_sequenced"] == S["hvws_envelope"]
    for m in ("sequence", "sequence_table", "sequence_totals", "envelope_sequenced_bound", "envelope_sequenced"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_the_header_declares_what_is_bound():
    """Argument counts of the declarations in include/hvws.h."""
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % n, src)
        assert m, n
        args = [a for a in m.group(1).split(",") if a.strip() != "void"]
        assert len(args) == len(libhv_amd._SIGS[n][1]), n


def test_the_constant():
    assert re.search(r"#define\s+HVWS_SEQ_HDR_MAX\s+45u\b", _header())
    assert libhv_amd.SEQ_HDR_MAX == 45 == len(b"M4294967295 4294967295 #18446744073709551615\n")


def test_null_context_is_refused():
    L = libhv_amd.lib()
    assert L.hvws_sequence(None, None, 0) == -2
    assert not L.hvws_sequence_device(None)
    assert L.hvws_get_sequence(None, None, 0, 0) == -2
    out = (ctypes.c_uint64 * 2)()
    assert L.hvws_get_sequence_totals(None, out) == -2
    assert L.hvws_envelope_sequenced_bound(None) == 0
    assert L.hvws_envelope_sequenced(None, None, 0, 0) == -2
