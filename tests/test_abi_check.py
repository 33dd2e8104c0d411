"""CPU: the ABI of hvws_check / hvws_replies_checked -- exported, bound with
argument types, and the header's constants equal to the binding's and the
oracle's (tests/test_abi.py enumerates include/hvws.h for the rest)."""
from __future__ import annotations

import ctypes
import os
import re

import libhv_amd
import wscheck as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_check", "hvws_get_check", "hvws_check_device", "hvws_replies_checked")


def _defines():
    src = open(os.path.join(ROOT, "include", "hvws.h")).read()
    out = {}
    for name, val in re.findall(r"^#define\s+(HVWS_\w+)\s+\(?(1u << \d+|0x[0-9A-Fa-f]+u|\d+u|UINT64_MAX)\)?\s*$", src, re.M):
        if val == "UINT64_MAX":
            out[name] = (1 << 64) - 1
        elif "<<" in val:
            out[name] = 1 << int(val.split("<<")[1])
        else:
            out[name] = int(val.rstrip("u"), 0)
    return out


def test_symbols_and_signatures():
    L = libhv_amd.lib()
    for n in NAMES:
        assert hasattr(L, n) and n in libhv_amd._SIGS, n
    assert libhv_amd._SIGS["hvws_check"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64,
                                                            ctypes.c_void_p])
    assert libhv_amd._SIGS["hvws_check_device"][0] is ctypes.c_void_p
    assert len(libhv_amd._SIGS["hvws_get_check"][1]) == 5
    for m in ("check", "check_result", "replies_checked"):
        assert callable(getattr(libhv_amd.Engine, m))


def test_constants_agree():
    d = _defines()
    want = {"HVWS_C_HEADER": 1, "HVWS_C_SEQUENCE": 2, "HVWS_C_CLOSE_BODY": 4, "HVWS_C_CLOSE_UTF8": 8,
            "HVWS_C_TEXT_UTF8": 16, "HVWS_C_SIZE": 32, "HVWS_C_ALL": 63, "HVWS_CK_OPEN": 1, "HVWS_CK_FAILED": 2,
            "HVWS_CHECK_NONE": (1 << 64) - 1, "HVWS_RF_FAILED": 4, "HVWS_RF_CLOSED": 1}
    for k, v in want.items():
        assert d.get(k) == v, (k, d.get(k))
    assert (libhv_amd.C_HEADER, libhv_amd.C_SEQUENCE, libhv_amd.C_CLOSE_BODY, libhv_amd.C_CLOSE_UTF8,
            libhv_amd.C_TEXT_UTF8, libhv_amd.C_SIZE) == C.CLASSES
    assert (libhv_amd.C_ALL, libhv_amd.CK_OPEN, libhv_amd.CK_FAILED, libhv_amd.CHECK_NONE, libhv_amd.RF_FAILED) == (
        C.C_ALL, C.CK_OPEN, C.CK_FAILED, C.NONE, C.RF_FAILED)


def test_null_context_is_refused():
    L = libhv_amd.lib()
    assert L.hvws_check(None, 0, 0, None) == -2
    assert L.hvws_get_check(None, None, None, None, None) == -2
    assert L.hvws_replies_checked(None, 0, None) == -2
    assert not L.hvws_check_device(None)
