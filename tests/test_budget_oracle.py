"""CPU: the hvws_budget model (tests/wsbudget.py) that the GPU test then holds the
device to, over delivery tables tests/wsfan.py makes from random small turns:

  - its closed form equals a sequential simulation of hio_write's rule (reference
    event/nio.c:554-560) at message granularity: a running write_bufsize per
    destination, the first write over the limit fails, nothing goes out after it;
  - wssend.closed_form is the length of wssend.expected for the same message;
  - every destination's frames of the kept table have exactly
    byte_off[d + 1] - byte_off[d] bytes;
  - the kept set is a prefix; a budget equal to a prefix sum keeps that delivery
    and one byte less drops it;

and the binding declares what the model speaks of."""
from __future__ import annotations

import ctypes
import os
import random
import re

import pytest

import libhv_amd
import wsbudget as G
import wsfan as W
import wsrfc as R
import wssend as S

POLICY = S.R_SERVER | S.R_ECHO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hvws_budget", "hvws_budget_device", "hvws_budget_count_device", "hvws_budget_count", "hvws_get_budget",
         "hvws_get_dest_budget", "hvws_get_budget_totals")
# (fragment, masked): the default 65535, fragments shorter than most messages, one longer
FORMS = ((0, False), (5, False), (126, False), (0, True), (5, True), (1, False))


def test_the_entry_points_exist_with_the_models_constant():
    L = libhv_amd.lib()
    for name in NAMES:
        assert hasattr(L, name) and name in libhv_amd._SIGS, name
    assert libhv_amd._SIGS["hvws_budget"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int])
    assert len(libhv_amd._SIGS["hvws_get_dest_budget"][1]) == 5
    assert libhv_amd._SIGS["hvws_get_budget_totals"][1][1] == ctypes.POINTER(ctypes.c_uint64)
    for m in ("budget", "budget_device", "budget_table", "dest_budget", "budget_totals"):
        assert callable(getattr(libhv_amd.Engine, m))
    src = open(os.path.join(ROOT, "include", "hvws.h")).read()
    assert re.search(r"^#define\s+HVWS_BF_OVER\s+1u\b", src, re.M)
    assert libhv_amd.BF_OVER == G.BF_OVER == 1
    # a null context is refused, by every entry point
    out = (ctypes.c_uint64 * 4)()
    assert L.hvws_budget(None, None, 0, 0, 0) == -2 and L.hvws_budget_count(None) == -1
    assert not L.hvws_budget_device(None) and not L.hvws_budget_count_device(None)
    assert L.hvws_get_budget(None, None, None, 0, 0) != 0 and L.hvws_get_dest_budget(None, None, None, None, None) == -2
    assert L.hvws_get_budget_totals(None, out) == -2


def turns(seed: int, n: int):
    """n random turns: (the message call's output bytes, the fan-out's result)."""
    rng = random.Random(seed)
    for _ in range(n):
        reads, topics, ndest, pub, dest_of, flags = W.random_case(rng)
        data, segs, _, _, _ = R.Chain(len(reads)).inputs(reads)
        out, pieces = R.rfc_batch(data, segs)[:2]
        rep, answered, _, _ = R.replies_of(pieces, len(reads), POLICY)
        yield out, W.fanout(rep, W.senders(pieces, answered), topics, ndest, pub, dest_of, flags), rng


def test_closed_form_is_the_length_of_the_frames():
    rng = random.Random(5)
    lengths = [0, 1, 4, 5, 6, 125, 126, 127, 251, 252, 253, 65535, 65536, 65537, 131070, 131071, 200000]
    lengths += [rng.randrange(0, 70000) for _ in range(40)]
    for n in lengths:
        body = bytes(n)
        for fragment in (0, 5, 126, 65536):
            if fragment == 5 and n > 2000:
                continue   # 40 000 frames say nothing 400 do not
            for masked in (False, True):
                data, offs, nfr = S.expected([(0x12, body, 7)], fragment, masked)
                assert (nfr, len(data)) == S.closed_form(n, fragment, masked), (n, fragment, masked)
                assert G.wire(n, fragment, masked) == len(data) > 0


def test_the_closed_form_is_the_sequential_rule():
    """1500 turns; the budgets as the GPU test draws them.  Both classes of
    destination are well represented, on the cases drawn here."""
    cut = whole = nonempty = 0
    kinds = set()
    for i, (out, fan, rng) in enumerate(turns(99, 1500)):
        fragment, masked = FORMS[i % len(FORMS)]
        table, reply, first, count = fan
        ndest = len(first)
        budgets = G.random_budgets(rng, fan, fragment, masked)
        kept, reply_out, first2, count2, byte_off, flags, totals = G.budget(fan, budgets, 12345, fragment, masked)
        written, closed = G.simulate(fan, budgets, fragment, masked)
        # the same deliveries go out, in the same order, and the same channels close
        at = [first[d] + j for d in range(ndest) for j in range(count2[d])]
        assert at == sorted(written) and sorted(set(at)) == at
        assert kept == [table[k] for k in at] and reply_out == [reply[k] for k in at]
        assert closed == [d for d in range(ndest) if flags[d] & G.BF_OVER]
        # the kept set is a prefix of every range, laid out densely
        assert all(0 <= count2[d] <= count[d] for d in range(ndest))
        assert first2 == [sum(count2[:d]) for d in range(ndest)]
        assert totals == (len(kept), byte_off[-1], len(table) - len(kept), len(closed))
        c = G.prefix_sums(fan, fragment, masked)
        for d in range(ndest):
            assert byte_off[d + 1] - byte_off[d] == (c[d][count2[d] - 1] if count2[d] else 0) <= budgets[d]
            assert bool(flags[d]) == (count2[d] < count[d])
            if flags[d]:
                assert c[d][count2[d]] > budgets[d]
            if not count[d]:
                assert flags[d] == 0
                continue
            nonempty += 1
            cut += 1 if flags[d] else 0
            whole += 0 if flags[d] else 1
            kinds.add("zero" if budgets[d] == 0 else "total" if budgets[d] == c[d][-1] else "other")
        # every destination's frames of the kept table have exactly its byte range
        for d in range(ndest):
            msgs = [(fl, out[o:o + ln], key) for o, ln, fl, key in kept[first2[d]:first2[d] + count2[d]]]
            assert len(S.expected(msgs, fragment, masked)[0]) == byte_off[d + 1] - byte_off[d]
        if not masked:
            per = W.destination_frames(out, kept, first2, count2, fragment)
            assert [len(b) for b in per] == [byte_off[d + 1] - byte_off[d] for d in range(ndest)]
    assert nonempty > 3000 and 4 * cut >= nonempty and 4 * whole >= nonempty, (nonempty, cut, whole)
    assert kinds == {"zero", "total", "other"}


def test_a_budget_equal_to_a_prefix_sum_keeps_and_one_byte_less_drops():
    seen = 0
    for i, (out, fan, rng) in enumerate(turns(7, 300)):
        fragment, masked = FORMS[i % len(FORMS)]
        table, reply, first, count = fan
        c = G.prefix_sums(fan, fragment, masked)
        for d in range(len(first)):
            for j in range(count[d]):
                b = [G.UNLIMITED] * len(first)
                b[d] = c[d][j]
                r = G.budget(fan, b, 0, fragment, masked)
                assert r[3][d] == j + 1 and bool(r[5][d]) == (j + 1 < count[d])
                b[d] = c[d][j] - 1
                r = G.budget(fan, b, 0, fragment, masked)
                assert r[3][d] == j and r[5][d] == G.BF_OVER
                # nobody else is touched
                assert all(r[3][e] == count[e] and not r[5][e] for e in range(len(first)) if e != d)
                seen += 1
    assert seen > 1000


def test_budget_all_stands_in_for_a_null_array():
    for out, fan, rng in turns(11, 100):
        ndest = len(fan[2])
        for b in (0, 1, 30, 400, G.UNLIMITED):
            assert G.budget(fan, None, b) == G.budget(fan, [b] * ndest, 77)
        assert G.budget(fan, None, G.UNLIMITED)[0] == fan[0] and G.budget(fan, None, 0)[0] == []
        assert G.budget(fan, None, 0)[6][3] == sum(1 for n in fan[3] if n)
