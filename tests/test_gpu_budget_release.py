"""GPU: tests/test_gpu_ctx_release.py's property for hvws_budget -- a destroyed
context that ran the pass (its size scan, the cut, the scans over the
destinations, the placement) and every getter holds no device and no pinned
bytes.  The kept table of each cycle is compared with tests/wsbudget.py, so the
cycle is known to have run what it claims."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import libhv_amd
import wsbudget as G
import wsfan as W
import wsharness as H
import wsmsg as M
import wsrfc as R
import wssend as S

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO


def held():
    """(device bytes, pinned bytes) from the first line of hvws_debug_dump."""
    r, w = os.pipe()
    try:
        libhv_amd.lib().hvws_debug_dump(w)
    finally:
        os.close(w)
    with os.fdopen(r) as f:
        first = f.readline()
    m = re.search(r"holding (\d+) device bytes, (\d+) pinned bytes", first)
    assert m, first
    return int(m.group(1)), int(m.group(2))


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    row = [H.build_frames_ref([(1 | FIN | MASK, b"room %d" % c, KEY), (9 | FIN | MASK, b"p", KEY)]) for c in range(3)]
    topics = [[0, 1, 2, 200], [2, 2]]
    pub, dest_of, ndest = [0, 1, libhv_amd.FAN_NONE], [0, 1, 2], 201
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    pieces = R.rfc_batch(data, segs)[1]
    rep, answered, _, _ = R.replies_of(pieces, 3, POLICY)
    fan = W.fanout(rep, W.senders(pieces, answered), topics, ndest, pub, dest_of)
    budgets = [G.UNLIMITED] * ndest
    budgets[2] = G.prefix_sums(fan)[2][1]           # destination 2 keeps two of its deliveries
    budgets[200] = 0
    want = G.budget(fan, budgets)
    assert want[6][2] and want[6][3] == 2
    first, member = W.flatten(topics)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        df, dm = eng.to_device(first), eng.to_device(member)
        db = eng.to_device(np.array(budgets, np.uint64))
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        assert eng.fanout(df, dm, 2, len(member), ndest, pub, dest_of) == len(fan[0])
        eng.budget(db, 0, 0, False)
        table, reply = eng.budget_table()
        assert [tuple(int(x) for x in r) for r in table.tolist()] == want[0] and reply.tolist() == want[1]
        f, c, off, fl = eng.dest_budget(ndest)
        assert (f.tolist(), c.tolist(), off.tolist(), fl.tolist()) == (want[2], want[3], want[4], want[5])
        assert eng.budget_totals() == want[6]
        eng.sync()
        for b in (rx, out, df, dm, db):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_budget_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0] and inside[1] > before[1], (before, inside)
