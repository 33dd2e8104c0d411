"""GPU: tests/test_gpu_ctx_release.py's property for hvws_route and
hvws_fanout_routed -- a destroyed context that ran both (the parse, the count
scan, the finish, the upload slot, the per-publication self counts, the sort,
the getters) holds no device and no pinned bytes.  The tables of each cycle are
compared with tests/wsroute.py, so the cycle is known to have run what it
claims."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import libhv_amd
import wsfan as W
import wsharness as H
import wsmsg as M
import wsrfc as R
import wsroute as T
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
    row = [H.build_frames_ref([(1 | FIN | MASK, b"P%d\nroom %d" % (c % 2, c), KEY), (9 | FIN | MASK, b"p", KEY),
                               (2 | FIN | MASK, b"S1\n" if c else b"oops", KEY)]) for c in range(3)]
    subs = [[0, 1, 2, 200], [2, 2]]
    dest_of, ndest = [0, 1, 2], 201
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    out_bytes, pieces = R.rfc_batch(data, segs)[:2]
    rep, answered, _, _ = R.replies_of(pieces, 3, POLICY)
    sender = W.senders(pieces, answered)
    want = T.route(rep, sender, out_bytes, 2, dest_of)
    fan = T.fanout_routed(want[0], want[1], sender, subs, ndest, dest_of)
    first, member = W.flatten(subs)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        df, dm = eng.to_device(first), eng.to_device(member)
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        eng.route(2, ndest, dest_of)
        rows, topic, kind = eng.route_table()
        assert ([tuple(int(x) for x in r) for r in rows.tolist()], topic.tolist(), kind.tolist()) == want[:3]
        assert [tuple(int(x) for x in e) for e in eng.route_events().tolist()] == want[3] and len(want[3]) == 2
        fl, bad = eng.route_flags(3)
        assert (fl.tolist(), bad.tolist()) == (want[4], want[5]) and eng.route_totals() == want[6]
        assert eng.fanout_routed(df, dm, len(member)) == len(fan[0])
        table, reply = eng.fanout_table()
        assert [tuple(int(x) for x in r) for r in table.tolist()] == fan[0] and reply.tolist() == fan[1]
        f, c = eng.dest_fanout(ndest)
        assert (f.tolist(), c.tolist()) == (fan[2], fan[3])
        eng.sync()
        for b in (rx, out, df, dm):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_route_and_the_routed_fanout_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0] and inside[1] > before[1], (before, inside)
