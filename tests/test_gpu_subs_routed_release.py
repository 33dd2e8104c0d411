"""GPU: tests/test_gpu_ctx_release.py's property for hvws_subs_update_routed --
a destroyed context that ran the call (the route, the routed fan-out and the
budget in front of it, the two compactions, the merged array, its upload slot,
both waits, the placement and the getters) holds no device and no pinned
bytes.  The table of each cycle is compared with tests/wssubs.py over
tests/wsturn.py's merged events, so the cycle is known to have run what it
claims."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import wsfan as W
import wsharness as H
import wsmsg as M
import wsrfc as R
import wssend as S
import wssubs as U
import wsturn as N
from test_gpu_fanout_release import held

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    msgs = [[b"S2\n", b"P0\n" + b"z" * 50], [b"U1\n"], [b"S0\n", b"junk"]]
    row = [H.build_frames_ref([(1 | FIN | MASK, m, KEY) for m in ms] + ([(8 | FIN | MASK, b"\x03\xe8", KEY)] if c == 1 else []))
           for c, ms in enumerate(msgs)]
    topics = [[0, 1, 2, 300], [2, 2, 1], []]
    dest_of, ndest = [0, 1, 2], 301
    host = [(U.JOIN, 2, 300), (U.LEAVE, 0, 300), (U.JOIN, 1, 1)]
    budgets = [1 << 40] * ndest
    budgets[300] = 5
    first, member = W.flatten(topics)
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        df, dm = eng.to_device(first), eng.to_device(member)
        of, om = eng.alloc(8 * 4), eng.alloc(4 * 16)
        db = eng.to_device(np.array(budgets, np.uint64))
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        eng.route(3, ndest, dest_of)
        eng.fanout_routed(df, dm, len(member))
        eng.budget(db, 0)
        n = eng.subs_update_routed(df, dm, len(member), host, of, om, 16, U.UNIQUE | N.OVER)
        ev = [tuple(int(x) for x in e) for e in eng.route_events().tolist()]
        over = eng.dest_budget(ndest)[3].tolist()
        m = N.merged(ev, eng.reply_flags(3).tolist(), eng.route_flags(3)[0].tolist(), dest_of, over, host, N.OVER)
        assert m == [(U.JOIN, 2, 0), (U.LEAVE, 1, 1), (U.JOIN, 0, 2), (U.DROP, 0, 1), (U.DROP, 0, 2), (U.DROP, 0, 300)] + host
        assert eng.subs_merged() == (3, 2, 1, 3)
        assert [tuple(int(x) for x in e) for e in eng.subs_events().tolist()] == m
        want_first, want_member, want_counts, _ = U.update(topics, (), m, U.UNIQUE)
        assert n == len(want_member) == libhv_amd.lib().hvws_subs_count(eng.ctx)
        assert eng.subs_counts() == want_counts
        assert of.download(8 * 4, np.uint64).tolist() == want_first.tolist()
        assert om.download(4 * n, np.uint32).tolist() == want_member.tolist()
        eng.sync()
        for b in (rx, out, df, dm, of, om, db):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_subs_update_routed_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0] and inside[1] > before[1], (before, inside)
