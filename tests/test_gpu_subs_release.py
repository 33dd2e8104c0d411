"""GPU: tests/test_gpu_ctx_release.py's property for hvws_subs_update -- a
destroyed context that ran the pass (its drops from a reply call's flags, the
pair sort, both scans, the placement, its upload slot and the getters) holds no
device and no pinned bytes.  The table of each cycle is compared with
tests/wssubs.py, so the cycle is known to have run what it claims."""
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
from test_gpu_fanout_release import held

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    row = [H.build_frames_ref([(1 | FIN | MASK, b"room %d" % c, KEY)] + ([(8 | FIN | MASK, b"\x03\xe8", KEY)] if c == 1 else []))
           for c in range(3)]
    topics = [[0, 1, 2, 300], [2, 2, 1], []]
    dest_of, ndest = [0, 1, 2], 301
    events = [(U.JOIN, 2, 300), (U.LEAVE, 0, 300), (U.JOIN, 2, 7), (U.DROP, 0, 2), (U.JOIN, 0, 2)]
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    pieces = R.rfc_batch(data, segs)[1]
    flags = R.replies_of(pieces, 3, POLICY)[3]
    closed = U.closed_dests(flags, dest_of)
    assert closed == [1]
    want_first, want_member, want_counts, _ = U.update(topics, closed, events, U.UNIQUE)
    first, member = W.flatten(topics)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        df, dm = eng.to_device(first), eng.to_device(member)
        of, om = eng.alloc(8 * 4), eng.alloc(4 * 16)
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        n = eng.subs_update(df, dm, 3, len(member), ndest, events, dest_of, of, om, 16, U.UNIQUE)
        assert n == len(want_member) == libhv_amd.lib().hvws_subs_count(eng.ctx)
        assert eng.subs_counts() == want_counts
        assert of.download(8 * 4, np.uint64).tolist() == want_first.tolist()
        assert om.download(4 * n, np.uint32).tolist() == want_member.tolist()
        eng.sync()
        for b in (rx, out, df, dm, of, om):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_subs_update_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0] and inside[1] > before[1], (before, inside)
