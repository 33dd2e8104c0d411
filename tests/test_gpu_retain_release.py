"""GPU: tests/test_gpu_ctx_release.py's property for hvws_retain -- a destroyed
context that ran it (the pick, the plan scan, the finish, the copy, the
getters) holds no device and no pinned bytes.  The tables of each cycle are
compared with tests/wsretain.py, so the cycle is known to have run what it
claims."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import wsfan as W
import wsharness as H
import wsmsg as M
import wsretain as N
import wsrfc as R
import wsroute as T
import wssend as S
from test_gpu_route_release import held

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO
SLOT = 32


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    row = [H.build_frames_ref([(1 | FIN | MASK, b"P%d\nroom %d says hello" % (c % 2, c), KEY), (9 | FIN | MASK, b"p", KEY),
                               (2 | FIN | MASK, b"S%d\n" % (c % 2), KEY)]) for c in range(3)]
    dest_of, ndest = [0, 1, 2], 201
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    out_bytes, pieces = R.rfc_batch(data, segs)[:2]
    rep, answered, _, _ = R.replies_of(pieces, 3, POLICY)
    sender = W.senders(pieces, answered)
    rows, topics, kinds, events = T.route(rep, sender, out_bytes, 2, dest_of)[:4]
    model = N.Store(2, SLOT)
    want = N.sequential(model, rows, topics, kinds, events, sender, 3, out_bytes)
    assert want[5] == (2, 0, 0, 2 * len(b"room 0 says hello"), 3)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        store, ret = eng.to_device(np.zeros(2 * SLOT, np.uint8)), eng.to_device(np.zeros(2 * 16, np.uint8))
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        eng.route(2, ndest, dest_of)
        eng.retain(store, SLOT, ret)
        got, topic, reply = eng.retain_table()
        assert ([tuple(int(x) for x in r) for r in got.tolist()], topic.tolist(), reply.tolist()) == want[:3]
        f, c = eng.segment_retain(3)
        assert (f.tolist(), c.tolist()) == want[3:5] and eng.retain_totals() == want[5]
        assert bytes(store.download(2 * SLOT)) == model.store_bytes()
        assert [tuple(int(x) for x in e) for e in ret.download(32).view(libhv_amd.RETAINED_DTYPE).tolist()] == model.entries()
        eng.sync()
        for b in (rx, out, store, ret):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_retain_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0], (before, inside)
