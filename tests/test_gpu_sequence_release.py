"""GPU: tests/test_gpu_ctx_release.py's property for hvws_sequence and
hvws_envelope_sequenced -- a destroyed context that ran them (the pairs, the
sort, the head scan, the numbers, the counters, the getters, the sequenced
envelope with the enveloped fan-out and the enveloped retain behind it) holds no
device and no pinned bytes.  The tables of each cycle are compared with
tests/wssequence.py, so the cycle is known to have run what it claims."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import wsenvelope as E
import wsfan as W
import wsharness as H
import wsmsg as M
import wsretain as N
import wsrfc as R
import wsroute as T
import wssend as S
import wssequence as Q
from test_gpu_route_release import held

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO
SLOT = 64


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    row = [H.build_frames_ref([(1 | FIN | MASK, b"P%d\nroom %d says hello" % (c % 2, c), KEY), (9 | FIN | MASK, b"p", KEY),
                               (2 | FIN | MASK, b"S%d\n" % (c % 2), KEY)]) for c in range(3)]
    dest_of, ndest = [0, 1, 200], 201
    subs = [[0, 200], [1]]
    seeds = [9, (1 << 64) - 2]
    data, segs, _, _, _ = R.Chain(3).inputs(row)
    out_bytes, pieces = R.rfc_batch(data, segs)[:2]
    rep, answered, _, _ = R.replies_of(pieces, 3, POLICY)
    sender = W.senders(pieces, answered)
    rows, topics, kinds, events = T.route(rep, sender, out_bytes, 2, dest_of)[:4]
    seq, after, totals = Q.sequential(seeds, topics, kinds)
    assert totals == (3, 2) and after == {0: 11, 1: (1 << 64) - 1}
    rows2, env_bytes, placed, etotals = Q.envelope_sequential(rows, topics, kinds, sender, dest_of, out_bytes, seq,
                                                              E.ENV_SENDER)
    assert etotals[:2] == (3, 3)
    model = N.Store(2, SLOT)
    snap = N.sequential(model, E.retain_rows(rows2, rows, kinds), topics, kinds, events, sender, 3, bytes(env_bytes))
    fan = T.fanout_routed(rows2, topics, sender, subs, ndest, dest_of)
    first, member = W.flatten(subs)
    with libhv_amd.Engine(0) as eng:
        rx, out = eng.to_device(np.frombuffer(data, np.uint8)), eng.alloc(CAP + 64)
        store, ret = eng.to_device(np.zeros(2 * SLOT, np.uint8)), eng.to_device(np.zeros(2 * 16, np.uint8))
        df, dm = eng.to_device(first), eng.to_device(member)
        ctr = eng.to_device(np.array(seeds, np.uint64))
        eng.scan(rx, len(data), segs)
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        eng.route(2, ndest, dest_of)
        eng.sequence(ctr)
        assert eng.sequence_table().tolist() == seq and eng.sequence_totals() == totals
        assert ctr.download(16).view(np.uint64).tolist() == [after[0], after[1]]
        env_cap = eng.envelope_sequenced_bound()
        assert env_cap == Q.bound(CAP, int(libhv_amd.lib().hvws_reply_capacity(eng.ctx)))
        env = eng.to_device(np.zeros(env_cap, np.uint8))
        eng.envelope_sequenced(env, env_cap, libhv_amd.ENV_SENDER)
        assert [tuple(int(x) for x in r) for r in eng.envelope_table().tolist()] == rows2
        assert eng.envelope_totals() == etotals
        assert bytes(env.download(etotals[3])) == bytes(env_bytes)
        assert eng.fanout_enveloped(df, dm, len(member)) == len(fan[0])
        assert [tuple(int(x) for x in r) for r in eng.fanout_table()[0].tolist()] == fan[0]
        eng.retain_enveloped(store, SLOT, ret)
        got, topic, reply = eng.retain_table()
        assert ([tuple(int(x) for x in r) for r in got.tolist()], topic.tolist(), reply.tolist()) == snap[:3]
        assert bytes(store.download(2 * SLOT)) == model.store_bytes()
        eng.sync()
        for b in (rx, out, store, ret, df, dm, ctr, env):
            b.free()
        return held()


def test_a_destroyed_context_that_ran_sequence_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    assert after == before, (before, inside, after)
    assert inside[0] > before[0], (before, inside)
