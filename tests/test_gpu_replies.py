"""GPU: hvws_replies -- the server's onMessage dispatch
(http/server/HttpHandler.cpp:174-200) over the piece table of hvws_messages --
against tests/wssend.py's rule over wsmsg.oracle_batch's pieces (and, for fresh
streams, over the reference's own onMessage log), and the whole server turn:
scan -> messages -> replies -> hvws_send_messages(d_n = the reply count on the
device), whose output must be the reference-built reply frames segment by
segment."""
from __future__ import annotations

import random

import numpy as np
import pytest

import libhv_amd
import streams
import wsharness as H
import wsmsg
import wssend as S

pytestmark = pytest.mark.gpu

FIN, MASK = S.FIN, S.MASK
IMPL = "ref" if H.have_ref() else "oracle"
POLICIES = [S.R_SERVER, S.R_SERVER | S.R_ECHO, 0]


def _stream(rng: random.Random, nf: int, p_close: float = 0.04):
    """Frames of one connection: text, binary, pings, pongs, a few closes,
    fragmented messages with control frames between the fragments.  Every
    third stream is streams.rand_frames' (all opcodes alike, reserved ones
    too: closes are frequent there)."""
    if rng.randrange(3) == 0:
        return H.build_frames_ref(streams.rand_frames(rng, nf, 300))
    out = []
    for _ in range(nf):
        x = rng.random()
        if x < p_close:
            op = 8
        elif x < 0.3:
            op = 9
        else:
            op = rng.choice([0, 0, 1, 1, 2, 2, 10, 3])
        L = rng.choice([0, 1, rng.randrange(126), rng.randrange(300)])
        fl = op | (FIN if rng.random() < 0.7 else 0) | (0 if rng.random() < 0.1 else MASK)
        out.append((fl, rng.randbytes(L), bytes(rng.randrange(256) for _ in range(4))))
    return H.build_frames_ref(out)


def _batch(streams_):
    data, segs = bytearray(), []
    for s in streams_:
        segs.append((len(data), len(s)))
        data += s
    return bytes(data), segs


class Turn:
    """One context's device buffers for a batch of at most `cap` bytes."""

    def __init__(self, eng, cap):
        self.eng, self.cap = eng, cap
        self.rx, self.msg, self.out = eng.alloc(cap + 64), eng.alloc(cap + 64), eng.alloc(2 * cap + 4096)
        self.moff = None

    def free(self):
        for b in (self.rx, self.msg, self.out, self.moff):
            if b is not None:
                b.free()

    def receive(self, data, segs, carries=None, state_in=None, step=False):
        """scan (or step) + messages, no host read in between."""
        eng, L = self.eng, libhv_amd.lib()
        self.rx.upload(np.frombuffer(data, np.uint8)) if data else None
        s, c = eng._segs(segs), eng._carry(len(segs), carries)
        fn = L.hvws_step if step else L.hvws_scan
        assert fn(eng.ctx, self.rx.ptr, len(data), s, c, len(segs)) == 0
        eng.messages(self.rx, len(data), not step, self.msg, self.cap, state_in)

    def send(self, fragment=0):
        """hvws_send_messages over the reply table, its count read on the device."""
        eng = self.eng
        table, d_n, n = eng.replies_device()
        if self.moff is None or self.moff.nbytes < 8 * (n + 1):
            if self.moff is not None:
                self.moff.free()
            self.moff = eng.alloc(8 * (n + 1))
        return eng.send_messages(self.out, self.out.nbytes, self.msg, self.cap, table, n, d_n, fragment, False,
                                 self.moff)


def _expect(data, segs, policy, carries=None, state_in=None, closed_in=None):
    out, pieces, _, st, carry = wsmsg.oracle_batch(data, segs, carries, state_in, with_carry=True)
    rep, answered, fc, flags = S.replies_of_pieces(pieces, len(segs), policy, closed_in)
    return out, pieces, rep, answered, fc, flags, st, carry


def _check_replies(eng, out, pieces, rep, answered, fc, flags, nseg):
    got_pieces = eng.message_table()
    assert got_pieces.tolist() == pieces.tolist()
    table, piece = eng.reply_table()
    assert [tuple(int(x) for x in r) for r in table.tolist()] == rep
    assert piece.tolist() == answered
    first, count = eng.segment_replies(nseg)
    assert (first.tolist(), count.tolist()) == (fc[0], fc[1])
    assert eng.reply_flags(nseg).tolist() == flags
    assert libhv_amd.lib().hvws_reply_count(eng.ctx) == len(rep)


def _check_turn(t: Turn, out, rep, fc, fragment=0):
    """The send's output, through d_msg_off, is each segment's reference-built
    reply frames."""
    nbytes, nfr = t.send(fragment)
    msgs = [(fl, out[o:o + n], 0) for o, n, fl, _ in rep]
    want, woffs, wfr = S.expected(msgs, fragment, False)
    assert (nbytes, nfr) == (len(want), wfr)
    got = bytes(t.out.download(nbytes))
    moff = t.moff.download(8 * (len(rep) + 1), np.uint64).tolist()
    assert moff == woffs
    for s, (f, c) in enumerate(zip(*fc)):
        assert got[moff[f]:moff[f + c]] == S.expected(msgs[f:f + c], fragment, False)[0], s
    assert got == want


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("nseg", [1, 3, 64])
def test_replies_fresh_batches(eng, nseg, policy):
    """Fresh connections, one batch; some segments hold no bytes.  Against the
    rule over the oracle's pieces and over the reference's onMessage log."""
    rng = random.Random(nseg * 8 + policy)
    ss = [b"" if nseg > 1 and i % 7 == 2 else _stream(rng, rng.randrange(1, 30)) for i in range(nseg)]
    data, segs = _batch(ss)
    t = Turn(eng, len(data))
    try:
        t.receive(data, segs)
        eng.replies(policy)
        out, pieces, rep, answered, fc, flags, _, _ = _expect(data, segs, policy)
        _check_replies(eng, out, pieces, rep, answered, fc, flags, nseg)
        if policy == 0:
            assert rep == [] and flags == [0] * nseg
        for s, stream in enumerate(ss):    # the reference's own message layer + the rule
            msgs = H.run_messages(IMPL, stream, [max(len(stream), 1)])[0]
            want, closed = S.replies_of_messages(msgs, policy)
            f, c = fc[0][s], fc[1][s]
            assert [(fl, out[o:o + n]) for o, n, fl, _ in rep[f:f + c]] == want, s
            assert flags[s] == (S.RF_CLOSED if closed else 0), s
        _check_turn(t, out, rep, fc)
    finally:
        t.free()


@pytest.mark.parametrize("policy", POLICIES[:2])
@pytest.mark.parametrize("nseg", [3, 64])
def test_replies_with_state_carried_in(eng, nseg, policy):
    """Two batches of the same connections, cut at random bytes: parser carry,
    message state and the closed flag carried over; the second batch's first
    pieces complete messages of the first (deferred)."""
    rng = random.Random(nseg + 100 * policy)
    ss = [_stream(rng, rng.randrange(2, 30), p_close=0.02) for _ in range(nseg)]
    cut = [rng.randrange(len(s) + 1) if i % 5 else 0 for i, s in enumerate(ss)]   # some first halves are empty
    d1, g1 = _batch([s[:c] for s, c in zip(ss, cut)])
    d2, g2 = _batch([s[c:] for s, c in zip(ss, cut)])
    t = Turn(eng, max(len(d1), len(d2)))
    try:
        t.receive(d1, g1)
        eng.replies(policy)
        out, pieces, rep, answered, fc, flags, st, carry = _expect(d1, g1, policy)
        _check_replies(eng, out, pieces, rep, answered, fc, flags, nseg)
        _check_turn(t, out, rep, fc)
        closed = [f & S.RF_CLOSED for f in flags]
        t.receive(d2, g2, carry, st)          # the same context: tables reused
        eng.replies(policy, closed)
        out, pieces, rep, answered, fc, flags2, _, _ = _expect(d2, g2, policy, carry, st, closed)
        _check_replies(eng, out, pieces, rep, answered, fc, flags2, nseg)
        assert all(f2 & S.RF_CLOSED for f, f2 in zip(flags, flags2) if f & S.RF_CLOSED)
        if nseg == 64:
            assert any(f & S.RF_DEFERRED for f in flags2)
        _check_turn(t, out, rep, fc, fragment=50)
    finally:
        t.free()


def test_close_in_the_middle_and_closed_in(eng):
    k = bytes([1, 2, 3, 4])
    B = H.build_frames_ref
    a = B([(9 | FIN | MASK, b"one", k), (1 | FIN | MASK, b"text", k), (8 | FIN | MASK, b"\x03\xe8", k),
           (9 | FIN | MASK, b"late", k), (8 | FIN | MASK, b"again", k)])
    b = B([(9 | FIN | MASK, b"p", k)])
    data, segs = _batch([a, b, b, a])
    t = Turn(eng, len(data))
    try:
        t.receive(data, segs)
        for policy, closed_in in ((S.R_SERVER | S.R_ECHO, None), (S.R_SERVER | S.R_ECHO, [0, 1, 0, 1]),
                                  (S.R_PONG, None), (S.R_SERVER, [0, 0, 0, 0])):
            eng.replies(policy, closed_in)
            out, pieces, rep, answered, fc, flags, _, _ = _expect(data, segs, policy, closed_in=closed_in)
            _check_replies(eng, out, pieces, rep, answered, fc, flags, 4)
            _check_turn(t, out, rep, fc)
        # the first case by hand
        eng.replies(S.R_SERVER | S.R_ECHO)
        table, _ = eng.reply_table()
        assert [int(x) for x in table["flags"]] == [10 | FIN, 1 | FIN, 8 | FIN, 10 | FIN, 10 | FIN, 10 | FIN,
                                                   1 | FIN, 8 | FIN]
        assert eng.reply_flags(4).tolist() == [S.RF_CLOSED, 0, 0, S.RF_CLOSED]
    finally:
        t.free()


def test_deferred_ping_and_deferred_close(eng):
    k = bytes([9, 8, 7, 6])
    B = H.build_frames_ref
    s0 = B([(0 | FIN | MASK, b"tail", k), (9 | FIN | MASK, b"own", k)])
    s1 = B([(0 | FIN | MASK, b"bye", k), (9 | FIN | MASK, b"late", k)])
    data, segs = _batch([s0, s1])
    st = wsmsg.states([(5, 9, 1), (2, 8, 1)])
    t = Turn(eng, len(data))
    try:
        t.receive(data, segs, None, st)
        eng.replies(S.R_SERVER)
        out, pieces, rep, answered, fc, flags, _, _ = _expect(data, segs, S.R_SERVER, None, st)
        assert flags == [S.RF_DEFERRED, S.RF_DEFERRED | S.RF_CLOSED] and answered == [1]
        _check_replies(eng, out, pieces, rep, answered, fc, flags, 2)
        _check_turn(t, out, rep, fc)
    finally:
        t.free()


def test_replies_need_messages():
    with libhv_amd.Engine(0) as e:
        with pytest.raises(libhv_amd.HvwsError, match="without a preceding hvws_messages") as ei:
            e.replies(S.R_SERVER)
        assert "(-2)" in str(ei.value)
        assert e.replies_device() == (None, None, 0)


def test_turn_after_step_and_twice(eng):
    """The turn after hvws_step (payloads already unmasked, masked = 0), twice
    on one context with batches of different sizes (tables reused)."""
    rng = random.Random(77)
    t = Turn(eng, 1 << 18)
    try:
        for nseg, fragment in ((40, 0), (5, 20), (64, 0)):
            ss = [_stream(rng, rng.randrange(1, 12), p_close=0.03) for _ in range(nseg)]
            data, segs = _batch(ss)
            assert len(data) <= t.cap
            policy = S.R_SERVER | S.R_ECHO
            t.receive(data, segs, step=True)
            eng.replies(policy)
            out, pieces, rep, answered, fc, flags, _, _ = _expect(data, segs, policy)
            _check_turn(t, out, rep, fc, fragment)     # first: nothing read between receive and send
            _check_replies(eng, out, pieces, rep, answered, fc, flags, nseg)
    finally:
        t.free()
