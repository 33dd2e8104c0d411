"""GPU: the server turn after hvws_messages_rfc -- hvws_replies(SERVER | ECHO)
and hvws_send_messages -- against the reply rule restated in tests/wsrfc.py and
frames built by tests/wssend.py.  The Q5 stream yields an echo and a PONG;
"close is final" goes by stream order across the two classes; closed_in; no
reply is ever deferred over a chain whose reads cut PINGs and CLOSEs; and the
turn after hvws_messages_joined equals the existing oracle."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wsjoin as J
import wsmsg as M
import wsrfc as R
import wssend as S

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
K2 = bytes([9, 8, 7, 6])
POLICY = S.R_SERVER | S.R_ECHO
CAP = 2048
B = H.build_frames_ref


def _frames(msgs) -> bytes:
    """Server frames of [(flags, bytes)], as the reference builds them."""
    return S.expected([(fl, d, 0) for fl, d in msgs], 0, False)[0]


class Turns:
    """A chain of server turns: scan, hvws_messages_rfc, hvws_replies,
    hvws_send_messages; every batch's tables against the oracles, each
    connection's sent bytes collected."""

    def __init__(self, eng, nconn: int):
        self.eng, self.n = eng, nconn
        self.ch = R.Chain(nconn)
        self.outs = [eng.alloc(CAP + 64), eng.alloc(CAP + 64)]
        self.tx = eng.alloc(2 * CAP)
        self.moff = eng.alloc(8 * 1024)
        self.closed = [0] * nconn
        self.sent = [b""] * nconn
        self.prev_len = 0
        self.flags_seen = 0

    def turn(self, row, closed_in=None):
        eng, ch, k = self.eng, self.ch, self.ch.batches
        assert all(r is not None for r in row)
        closed = self.closed if closed_in is None else closed_in
        data, segs, _, carries, st = ch.inputs(row)
        want = ch.oracle(row)
        rep, answered, fc, flags = R.replies_of(want[1], self.n, POLICY, closed)
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        cur, old = self.outs[k % 2], self.outs[(k + 1) % 2]
        try:
            eng.scan(rx, len(data), segs, carries)
            eng.messages_rfc(rx, len(data), True, cur, CAP, st, old if k else None, self.prev_len)
            eng.replies(POLICY, closed)
            table, d_n, n = eng.replies_device()
            assert n + 1 <= 1024   # moff holds the table's capacity
            nbytes, _ = eng.send_messages(self.tx, 2 * CAP, cur, CAP, table, n, d_n, 0, False, self.moff)
            assert eng.message_table().tolist() == want[1].tolist(), k
            got_table, piece = eng.reply_table()
            assert [tuple(int(x) for x in r) for r in got_table.tolist()] == rep, k
            assert piece.tolist() == answered, k
            first, count = eng.segment_replies(self.n)
            assert (first.tolist(), count.tolist()) == (fc[0], fc[1]), k
            got_flags = eng.reply_flags(self.n).tolist()
            assert got_flags == flags, k
            for f in got_flags:
                self.flags_seen |= f
            offs = self.moff.download(8 * (len(rep) + 1), np.uint64).tolist()
            got = bytes(self.tx.download(nbytes)) if nbytes else b""
            out = want[0]
            assert got == _frames([(fl, out[o:o + ln]) for o, ln, fl, _ in rep]), k
            batch = []
            for s in range(self.n):
                batch.append(got[offs[int(first[s])]: offs[int(first[s]) + int(count[s])]])
                self.sent[s] += batch[-1]
            self.closed = [1 if f & S.RF_CLOSED else 0 for f in got_flags]
        finally:
            eng.sync()
            rx.free()
        ch.take(want, row)
        self.prev_len = len(want[0])
        return batch

    def free(self):
        for b in self.outs + [self.tx, self.moff]:
            b.free()


def test_q5_stream_is_an_echo_and_a_pong(eng):
    t = Turns(eng, 1)
    try:
        sent = t.turn([B([(1 | MASK, b"AB", KEY), (9 | FIN | MASK, b"PING", KEY), (0 | FIN | MASK, b"CD", KEY)])])
        assert sent[0] == _frames([(1 | FIN, b"ABCD"), (10 | FIN, b"PING")])
        assert t.closed == [0]
    finally:
        t.free()


def test_close_is_final_by_stream_order(eng):
    """One batch.  0: a text completes after the CLOSE frame, a PING lies before
    it and one after it.  1: an echo, a PONG and the CLOSE, all answered.  2:
    closed on the way in.  3: two CLOSE frames, a PING between them."""
    s0 = B([(1 | MASK, b"hello ", KEY), (9 | FIN | MASK, b"early", K2), (8 | FIN | MASK, b"\x03\xe8bye", KEY),
            (9 | FIN | MASK, b"late", K2), (0 | FIN | MASK, b"world", KEY), (2 | FIN | MASK, b"after", K2)])
    s1 = B([(1 | FIN | MASK, b"x", KEY), (2 | MASK, b"bin", K2), (9 | FIN | MASK, b"p", KEY), (0 | FIN | MASK, b"ary", K2),
            (8 | FIN | MASK, b"", KEY)])
    s2 = B([(1 | FIN | MASK, b"unheard", KEY), (9 | FIN | MASK, b"unanswered", K2)])
    s3 = B([(8 | FIN | MASK, b"\x03\xe9first", KEY), (9 | FIN | MASK, b"between", K2), (8 | FIN | MASK, b"second", KEY)])
    t = Turns(eng, 4)
    try:
        sent = t.turn([s0, s1, s2, s3], closed_in=[0, 0, 1, 0])
        assert sent[0] == _frames([(10 | FIN, b"early"), (8 | FIN, b"\x03\xe8bye")])
        assert sent[1] == _frames([(1 | FIN, b"x"), (2 | FIN, b"binary"), (10 | FIN, b"p"), (8 | FIN, b"")])
        assert sent[2] == b""
        assert sent[3] == _frames([(8 | FIN, b"\x03\xe9first")])
        # the CLOSE is the last frame of its connection's range
        assert sent[0].endswith(_frames([(8 | FIN, b"\x03\xe8bye")])) and sent[1].endswith(_frames([(8 | FIN, b"")]))
        assert t.closed == [1, 1, 1, 1]
        # the messages themselves were all delivered: only the replies stop
        assert t.ch.data_log[0] == [(1, b"hello world"), (2, b"after")]
        assert [op for op, _ in t.ch.ctl_log[0]] == [9, 8, 9]
        # a closed connection stays closed in its next batch
        sent = t.turn([B([(9 | FIN | MASK, b"again", KEY)])] + [b""] * 3)
        assert sent == [b""] * 4 and t.closed == [1, 1, 1, 1]
    finally:
        t.free()


def test_nothing_is_deferred_when_reads_cut_pings_and_closes(eng):
    """Three connections over four batches: a PING of 100 bytes in 3 reads; a
    text of 3 fragments with a PING between them in 4; a CLOSE cut in two inside
    a fragmented binary message that completes after it."""
    ping = B([(9 | FIN | MASK, bytes(range(100)), KEY), (1 | FIN | MASK, b"after the ping", K2)])
    text = B([(1 | MASK, b"A" * 40, KEY), (0 | MASK, b"B" * 30, K2), (9 | FIN | MASK, b"PING", KEY),
              (0 | FIN | MASK, b"C" * 50, K2), (2 | FIN | MASK, b"bin", KEY)])
    close = B([(2 | MASK, b"first", KEY), (8 | FIN | MASK, b"\x03\xe8 going away now", K2),
               (0 | FIN | MASK, b" and last", KEY), (9 | FIN | MASK, b"late", K2)])
    cuts = [[30, 80, len(ping)],
            [20, 60, 6 + 40 + 6 + 30 + 6 + 2, len(text)],
            [6 + 5 + 6 + 7, len(close)]]
    ss = [ping, text, close]
    reads = []
    for k in range(4):
        row = []
        for s, c in zip(ss, cuts):
            a = c[k - 1] if 0 < k <= len(c) else (0 if k == 0 else len(s))
            b = c[k] if k < len(c) else len(s)
            row.append(s[a:b])
        reads.append(row)
    assert all(b"".join(r[i] for r in reads) == ss[i] for i in range(3))
    t = Turns(eng, 3)
    try:
        for row in reads:
            t.turn(row)
        assert not t.flags_seen & S.RF_DEFERRED and t.ch.totals_ok
        # a batch's data replies come before its control replies
        assert t.sent[0] == _frames([(1 | FIN, b"after the ping"), (10 | FIN, bytes(range(100)))])
        assert t.sent[1] == _frames([(1 | FIN, b"A" * 40 + b"B" * 30 + b"C" * 50), (2 | FIN, b"bin"), (10 | FIN, b"PING")])
        assert t.sent[2] == _frames([(8 | FIN, b"\x03\xe8 going away now")])
        assert t.closed == [0, 0, 1]
        assert t.ch.data_log[2] == [(2, b"first and last")]
    finally:
        t.free()


def test_the_turn_after_the_joined_form_is_unchanged(eng):
    """The same batch through hvws_messages_joined: Q5 and Q6 as before, close
    by piece order, against the existing oracle (tests/wssend.py)."""
    s0 = B([(1 | MASK, b"hello ", KEY), (9 | FIN | MASK, b"early", K2), (8 | FIN | MASK, b"\x03\xe8bye", KEY),
            (9 | FIN | MASK, b"late", K2), (0 | FIN | MASK, b"world", KEY)])
    s1 = B([(0 | FIN | MASK, b"lone continuation", KEY), (1 | MASK, b"AB", KEY), (9 | FIN | MASK, b"PING", KEY),
            (0 | FIN | MASK, b"CD", KEY)])
    data, segs = J.Chain(2).inputs([s0, s1])
    want = J.joined_batch(data, segs)
    rep, answered, fc, flags = S.replies_of_pieces(want[1], 2, POLICY, None)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = eng.alloc(CAP)
    try:
        eng.scan(rx, len(data), segs)
        eng.messages_joined(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        assert eng.message_table().tolist() == want[1].tolist()
        table, piece = eng.reply_table()
        assert [tuple(int(x) for x in r) for r in table.tolist()] == rep
        assert piece.tolist() == answered
        first, count = eng.segment_replies(2)
        assert (first.tolist(), count.tolist()) == (fc[0], fc[1])
        assert eng.reply_flags(2).tolist() == flags
        # Q5: the PONGs carry the fragments; Q6: the lone CONTINUE is a CLOSE
        got = [(int(r["flags"]), want[0][int(r["off"]): int(r["off"]) + int(r["len"])]) for r in table]
        assert got == [(10 | FIN, b"hello early"), (8 | FIN, b"\x03\xe8bye"), (8 | FIN, b"lone continuation")]
        # and the rfc form on the same batch answers the lone CONTINUE with nothing
        eng.messages_rfc(rx, len(data), True, out, CAP)
        eng.replies(POLICY)
        rt = R.rfc_batch(data, segs)
        table, _ = eng.reply_table()
        got = [(int(r["flags"]), rt[0][int(r["off"]): int(r["off"]) + int(r["len"])]) for r in table]
        assert got == [(10 | FIN, b"early"), (8 | FIN, b"\x03\xe8bye"), (1 | FIN, b"ABCD"), (10 | FIN, b"PING")]
    finally:
        eng.sync()
        rx.free()
        out.free()
