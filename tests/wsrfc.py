"""Oracle for hvws_messages_rfc (include/hvws.h): the records of
wsharness.scan_segment filtered into the data class and the control class, and
wsjoin's piece and carry rules applied to each class as a connection of its
own -- per connection the carried data bytes, the data payloads, the carried
control bytes, the control payloads -- with a driver that chains batches over
two alternating buffers, threading each connection's parser carry and
hvws_rfc_state, and the reply rule hvws_replies follows after that call.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

import wsmsg as M

NOREC = (1 << 64) - 1
M_CTL = 1 << 6
FRESH = ((0, 0, 0), (0, 0, 0), 0, 0)   # (data, ctl, data_off, ctl_off)


def _dtype():
    import libhv_amd

    return libhv_amd.RFC_STATE_DTYPE


def states(seq) -> np.ndarray:
    """[((pending, opcode, open), (pending, opcode, open), data_off, ctl_off)] -> RFC_STATE_DTYPE array."""
    a = np.zeros(len(seq), dtype=_dtype())
    for i, (d, c, do, co) in enumerate(seq):
        a[i] = (d, c, do, co)
    return a


def klass(info: int) -> int:
    """0: a data record, 1: a control record, 2: neither (its header is incomplete)."""
    if not info & (M.I_HDR | M.I_BODY | M.I_END):
        return 2
    return 1 if (info & 0xF) >= 8 else 0


def rfc_batch(data: bytes, segs, carries=None, state_in=None, prev: bytes = b""):
    """One batch -> (out bytes, pieces [MSG_DTYPE], (first, count) per segment,
    state_out [RFC_STATE_DTYPE], parser carries out)."""
    import wsharness as H

    md, _ = M._dtypes()
    out = bytearray()
    pieces: List[tuple] = []
    firsts, counts, st_out, carry_out = [], [], [], []
    rec_base = 0
    for s, (off, n) in enumerate(segs):
        recs, carry, _, plain = H.scan_segment(data[off:off + n], carries[s] if carries is not None else None)
        carry_out.append(carry)
        firsts.append(len(pieces))
        new = []
        for k, name in ((0, "data"), (1, "ctl")):
            if state_in is not None:
                pend, latch, open_in = (int(x) for x in state_in[name][s])
                poff = int(state_in[name + "_off"][s])
            else:
                pend, latch, open_in, poff = 0, 0, 0, 0
            none = 8 if k else 0            # nothing latched: Q6 is the control class's only
            start, first_piece = len(out), True
            if pend:
                assert open_in and 0 <= poff and poff + pend <= len(prev), "a carried range leaves the previous output"
                out += prev[poff:poff + pend]
            mine = [(i, r) for i, r in enumerate(recs) if klass(int(r["info"])) == k]
            closed_last = False
            for i, r in mine:
                info = int(r["info"])
                if info & M.I_HDR and info & 0xF:
                    latch = info & 0xF
                o, ln = int(r["pay_off"]), int(r["pay_len"])
                out += plain[o:o + ln]
                closed_last = bool(info & M.I_END and (info & M.FIN or k))
                if closed_last or i == mine[-1][0]:
                    ln = len(out) - start
                    pieces.append((start, ln, ln, rec_base + i, s, (latch or none) | (M.M_END if closed_last else 0)
                                   | (M.M_CONT if first_piece and open_in else 0) | (M_CTL if k else 0)))
                    if closed_last:
                        start, first_piece = len(out), False
            if not mine:
                if pend:   # no records: the carried bytes are one open piece
                    pieces.append((start, pend, pend, NOREC, s, (latch or none) | M.M_CONT | (M_CTL if k else 0)))
                new.append(((pend, latch, open_in), start if pend else 0))
            elif closed_last:
                new.append(((0, latch, 0), 0))
            else:
                ln = len(out) - start
                new.append(((ln, latch, 1), start if ln else 0))
        st_out.append((new[0][0], new[1][0], new[0][1], new[1][1]))
        counts.append(len(pieces) - firsts[-1])
        rec_base += len(recs)
    table = np.zeros(len(pieces), dtype=md)
    for i, p in enumerate(pieces):
        table[i] = p
    return (bytes(out), table, (np.array(firsts, np.uint64), np.array(counts, np.uint64)), states(st_out), carry_out)


def messages_of(out: bytes, table) -> List[Tuple[int, int, int, bytes]]:
    """The whole messages of one batch in stream order: [(seg, is control, opcode, bytes)]."""
    done = sorted((p for p in table if int(p["info"]) & M.M_END), key=lambda p: int(p["rec"]))
    return [(int(p["seg"]), 1 if int(p["info"]) & M_CTL else 0, int(p["info"]) & 0xF,
             out[int(p["off"]): int(p["off"]) + int(p["len"])]) for p in done]


class Chain:
    """`nconn` connections over batches.  A batch's reads: one bytes per
    connection (b"" = an empty read, a segment of length 0) or None = left out
    of the batch (only a connection with nothing pending may be: its bytes lie
    in a buffer this driver does not keep).  prev: the previous batch's output."""

    def __init__(self, nconn: int):
        self.n = nconn
        self.carry: List[Optional[object]] = [None] * nconn
        self.state = states([FRESH] * nconn)
        self.prev = b""
        self.data_log: List[List[Tuple[int, bytes]]] = [[] for _ in range(nconn)]
        self.ctl_log: List[List[Tuple[int, bytes]]] = [[] for _ in range(nconn)]
        self.merged: List[List[Tuple[int, bytes]]] = [[] for _ in range(nconn)]
        self.batches = 0
        self.totals_ok = True

    def inputs(self, reads: Sequence[Optional[bytes]]):
        """-> (batch bytes, segments, the connections in it, their carries, their states)."""
        assert len(reads) == self.n
        conns = [c for c in range(self.n) if reads[c] is not None]
        for c in range(self.n):
            if reads[c] is None:
                assert not int(self.state["data"]["pending"][c]) and not int(self.state["ctl"]["pending"][c])
        segs, at = [], 0
        for c in conns:
            segs.append((at, len(reads[c])))
            at += len(reads[c])
        return (b"".join(reads[c] for c in conns), segs, conns, [self.carry[c] for c in conns],
                self.state[conns].copy())

    def oracle(self, reads: Sequence[Optional[bytes]]):
        data, segs, conns, carries, st = self.inputs(reads)
        return rfc_batch(data, segs, carries, st, self.prev)

    def take(self, res, reads: Sequence[Optional[bytes]]) -> None:
        out, table, _, st, carry = res
        conns = [c for c in range(self.n) if reads[c] is not None]
        for p in table:
            if int(p["total"]) != int(p["len"]):
                self.totals_ok = False
        for seg, ctl, op, body in messages_of(out, table):
            c = conns[seg]
            (self.ctl_log if ctl else self.data_log)[c].append((op, body))
            self.merged[c].append((op, body))
        for i, c in enumerate(conns):
            self.carry[c] = carry[i]
            self.state[c] = st[i]
        self.prev = out
        self.batches += 1

    def run(self, reads: Sequence[Optional[bytes]]):
        res = self.oracle(reads)
        self.take(res, reads)
        return res


def run_stream(data: bytes, chunks: Sequence[int]) -> Chain:
    """One stream cut into single-segment batches of the given sizes (0 allowed)
    -> the chain after the last batch."""
    ch = Chain(1)
    at = 0
    for n in chunks:
        n = min(n, len(data) - at)
        ch.run([data[at:at + n]])
        at += n
    assert at == len(data)
    return ch


def replies_of(table, nseg: int, policy: int, closed_in=None):
    """hvws_replies after hvws_messages_rfc over one batch's pieces -> (replies
    [(off, len, flags, key)], the piece each answers, (first, count) per
    segment, flags per segment).  Close is final by stream order: with c the
    segment's selected CLOSE piece of the smallest rec, only pieces with
    rec < rec(c), and c itself, are answered; nothing is ever deferred."""
    import wssend as S

    sel = [S.reply_op(int(p["info"]) & 0xF, policy) if int(p["info"]) & M.M_END else 0 for p in table]
    closed = [bool(closed_in[s]) if closed_in is not None else False for s in range(nseg)]
    close_at = [None] * nseg   # (rec, piece) of c
    for i, p in enumerate(table):
        s, rec = int(p["seg"]), int(p["rec"])
        if sel[i] == 8 and not closed[s] and (close_at[s] is None or rec < close_at[s][0]):
            close_at[s] = (rec, i)
    replies, answered = [], []
    first, count = [0] * nseg, [0] * nseg
    cur = 0
    for i, p in enumerate(table):
        s, rec = int(p["seg"]), int(p["rec"])
        while cur <= s:
            first[cur] = len(replies)
            cur += 1
        if not sel[i] or closed[s]:
            continue
        if close_at[s] is None or rec < close_at[s][0] or i == close_at[s][1]:
            assert int(p["total"]) == int(p["len"])
            replies.append((int(p["off"]), int(p["len"]), sel[i] | S.FIN, 0))
            answered.append(i)
            count[s] += 1
    while cur < nseg:
        first[cur] = len(replies)
        cur += 1
    flags = [S.RF_CLOSED if closed[s] or close_at[s] is not None else 0 for s in range(nseg)]
    return replies, answered, (first, count), flags
