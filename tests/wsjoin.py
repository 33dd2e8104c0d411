"""Oracle for hvws_messages_joined (include/hvws.h): wsmsg.oracle_batch with
each segment's carried bytes -- a range of the previous batch's output -- laid
ahead of the segment's payload bytes, the piece and carry rules of the joined
form applied, and a driver that chains batches over two alternating buffers,
threading each connection's parser carry, message state and carry offset.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

import wsmsg as M

NOREC = (1 << 64) - 1


def joined_batch(data: bytes, segs, carries=None, state_in=None, prev: bytes = b"", prev_off=None):
    """One batch -> (out bytes, pieces [MSG_DTYPE], (first, count) per segment,
    state_out [MSG_STATE_DTYPE], carry offset per segment, parser carries out)."""
    out0, tab0, (f0, c0), st_out, carry_out = M.oracle_batch(data, segs, carries, state_in, with_carry=True)
    md, _ = M._dtypes()
    out = bytearray()
    pieces: List[tuple] = []
    firsts, counts, carry_off = [], [], []
    for s in range(len(segs)):
        pend, opcode, opened = (int(x) for x in state_in[s]) if state_in is not None else M.FRESH
        firsts.append(len(pieces))
        start = len(out)
        if pend:
            o = int(prev_off[s])
            assert 0 <= o and o + pend <= len(prev), "a carried range leaves the previous output"
            out += prev[o:o + pend]
        mine = tab0[int(f0[s]): int(f0[s]) + int(c0[s])]
        if len(mine) == 0 and pend:   # no records: the carried bytes are one open piece
            assert opened
            pieces.append((start, pend, pend, NOREC, s, (opcode or 8) | M.M_CONT))
        for i, p in enumerate(mine):
            off, ln = int(p["off"]), int(p["len"])
            out += out0[off:off + ln]
            if i == 0:   # begins at the carried bytes
                pieces.append((start, ln + pend, ln + pend, int(p["rec"]), s, int(p["info"])))
                assert int(p["total"]) == ln + pend
            else:
                pieces.append((len(out) - ln, ln, ln, int(p["rec"]), s, int(p["info"])))
                assert int(p["total"]) == ln
        counts.append(len(pieces) - firsts[-1])
        carry_off.append(pieces[-1][0] if counts[-1] and int(st_out["pending"][s]) else 0)
        if int(st_out["pending"][s]):   # the trailing open piece holds exactly what is pending
            assert counts[-1] and pieces[-1][1] == int(st_out["pending"][s]) and not pieces[-1][5] & M.M_END
    table = np.zeros(len(pieces), dtype=md)
    for i, p in enumerate(pieces):
        table[i] = p
    return (bytes(out), table, (np.array(firsts, np.uint64), np.array(counts, np.uint64)), st_out,
            np.array(carry_off, np.uint64), carry_out)


class Chain:
    """`nconn` connections, every one a segment of every batch (an empty read is
    a segment of length 0).  inputs() lays a batch out and gives what
    hvws_messages_joined takes besides the buffers; take() threads a batch's
    results on.  prev: the previous batch's output (the other buffer)."""

    def __init__(self, nconn: int):
        self.n = nconn
        self.carry: List[Optional[object]] = [None] * nconn
        self.state = M.states([M.FRESH] * nconn)
        self.off = np.zeros(nconn, np.uint64)
        self.prev = b""
        self.logs: List[List[Tuple[int, bytes]]] = [[] for _ in range(nconn)]
        self.batches = 0
        self.spans = [0] * nconn        # batches the open message has lain in
        self.max_span = 0
        self.totals_ok = True

    def inputs(self, reads: Sequence[bytes]):
        assert len(reads) == self.n
        segs, at = [], 0
        for r in reads:
            segs.append((at, len(r)))
            at += len(r)
        return b"".join(reads), segs

    def oracle(self, reads: Sequence[bytes]):
        data, segs = self.inputs(reads)
        return joined_batch(data, segs, self.carry, self.state, self.prev, self.off)

    def take(self, res) -> None:
        out, table, (first, count), st, off, carry = res
        for p in table:
            s = int(p["seg"])
            if int(p["total"]) != int(p["len"]):
                self.totals_ok = False
            if int(p["info"]) & M.M_END:
                self.logs[s].append((int(p["info"]) & 0xF, out[int(p["off"]): int(p["off"]) + int(p["len"])]))
        for s in range(self.n):   # max_span: the most batches a completed message lay in
            mine = table[int(first[s]): int(first[s]) + int(count[s])]
            if len(mine) == 0:
                self.spans[s] += 1 if int(st["open"][s]) else 0
                continue
            span = self.spans[s] + 1 if int(mine[0]["info"]) & M.M_CONT else 1
            if int(mine[0]["info"]) & M.M_END:
                self.max_span = max(self.max_span, span)
            if not int(st["open"][s]):
                self.spans[s] = 0
            else:
                self.spans[s] = span if len(mine) == 1 else 1
        self.carry, self.state, self.off, self.prev = list(carry), st, off, out
        self.batches += 1

    def run(self, reads: Sequence[bytes]):
        res = self.oracle(reads)
        self.take(res)
        return res


def mixed_frames(rng, nf: int, p_close: float = 0.04, max_len: int = 300):
    """Frames of one connection: text, binary, pings, pongs, a few closes,
    fragmented messages with control frames between the fragments."""
    out = []
    for _ in range(nf):
        x = rng.random()
        op = 8 if x < p_close else 9 if x < 0.3 else rng.choice([0, 0, 1, 1, 2, 2, 10, 3])
        n = rng.choice([0, 1, rng.randrange(126), rng.randrange(max_len + 1)])
        fl = op | (M.FIN if rng.random() < 0.7 else 0) | (0 if rng.random() < 0.1 else M.MASK)
        out.append((fl, rng.randbytes(n), bytes(rng.randrange(256) for _ in range(4))))
    return out


def run_stream(data: bytes, chunks: Sequence[int]):
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
