"""Message-reassembly oracle for hvws_messages (include/hvws.h): the
reference's message rule (WebSocketParser::FeedRecvData, quirks included)
restated over the frame records of wsharness.scan_segment, one record at a
time, with the output layout, the piece table and the carried state the
header describes.  tests/test_messages_oracle.py pins it to the reference's
own message layer.

A helper, not a test module."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

I_HDR, I_BODY, I_END = 1 << 10, 1 << 11, 1 << 12
FIN, MASK = 0x10, 0x20
M_END, M_CONT = 1 << 4, 1 << 5
FRESH = (0, 0, 0)   # (pending, opcode, open)


def _dtypes():
    import libhv_amd

    return libhv_amd.MSG_DTYPE, libhv_amd.MSG_STATE_DTYPE


def states(seq: Sequence[Tuple[int, int, int]]) -> np.ndarray:
    """[(pending, opcode, open)] -> MSG_STATE_DTYPE array."""
    _, sd = _dtypes()
    a = np.zeros(len(seq), dtype=sd)
    for i, (p, o, n) in enumerate(seq):
        a[i] = (p, o, n)
    return a


def oracle_batch(data: bytes, segs, carries=None, state_in=None, with_carry: bool = False):
    """One batch -> (out bytes, pieces [MSG_DTYPE], (first, count) per segment,
    state_out [MSG_STATE_DTYPE]); with_carry: the parser carries out as a fifth."""
    import wsharness as H

    md, _ = _dtypes()
    out = bytearray()
    pieces: List[tuple] = []
    firsts, counts, st_out, carry_out = [], [], [], []
    rec_base = 0
    for s, (off, n) in enumerate(segs):
        recs, carry, _, plain = H.scan_segment(data[off:off + n], carries[s] if carries is not None else None)
        carry_out.append(carry)
        pend_in, latch, open_in = (int(x) for x in state_in[s]) if state_in is not None else FRESH
        firsts.append(len(pieces))
        start, first_piece, closed_at = len(out), True, None

        def close(i: int, end: bool) -> None:
            nonlocal start, first_piece
            ln = len(out) - start
            info = (latch or 8) | (M_END if end else 0) | (M_CONT if first_piece and open_in else 0)
            pieces.append((start, ln, ln + (pend_in if first_piece else 0), rec_base + i, s, info))
            start, first_piece = len(out), False

        for i, r in enumerate(recs):
            info = int(r["info"])
            if info & I_HDR and info & 0xF:
                latch = info & 0xF
            o, ln = int(r["pay_off"]), int(r["pay_len"])
            out += plain[o:o + ln]
            if info & I_END and info & FIN:
                close(i, True)
                closed_at = i
        if len(recs) and closed_at != len(recs) - 1:   # the trailing open piece
            close(len(recs) - 1, False)
            st_out.append((pieces[-1][2], latch, 1))
        elif len(recs):
            st_out.append((0, latch, 0))
        else:
            st_out.append((pend_in, latch, open_in))
        counts.append(len(pieces) - firsts[-1])
        rec_base += len(recs)
    table = np.zeros(len(pieces), dtype=md)
    for i, p in enumerate(pieces):
        table[i] = p
    res = (bytes(out), table, (np.array(firsts, np.uint64), np.array(counts, np.uint64)), states(st_out))
    return res + (carry_out,) if with_carry else res


class Joiner:
    """Concatenates one connection's pieces across batches, as a caller of
    hvws_messages would: -> the onMessage log [(opcode, bytes)]."""

    def __init__(self):
        self.msgs: List[Tuple[int, bytes]] = []
        self.cur = bytearray()
        self.totals_ok = True

    def feed(self, out: bytes, pieces) -> None:
        for p in pieces:
            self.cur += out[int(p["off"]): int(p["off"]) + int(p["len"])]
            if int(p["total"]) != len(self.cur):
                self.totals_ok = False
            if int(p["info"]) & M_END:
                self.msgs.append((int(p["info"]) & 0xF, bytes(self.cur)))
                self.cur = bytearray()


def run_stream(data: bytes, chunks: Sequence[int]):
    """One stream cut into single-segment batches of the given sizes, the
    parser carry and the message state threaded through -> (log, joiner)."""
    j = Joiner()
    carry, st = None, states([FRESH])
    at = 0
    for n in chunks:
        if at >= len(data):
            break
        n = min(n, len(data) - at)
        out, pieces, _, st, carries = oracle_batch(data[at:at + n], [(0, n)], [carry] if carry is not None else None,
                                                   st, with_carry=True)
        carry = carries[0]
        j.feed(out, pieces)
        at += n
    return j.msgs, j


def edge_bounds(tile: int) -> Tuple[int, int]:
    """Two multiples of the tile behind edge_frames' first frame of 66000 bytes."""
    m = 66000 // tile + 2
    return m * tile, (m + 2) * tile


def edge_frames(tile: int, seed: int = 5) -> List[Tuple[int, bytes, Optional[bytes]]]:
    """Frames whose record boundaries fall, in the output, at every offset from
    25 before to 25 after the two multiples of `tile` in edge_bounds (so from 17
    before to 17 after even when up to 7 payload bytes of the first frame stayed
    in an earlier batch), with every header length (2, 4, 6, 8, 10, 14).  The
    first frame is masked, has a 14-byte header and spans whole tiles."""
    r = random.Random(seed)
    frames: List[Tuple[int, bytes, Optional[bytes]]] = []

    def add(n: int, masked: bool, fin: bool = True, op: int = 2) -> None:
        key = bytes(r.randrange(1, 256) for _ in range(4)) if masked else None
        frames.append((op | (FIN if fin else 0) | (MASK if masked else 0), r.randbytes(n), key))

    assert 2 * tile <= 66000
    total = 0
    for b in edge_bounds(tile):
        # up to 25 before the boundary: frames of every header form
        fill = b - 25 - total
        sizes = [66000, 300, 131, 127, 126, 125, 77, 33, 7, 3, 1]
        k = 0
        while fill > 0:
            n = next(x for x in sizes if x <= fill)
            add(n, masked=(k % 3 != 2), fin=(k % 4 != 1), op=(1, 2, 0, 9)[k % 4])
            fill -= n
            total += n
            k += 1
        for j in range(50):   # one-byte records: a boundary at every offset b - 25 .. b + 25
            add(1, masked=(j % 2 == 0), fin=(j % 5 != 0))
            total += 1
            if j % 7 == 3:
                add(0, masked=True)
    add(66000, False)   # 10-byte header; whole tiles inside an unmasked record
    add(4001, True)
    return frames
