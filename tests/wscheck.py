"""Oracle for hvws_check and hvws_replies_checked (include/hvws.h): the rules
restated in plain Python over the frame records of wsharness.scan_segment, the
pieces and bytes of wsrfc.rfc_batch and the verdicts of wsutf8.fold; a driver
that chains batches, threading every kind of per-connection state and counting
frames and messages so that a verdict can be named by its place in the stream;
the named streams both test files run; and the reply rule as a filter over
wsrfc.replies_of.

A helper, not a test module."""
from __future__ import annotations

import random
import struct
from typing import List, Optional, Sequence, Tuple

import numpy as np

import wsmsg as M
import wsrfc as R
import wssend as S
import wsutf8 as U
import wsvalidate as V

C_HEADER, C_SEQUENCE, C_CLOSE_BODY, C_CLOSE_UTF8, C_TEXT_UTF8, C_SIZE = 1, 2, 4, 8, 16, 32
C_ALL = 63
CLASSES = (C_HEADER, C_SEQUENCE, C_CLOSE_BODY, C_CLOSE_UTF8, C_TEXT_UTF8, C_SIZE)
CODE = {C_HEADER: 1002, C_SEQUENCE: 1002, C_CLOSE_BODY: 1002, C_CLOSE_UTF8: 1007, C_TEXT_UTF8: 1007, C_SIZE: 1009}
CK_OPEN, CK_FAILED = 1, 2
NONE = (1 << 64) - 1
RF_CLOSED = S.RF_CLOSED
RF_FAILED = 4
I_INVALID, I_VSHIFT = 1 << 14, 16
FIN, MASK = M.FIN, M.MASK
MIB = 1 << 20


def code_of(why: int) -> int:
    """The close code of the lowest set class bit; 0 when nothing failed."""
    for c in CLASSES:
        if why & c:
            return CODE[c]
    return 0


def close_code_ok(code: int) -> bool:
    return 1000 <= code <= 1003 or 1007 <= code <= 1011 or 3000 <= code <= 4999


def record_bits(info: int, length: int, is_open: int, classes: int, max_message: int) -> Tuple[int, int]:
    """One record -> (classes violated there, the open bit after it)."""
    bits, op = 0, info & 0xF
    if info & I_INVALID:
        bits |= C_HEADER
    if info & M.I_HDR and op <= 2:
        if (not is_open) if op == 0 else is_open:
            bits |= C_SEQUENCE
        is_open = 0 if info & FIN else 1
    if max_message and info & M.I_HDR and op < 8 and length > max_message:
        bits |= C_SIZE
    return bits & classes, is_open


def piece_bits(piece, out: bytes, classes: int, max_message: int) -> int:
    info, ln, off = int(piece["info"]), int(piece["len"]), int(piece["off"])
    if not info & R.M_CTL:
        return C_SIZE & classes if max_message and ln > max_message else 0
    if not info & M.M_END or info & 0xF != 8 or ln == 0:
        return 0
    if ln == 1 or ln > 125:
        return C_CLOSE_BODY & classes
    body = out[off:off + ln]
    bits = 0 if close_code_ok(struct.unpack(">H", body[:2])[0]) else C_CLOSE_BODY
    if ln > 2 and U.run(U.ACCEPT, body[2:]) != U.ACCEPT:
        bits |= C_CLOSE_UTF8
    return bits & classes


def check_batch(infos: Sequence[Sequence[int]], lengths: Sequence[Sequence[int]], firsts: Sequence[int], table,
                out: bytes, state_in=None, classes: int = C_ALL, max_message: int = 0, u8_bad=None):
    """One batch -> (state_out, fail_rec, why, code), one entry per segment.
    infos / lengths: per segment, its records' info (HVWS_I_INVALID included)
    and full frame length; firsts: each segment's first record index; table /
    out: the pieces and bytes of rfc_batch; u8_bad: wsutf8's bad[] per segment."""
    nseg = len(infos)
    st_out, fail, why, code = [], [], [], []
    pieces = [[] for _ in range(nseg)]
    for p in table:
        pieces[int(p["seg"])].append(p)
    for s in range(nseg):
        word = int(state_in[s]) if state_in is not None else 0
        assert not word & ~(CK_OPEN | CK_FAILED)
        if word & CK_FAILED:
            st_out.append(CK_FAILED), fail.append(firsts[s]), why.append(0), code.append(0)
            continue
        found = {}
        is_open = word & CK_OPEN
        for i, (info, length) in enumerate(zip(infos[s], lengths[s])):
            bits, is_open = record_bits(int(info), int(length), is_open, classes, max_message)
            if bits:
                found[firsts[s] + i] = found.get(firsts[s] + i, 0) | bits
        for p in pieces[s]:
            bits = piece_bits(p, out, classes, max_message)
            if bits:
                rec = firsts[s] if int(p["rec"]) == R.NOREC else int(p["rec"])
                found[rec] = found.get(rec, 0) | bits
        if classes & C_TEXT_UTF8 and u8_bad is not None and int(u8_bad[s]) != NONE:
            found[int(u8_bad[s])] = found.get(int(u8_bad[s]), 0) | C_TEXT_UTF8
        if found:
            f = min(found)
            st_out.append(CK_FAILED), fail.append(f), why.append(found[f]), code.append(code_of(found[f]))
        else:
            st_out.append(is_open), fail.append(NONE), why.append(0), code.append(0)
    return (np.array(st_out, np.uint32), np.array(fail, np.uint64), np.array(why, np.uint32),
            np.array(code, np.uint16))


def replies_checked_of(table, nseg: int, policy: int, fail_rec, closed_in=None):
    """hvws_replies_checked: wsrfc.replies_of with the replies to pieces at or
    after their connection's fail_rec taken out, and RF_FAILED | RF_CLOSED for a
    failed connection."""
    rep, answered, _, flags = R.replies_of(table, nseg, policy, closed_in)
    keep = [k for k, i in enumerate(answered) if int(table[i]["rec"]) < int(fail_rec[int(table[i]["seg"])])]
    rep, answered = [rep[k] for k in keep], [answered[k] for k in keep]
    first, count = [0] * nseg, [0] * nseg
    for s in range(nseg):
        mine = [k for k, i in enumerate(answered) if int(table[i]["seg"]) == s]
        count[s] = len(mine)
        first[s] = mine[0] if mine else sum(1 for i in answered if int(table[i]["seg"]) < s)
    flags = [f | (RF_FAILED | RF_CLOSED if int(fail_rec[s]) != NONE else 0) for s, f in enumerate(flags)]
    return rep, answered, (first, count), flags


class Want:
    """What one batch must give: rfc = rfc_batch's result, u8 = (state_out, bad),
    verdict = check_batch's, firsts = each segment's first record index."""

    def __init__(self, rfc, infos, lengths, firsts, u8, verdict):
        self.rfc, self.infos, self.lengths, self.firsts, self.u8, self.verdict = rfc, infos, lengths, firsts, u8, verdict


class Checked:
    """`nconn` connections over batches (wsrfc.Chain's reads), each with its
    parser carry, hvws_rfc_state, hvws_utf8 word and hvws_check word.  vmask: the
    hvws_set_validation classes the scans run under.  failed[c]: None, or
    (frame ordinal, data message ordinal, code, why) of the connection's first
    failure, the ordinals counted from the start of its stream."""

    def __init__(self, nconn: int, classes: int = C_ALL, max_message: int = 0, vmask: int = 0):
        self.n, self.classes, self.max_message, self.vmask = nconn, classes, max_message, vmask
        self.ch = R.Chain(nconn)
        self.u8 = np.zeros(nconn, np.uint32)
        self.ck = np.zeros(nconn, np.uint32)
        self.stream = [b""] * nconn
        self.hdrs = [0] * nconn    # headers completed so far
        self.ends = [0] * nconn    # frames completed so far
        self.msgs = [0] * nconn    # data messages completed so far
        self.failed: List[Optional[Tuple[int, int, int, int]]] = [None] * nconn
        self.sticky_ok = True

    def conns(self, reads):
        return [c for c in range(self.n) if reads[c] is not None]

    def oracle(self, reads: Sequence[Optional[bytes]]) -> Want:
        data, segs, conns, carries, st = self.ch.inputs(reads)
        rfc = R.rfc_batch(data, segs, carries, st, self.ch.prev)
        recs, _, u8_out, bad, firsts, _ = U.oracle_batch(data, segs, carries, self.u8[conns])
        ends = list(firsts[1:]) + [len(recs)]
        infos, lengths = [], []
        for i, c in enumerate(conns):
            mine = recs[firsts[i]:ends[i]]
            info = [int(x) for x in mine["info"]] if len(mine) else []
            if self.vmask:   # the k-th completed header of the stream is the k-th frame's
                viol = V.violations(self.stream[c] + reads[c])
                k = self.hdrs[c]
                for j, x in enumerate(info):
                    if x & M.I_HDR:
                        v = viol[k][1] & self.vmask
                        if v:
                            info[j] = x | I_INVALID | (v << I_VSHIFT)
                        k += 1
            infos.append(info)
            lengths.append([int(x) for x in mine["length"]] if len(mine) else [])
        verdict = check_batch(infos, lengths, firsts, rfc[1], rfc[0], self.ck[conns], self.classes, self.max_message, bad)
        return Want(rfc, infos, lengths, firsts, (u8_out, bad), verdict)

    def take(self, want: Want, reads: Sequence[Optional[bytes]]) -> None:
        conns = self.conns(reads)
        st_out, fail, why, code = want.verdict
        for i, c in enumerate(conns):
            info = want.infos[i]
            if self.failed[c] is not None:
                self.sticky_ok = self.sticky_ok and int(st_out[i]) == CK_FAILED and int(fail[i]) == want.firsts[i]
            elif int(fail[i]) != NONE:
                upto = info[: int(fail[i]) - want.firsts[i]]
                self.failed[c] = (self.ends[c] + sum(1 for x in upto if x & M.I_END),
                                  self.msgs[c] + sum(1 for x in upto if R.klass(x) == 0 and x & M.I_END and x & FIN),
                                  int(code[i]), int(why[i]))
            self.hdrs[c] += sum(1 for x in info if x & M.I_HDR)
            self.ends[c] += sum(1 for x in info if x & M.I_END)
            self.msgs[c] += sum(1 for x in info if R.klass(x) == 0 and x & M.I_END and x & FIN)
            self.stream[c] += reads[c]
            self.u8[c] = want.u8[0][i]
            self.ck[c] = st_out[i]
        self.ch.take(want.rfc, reads)

    def run(self, reads: Sequence[Optional[bytes]]) -> Want:
        want = self.oracle(reads)
        self.take(want, reads)
        return want


def feed(stream: bytes, chunks: Sequence[int], classes: int = C_ALL, max_message: int = 0, vmask: int = 0) -> Checked:
    """One stream cut into single-segment batches of the given sizes -> the chain after the last."""
    ck = Checked(1, classes, max_message, vmask)
    at = 0
    for n in chunks:
        n = min(n, len(stream) - at)
        ck.run([stream[at:at + n]])
        at += n
    assert at == len(stream)
    return ck


# ---- the named streams ---------------------------------------------------------

KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
K2 = bytes([9, 8, 7, 6])


def B(frames) -> bytes:
    import wsharness as H

    return H.build_frames_ref([(fl | MASK, body, KEY if i % 2 == 0 else K2) for i, (fl, body) in enumerate(frames)])


def close(code: int, reason: bytes = b"bye"):
    return (8 | FIN, struct.pack(">H", code) + reason)


class Stream:
    """A named stream, the settings it runs under, and what must come of it:
    want = None (clean) or (ordinal of the failing frame, close code); by_piece:
    the failure is the size class's by-piece form, whose frame depends on the
    cuts (compare the data message's ordinal, `msg`)."""

    def __init__(self, name, data, want, vmask=0, max_message=0, by_piece=False, msg=0, why=None):
        self.name, self.data, self.want, self.vmask, self.max_message = name, data, want, vmask, max_message
        self.by_piece, self.msg, self.why = by_piece, msg, why


def table() -> List[Stream]:
    ping = (9 | FIN, b"ping")
    huge = bytes([0x82, 0xFF]) + struct.pack(">Q", 1 << 40) + KEY   # a 2^40-byte binary frame's header
    t = [
        Stream("lone_continue", B([(0 | FIN, b"x")]), (0, 1002), why=C_SEQUENCE),
        Stream("text_then_text", B([(1, b"a"), (1 | FIN, b"b")]), (1, 1002), why=C_SEQUENCE),
        Stream("text_ping_continue", B([(1, b"AB"), ping, (0 | FIN, b"CD")]), None),
        Stream("continue_after_complete", B([(1 | FIN, b"a"), ping, (0 | FIN, b"b")]), (2, 1002), why=C_SEQUENCE),
        Stream("close_empty", B([(1 | FIN, b"a"), (8 | FIN, b"")]), None),
        Stream("close_one_byte", B([ping, (8 | FIN, b"\x03")]), (1, 1002), why=C_CLOSE_BODY),
    ]
    for code in (999, 1004, 1005, 1006, 1012, 1015, 2999, 5000):
        t.append(Stream(f"close_{code}", B([(2 | FIN, b"bin"), close(code)]), (1, 1002), why=C_CLOSE_BODY))
    for code in (1000, 1011, 3000, 4999):
        t.append(Stream(f"close_{code}", B([(2 | FIN, b"bin"), close(code, "café €".encode())]), None))
    t += [
        Stream("close_reason_cut", B([ping, close(1000, "going €".encode()[:-1])]), (1, 1007), why=C_CLOSE_UTF8),
        Stream("close_126_bytes", B([(1 | FIN, b"a"), close(1000, b"r" * 124)]), (1, 1002), vmask=V.V_CONTROL),
        Stream("text_overlong", B([(1, b"ok "), ping, (0 | FIN, b"\xc0\xaf")]), (2, 1007), why=C_TEXT_UTF8),
        Stream("huge_header", B([(1 | FIN, b"small")]) + huge, (1, 1009), max_message=MIB, why=C_SIZE),
        Stream("three_fragments_cross", B([(2 | FIN, b"one"), (1, b"aaaa"), (0, b"bbbb"), ping, (0 | FIN, b"cccc")]),
               (4, 1009), max_message=10, by_piece=True, msg=1),
        Stream("two_in_one_frame", B([(1 | FIN, b"a"), (0 | FIN, b"twelve bytes")]), (1, 1002), max_message=10,
               why=C_SEQUENCE | C_SIZE),
        Stream("second_violation_ignored", B([(1 | FIN, b"\xc0\xaf"), (0 | FIN, b"lone"), (8 | FIN, b"\x03")]), (0, 1007),
               why=C_TEXT_UTF8),
    ]
    return t


# ---- seeded streams --------------------------------------------------------------

def gen_stream(seed: int, clean: int = 6, dirty: int = 6) -> Tuple[bytes, int]:
    """A clean prefix of `clean` messages (valid text, binary, pings and pongs
    between fragments: wsutf8.gen_frames), then `dirty` frames each of which may
    break a header rule (wsvalidate.make_frame), carry random bytes as text, come
    out of sequence or be a Close of any kind -> (wire bytes, frames of the prefix)."""
    import wsharness as H

    r = random.Random(seed)
    frames, _ = U.gen_frames(seed, clean, 24, True, 0.0)
    wire = H.build_frames_ref(frames)
    for _ in range(dirty):
        u = r.random()
        if u < 0.4:
            wire += V.make_frame(r, 0.4, 160)[0]
        elif u < 0.7:
            body = r.choice([b"", b"\x03", close(r.choice([1000, 1001, 1005, 3000, 999]))[1],
                             close(1000, bytes(r.randrange(256) for _ in range(r.randint(1, 6))))[1]])
            wire += H.build_frames_ref([(8 | FIN | MASK, body, KEY)])
        else:
            op = r.choice([0, 1, 2])
            body = r.choice(U.POOL).encode() * r.randint(0, 3)
            wire += H.build_frames_ref([(op | (FIN if r.random() < 0.6 else 0) | MASK, body, K2)])
    return wire, len(frames)


def gen_fragmented(seed: int, nmsg: int = 8, max_bytes: int = 40) -> bytes:
    """Well-formed traffic only (no violation but the size class's): binary and
    valid text messages in 1 .. 4 fragments with pings and pongs between them."""
    import wsharness as H

    return H.build_frames_ref(U.gen_frames(seed, nmsg, max_bytes, True, 0.0)[0])
