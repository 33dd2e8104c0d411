"""Cases and the checker for tests/test_gpu_passes_paths.py: the passes that
read the frame table -- hvws_utf8, hvws_messages, hvws_messages_joined,
hvws_messages_rfc and, through the last, hvws_replies / hvws_send_messages --
behind every scan path.

Every expectation is the CPU oracles' (wsutf8, wsmsg, wsjoin, wsrfc, wssend,
wsharness.scan_segment); none is taken from a GPU run.  The generators build
batches whose shape sends the scan down one path; tests/test_passes_cases.py
proves on the CPU that the cases are what they claim.

Frames come from wsjoin.mixed_frames -- fragments, PINGs between fragments,
CLOSEs, unmasked and zero-length frames -- with the data opcodes made a legal
sequence (a CONTINUE exactly while a data message is open): hvws_utf8 restarts
a text message at a new text header and skips the reserved opcodes, the message
rule appends, so only over legal sequences do the two agree on what "the text
message" is, which check 5 of check_passes (the join of hvws_msg.rec with
bad[s]) stands on.  Text payloads come from wsutf8.gen_frames.

A helper, not a test module; the GPU binding is imported where it is used."""
from __future__ import annotations

import functools
import hashlib
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

import streams
import wsharness as H
import wsjoin as J
import wsmsg as M
import wsrfc as R
import wssend as S
import wsutf8 as U

FIN, MASK = M.FIN, M.MASK
SENTINEL, SLACK = 0xA5, 64
POLICY = S.R_SERVER | S.R_ECHO
NOREC = R.NOREC
KEY = b"\x11\x22\x33\x44"


# ------------------------------------------------------------------ frames

@functools.lru_cache(maxsize=None)
def _texts(seed: int, bad: float) -> Tuple[bytes, ...]:
    """The text messages of wsutf8.gen_frames(seed), fragments joined."""
    frames, _ = U.gen_frames(seed, 160, bad=bad)
    out, cur = [], None
    for fl, payload, _ in frames:
        op = fl & 0xF
        if op >= 8:
            continue
        if op:
            cur = bytearray() if op == 1 else None
        if cur is not None:
            cur += payload
            if fl & FIN:
                out.append(bytes(cur))
                cur = None
    assert len(out) > 50
    return tuple(out)


def conn_frames(seed: int, nf: int, max_len: int = 300, bad: float = 0.45, clean: bool = False,
                p_close: float = 0.04, legal: bool = True):
    """One connection's frames [(flags, payload, key)]: wsjoin.mixed_frames
    with a legal data opcode sequence and text payloads from wsutf8.gen_frames
    (one to three of its messages joined, cut into the message's fragments at
    random bytes, empty fragments included).  clean: only frames the sieve's
    plausibility filter passes -- masked, opcodes 0-2 / 8-10, control frames
    FIN and at most 125 bytes.  legal=False: wsjoin.mixed_frames as they come
    -- a new text or binary header inside an open message, lone continuations,
    random payloads as text."""
    rng = random.Random(seed)
    raw = J.mixed_frames(rng, nf, p_close=p_close, max_len=max_len)
    if not legal:
        return raw
    texts = _texts(seed, bad)
    out, groups, is_open = [], [], False
    for fl, payload, key in raw:
        op = fl & 0xF
        if clean:
            fl |= MASK
            if op >= 8:
                fl |= FIN
                payload = payload[:125]
        if op < 8:
            if is_open:
                op2 = 0
            else:
                op2 = op if op in (1, 2, 3) else rng.choice([1, 2])
                if clean and op2 == 3:
                    op2 = 2
                groups.append((op2, []))
            groups[-1][1].append(len(out))
            is_open = not fl & FIN
            fl = (fl & ~0xF) | op2
        out.append([fl, payload, key])
    ti = 0
    for op, idx in groups:
        if op != 1:
            continue
        k = rng.choice([1, 1, 1, 3])
        t = b"".join(texts[(ti + j) % len(texts)] for j in range(k))
        ti += k
        cuts = sorted(rng.randint(0, len(t)) for _ in range(len(idx) - 1))
        for i, a, b in zip(idx, [0] + cuts, cuts + [len(t)]):
            out[i][1] = t[a:b]
    return [tuple(f) for f in out]


def headers(data: bytes) -> List[Tuple[int, int]]:
    """(first header byte, first payload byte) of every frame of a stream of whole frames."""
    recs = H.scan_segment(data)[0]
    assert np.all(recs["info"] & M.I_HDR) and np.all(recs["info"] & M.I_END)
    return [(int(r["hdr_off"]), int(r["pay_off"])) for r in recs]


def layout(parts: Sequence[bytes], rng: random.Random) -> Tuple[bytes, List[Tuple[int, int]]]:
    """One segment per part, gaps of 0-16 bytes (random, no scan may touch them) between."""
    buf, segs = bytearray(), []
    for p in parts:
        buf += rng.randbytes(rng.randint(0, 16))
        segs.append((len(buf), len(p)))
        buf += p
    buf += rng.randbytes(rng.randint(0, 16))
    return bytes(buf), segs


class Case:
    """Connections (streams of whole frames), each cut once: batches[0] holds
    [0, cut) of every connection, batches[1] the rest, whole the uncut streams."""

    def __init__(self, conns: Sequence[bytes], cuts: Sequence[int], seed: int, raw: Sequence[int] = ()):
        self.conns, self.cuts, self.raw = list(conns), list(cuts), tuple(raw)   # raw: connections of illegal sequences
        rng = random.Random(seed)
        self.batches = [layout([c[:k] for c, k in zip(conns, cuts)], rng),
                        layout([c[k:] for c, k in zip(conns, cuts)], rng)]
        self.whole = layout(conns, rng)

    def cuts_in_header(self) -> int:
        return sum(any(a < k < b for a, b in headers(c)) for c, k in zip(self.conns, self.cuts))


# ---------------------------------------------------------------- the cases

RAW1 = (6, 17, 24, 33)


@functools.lru_cache(maxsize=None)
def case1(seed: int = 1) -> Case:
    """40 mixed connections of 40 frames, payloads of 0-300 bytes; odd ones cut
    inside a header, the others at a random byte; one read ends with its stream
    (an empty second segment).  Even connections have invalid text among
    theirs, odd ones only valid text.  Four connections (RAW1) keep
    wsjoin.mixed_frames' illegal opcode sequences: every check but the join of
    rec with bad[s] runs on them."""
    rng = random.Random(7000 + seed)
    conns, cuts = [], []
    for i in range(40):
        data = H.build_frames_ref(conn_frames(1000 * seed + i, 40, 300, bad=0.45 if i % 2 == 0 else 0.0,
                                              legal=i not in RAW1))
        if i == 38:
            cut = len(data)
        elif i % 2:
            a, b = rng.choice(headers(data))
            cut = a + rng.randint(1, b - a - 1)
        else:
            cut = rng.randrange(1, len(data))
        conns.append(data)
        cuts.append(cut)
    return Case(conns, cuts, 7100 + seed, RAW1)


def _text200(rng: random.Random, n: int, mutate: bool) -> bytes:
    """n bytes of text from wsutf8.POOL, padded with ASCII; mutate: one byte from wsutf8.MUTATIONS."""
    text = ""
    while len(text.encode()) < n:
        text += rng.choice(U.POOL)
    while len(text.encode()) > n:
        text = text[1:]
    p = text.encode()
    p += b"." * (n - len(p))
    if mutate:
        j = rng.randrange(n)
        p = p[:j] + bytes([rng.choice(U.MUTATIONS)]) + p[j + 1:]
    return p


@functools.lru_cache(maxsize=None)
def case2(seed: int = 1) -> Case:
    """32 connections of 48 whole masked frames of 208 bytes (200-byte payloads:
    a text, a binary, a text in two fragments, again and again; every third text
    of an even connection is invalid), cut inside a frame -- odd connections
    inside its header."""
    rng = random.Random(7200 + seed)
    conns, cuts = [], []
    for i in range(32):
        frames, nt = [], 0
        while len(frames) < 48:
            for kind in ("text", "binary", "split"):
                if kind == "binary":
                    frames.append((2 | FIN | MASK, rng.randbytes(200), rng.randbytes(4)))
                    continue
                nt += 1
                t = _text200(rng, 200 if kind == "text" else 400, i % 2 == 0 and nt % 3 == 0)
                if kind == "text":
                    frames.append((1 | FIN | MASK, t, rng.randbytes(4)))
                else:
                    frames.append((1 | MASK, t[:200], rng.randbytes(4)))
                    frames.append((0 | FIN | MASK, t[200:], rng.randbytes(4)))
        data = H.build_frames_ref(frames[:48])
        a, b = headers(data)[rng.randrange(20, 29)]
        cuts.append(a + rng.randint(1, b - a - 1) if i % 2 else b + rng.randrange(1, 200))
        conns.append(data)
    return Case(conns, cuts, 7300 + seed)


@functools.lru_cache(maxsize=None)
def case3(seed: int = 1):
    """(thin, dense): 16 segments of 2 frames, and the same with 200 tiny frames in segment 7."""
    parts = [H.build_frames_ref(conn_frames(3000 * seed + s, 2, 60)) for s in range(16)]
    dense = list(parts)
    dense[7] = H.build_frames_ref(conn_frames(3100 * seed, 200, 9))
    rng = random.Random(7400 + seed)
    return layout(parts, rng), layout(dense, rng)


@functools.lru_cache(maxsize=None)
def case4_checked(seed: int = 1) -> bytes:
    """One stream of about 2.8 MiB of about 1 KiB frames: its record bound,
    len / 2 + 3, exceeds the table a fresh context sizes from its first guess
    (Overflow.FIRST_TABLE records), so the device checks the count against that
    table; its few thousand records fit."""
    return H.build_frames_ref(conn_frames(4000 + seed, 2900, 11000, bad=0.003, p_close=0.001))


class Overflow:
    """The stream of test_gpu_parity.test_single_segment_table_overflow, longer:
    n whole FIN frames, 80 % of them 2-byte unmasked empty binary frames, the
    rest masked ASCII text of at most 9 bytes.  1.4 M of them: the table a fresh
    context allocates for its first guess of 2^20 records has a quarter of room
    on top (ensure_frames), so only more than 1.25 * 2^20 = 1 310 720 records
    overflow it -- 1.2 M fit, and take the checked-and-accepted form.  Every
    record is a complete message, so expect(k) gives what hvws_utf8 and
    hvws_messages must return for the first k frames from the frame list alone."""

    # Records the first one-stream table of a context holds: scan_single's guess kSingleMin = 2^20 and the
    # quarter ensure_frames adds (libhv_amd/csrc/hvws_engine.cpp).  If either changes, this must follow, or
    # the overflow and checked cases quietly fall back to the other forms.
    FIRST_TABLE = (5 << 20) // 4

    def __init__(self, n: int = 1_400_000, seed: int = 8):
        rng = np.random.default_rng(seed)
        self.n = n
        self.is_text = rng.random(n) >= 0.8
        self.lens = np.where(self.is_text, rng.integers(0, 10, n), 0).astype(np.uint64)
        self.chars = rng.integers(0x20, 0x7F, int(self.lens.sum()), dtype=np.uint8)
        tl = self.lens[self.is_text].astype(np.int64)
        toff = np.concatenate([[0], np.cumsum(tl)])
        cb = self.chars.tobytes()
        blob = np.frombuffer(H.build_frames_ref([(1 | FIN | MASK, cb[toff[i]:toff[i + 1]], KEY) for i in range(len(tl))]),
                             np.uint8)
        empty = H.build_frames_ref([(2 | FIN, b"", None)])
        assert len(empty) == 2 and len(blob) == int(tl.sum()) + 6 * len(tl)
        size = np.where(self.is_text, self.lens.astype(np.int64) + 6, 2)
        self.off = np.concatenate([[0], np.cumsum(size)])
        wire = np.empty(int(self.off[-1]), np.uint8)
        e = self.off[:-1][~self.is_text]
        wire[e], wire[e + 1] = empty[0], empty[1]
        boff = np.concatenate([[0], np.cumsum(tl + 6)])[:-1]
        wire[np.repeat(self.off[:-1][self.is_text] - boff, tl + 6) + np.arange(len(blob))] = blob
        self.wire = wire
        # the unmasked batch: each text frame's payload bytes are its characters
        self.plain = wire.copy()
        poff = self.off[:-1][self.is_text] + 6
        self.plain[np.repeat(poff - toff[:-1], tl) + np.arange(len(self.chars))] = self.chars

    @functools.lru_cache(maxsize=2)
    def expect(self, k: Optional[int] = None):
        """-> (out bytes, pieces, (first, count), msg state, words, utf8 state, bad) of the first k frames."""
        k = self.n if k is None else k
        md, _ = M._dtypes()
        lens = self.lens[:k]
        ends = np.cumsum(lens)
        table = np.zeros(k, md)
        table["off"], table["len"], table["total"] = ends - lens, lens, lens
        table["rec"] = np.arange(k, dtype=np.uint64)
        ops = np.where(self.is_text[:k], 1, 2).astype(np.uint32)
        table["info"] = ops | np.uint32(M.M_END)
        words = np.where(lens > 0, np.uint32(0xFFFFFFF0), np.uint32(U.IDENTITY)).astype(np.uint32)
        return (self.chars[:int(ends[-1])].tobytes(), table, (np.array([0], np.uint64), np.array([k], np.uint64)),
                M.states([(0, int(ops[-1]), 0)]), words, np.array([0], np.uint32), np.array([U.NONE], np.uint64))


@functools.lru_cache(maxsize=None)
def overflow() -> Overflow:
    return Overflow()


@functools.lru_cache(maxsize=None)
def case4_sieved(seed: int = 1):
    """(clean, quirks, cut): a 256 KiB mixed stream every frame of which the
    sieve's filter passes; the same with an unmasked and an RSV frame in its
    middle (between two data messages); the clean stream cut 3 bytes into its
    last header."""
    frames = conn_frames(4100 + seed, 5900, 300, bad=0.001, clean=True, p_close=0.0005)
    clean = H.build_frames_ref(frames)
    is_open, mid = False, None
    for i, (fl, _, _) in enumerate(frames):
        if i >= len(frames) // 2 and not is_open:
            mid = i
            break
        if fl & 0xF < 8:
            is_open = not fl & FIN
    rng = random.Random(7500 + seed)
    odd = H.build_frames_ref([(2 | FIN, rng.randbytes(300), None)]) + \
        streams.with_rsv(H.build_frames_ref([(1 | FIN | MASK, b"reserved bits", KEY)]))
    at = headers(clean)[mid][0]
    quirks = clean[:at] + odd + clean[at:]
    return clean, quirks, headers(clean)[-1][0] + 3


# ------------------------------------------------------ states and oracles

class State:
    """What one connection set carries from a batch into the next, of every
    kind: parser carries, the UTF-8 words, hvws_messages' states, the joined
    form's states and offsets, the RFC form's states, the closed flags, the
    connections whose rejected text message is still open (check 5), and the
    two previous outputs the joined and RFC forms' offsets point into."""

    def __init__(self, parser, u8, msg, join, join_off, rfc, closed, pending, join_out: bytes, rfc_out: bytes,
                 raw: Sequence[int] = (), null: bool = False):
        self.parser, self.u8, self.msg, self.join, self.join_off = parser, u8, msg, join, join_off
        self.rfc, self.closed, self.pending, self.join_out, self.rfc_out = rfc, closed, pending, join_out, rfc_out
        self.raw = tuple(raw)   # connections of illegal opcode sequences: no join of rec with bad[s] for them
        self.null = null        # fresh(): nothing is carried, the passes take NULL for their states

    def key(self):
        return (self.u8.tobytes(), self.msg.tobytes(), self.join.tobytes(), self.join_off.tobytes(), self.rfc.tobytes(),
                bytes(self.closed), tuple(self.pending), self.raw, hashlib.sha1(self.join_out).digest(),
                hashlib.sha1(self.rfc_out).digest())


def fresh(nseg: int, raw: Sequence[int] = ()) -> State:
    return State(None, np.zeros(nseg, np.uint32), M.states([M.FRESH] * nseg), M.states([M.FRESH] * nseg),
                 np.zeros(nseg, np.uint64), R.states([R.FRESH] * nseg), np.zeros(nseg, np.uint8), [False] * nseg, b"", b"", raw, True)


def join_check(table, bad, out: bytes, u8_in, pending_in, skip: Sequence[int] = ()) -> List[bool]:
    """The documented join of hvws_msg.rec with bad[s] over the RFC form's
    table: for a connection rejected in this batch, the data piece with the
    smallest rec >= bad[s] is a text message that wsutf8.is_utf8 rejects, once
    it is complete (-> still pending: the connections where it is not), and
    every text message completed before it is valid; no other connection has a
    completed invalid text message.  A connection that came in rejected got its
    verdict in an earlier batch: only a message still pending from then is
    looked at."""
    nseg = len(bad)
    by_seg = [[] for _ in range(nseg)]
    for p in table:
        if not int(p["info"]) & R.M_CTL:
            by_seg[int(p["seg"])].append(p)
    body = lambda p: out[int(p["off"]): int(p["off"]) + int(p["len"])]
    is_text = lambda p: int(p["info"]) & 0xF == 1
    done = lambda p: bool(int(p["info"]) & M.M_END)
    pending = [False] * nseg
    for s, pieces in enumerate(by_seg):
        if s in skip:   # illegal opcode sequences: hvws_utf8 and the message rule differ on what the text message is
            continue
        if int(u8_in[s]) & 15 > 7:
            if pending_in[s]:
                if not pieces:
                    pending[s] = True
                    continue
                p = pieces[0]
                assert int(p["info"]) & M.M_CONT and is_text(p), (s, "the rejected message does not continue")
                if done(p):
                    assert not U.is_utf8(body(p)), (s, "the rejected message is valid UTF-8")
                else:
                    pending[s] = True
            continue
        if int(bad[s]) == U.NONE:
            for p in pieces:
                assert not (done(p) and is_text(p)) or U.is_utf8(body(p)), (s, int(p["rec"]), "invalid text, bad == NONE")
            continue
        cand = [p for p in pieces if int(p["rec"]) != NOREC and int(p["rec"]) >= int(bad[s])]
        assert cand, (s, "no data piece at or behind bad[s]")
        hit = min(cand, key=lambda p: int(p["rec"]))
        assert is_text(hit), (s, int(hit["rec"]), "bad[s] joins a piece that is no text message")
        if done(hit):
            assert not U.is_utf8(body(hit)), (s, int(hit["rec"]), "bad[s] joins a valid text message")
        else:
            pending[s] = True
        for p in pieces:
            if int(p["rec"]) < int(hit["rec"]) and done(p) and is_text(p):
                assert U.is_utf8(body(p)), (s, int(p["rec"]), "invalid text ahead of bad[s]")
    return pending


class Expect:
    """The oracles' results for one batch from one State."""

    def __init__(self, data: bytes, segs, carries, st: State):
        nseg = len(segs)
        plain = bytearray(data)
        for s, (off, n) in enumerate(segs):
            plain[off:off + n] = H.scan_segment(data[off:off + n], carries[s] if carries is not None else None)[3]
        self.plain = np.frombuffer(bytes(plain), np.uint8)
        self.recs, self.words, self.u8, self.bad, self.firsts, self.carry = U.oracle_batch(data, segs, carries, st.u8)
        self.msg = M.oracle_batch(data, segs, carries, st.msg)
        self.join = J.joined_batch(data, segs, carries, st.join, st.join_out, st.join_off)
        self.rfc = R.rfc_batch(data, segs, carries, st.rfc, st.rfc_out)
        self.rep = R.replies_of(self.rfc[1], nseg, POLICY, st.closed)
        out = self.rfc[0]
        self.sent = S.expected([(fl, out[o:o + ln], 0) for o, ln, fl, _ in self.rep[0]], 0, False)
        self.pending = join_check(self.rfc[1], self.bad, out, st.u8, st.pending, st.raw)
        self.raw = st.raw
        self.closed = np.array([1 if f & S.RF_CLOSED else 0 for f in self.rep[3]], np.uint8)

    def next(self) -> State:
        return State(self.carry, self.u8, self.msg[3], self.join[3], self.join[4], self.rfc[3], self.closed,
                     self.pending, self.join[0], self.rfc[0], self.raw)


_MEMO = {}


def expect(data: bytes, segs, carries, st: State) -> Expect:
    """Expect(...), computed once per distinct input: every scan mode asks for the same few."""
    key = (hashlib.sha1(data).digest(), tuple(segs),
           None if carries is None else tuple(None if c is None else c.fields() for c in carries), st.key())
    if key not in _MEMO:
        _MEMO[key] = Expect(data, segs, carries, st)
    return _MEMO[key]


# -------------------------------------------------------------- the checker

def _same_table(got, want, what) -> None:
    assert len(got) == len(want), (what, "pieces", len(got), len(want))
    for f in want.dtype.names:
        if not np.array_equal(got[f], want[f]):
            k = int(np.flatnonzero(got[f] != want[f])[0])
            raise AssertionError(f"{what}: {f} of piece {k}: got {int(got[f][k]):#x}, expected {int(want[f][k]):#x}")


def _same_bytes(got: np.ndarray, want: bytes, what) -> None:
    """got: the output buffer with its slack; want: the bytes up to the total."""
    w = np.frombuffer(want, np.uint8)
    if not np.array_equal(got[:len(w)], w):
        k = int(np.flatnonzero(got[:len(w)] != w)[0])
        raise AssertionError(f"{what}: output byte {k} of {len(w)}: got {int(got[k]):#x}, expected {int(w[k]):#x}")
    assert np.all(got[len(w):] == SENTINEL), (what, "a byte at or beyond the total was written")


def _same_states(got, want, what) -> None:
    assert got.tobytes() == want.tobytes(), (what, got.tolist(), want.tolist())


class Prev:
    """The device buffers of the joined and the RFC form's previous outputs."""

    def __init__(self, d_join, join_len: int, d_rfc, rfc_len: int):
        self.d_join, self.join_len, self.d_rfc, self.rfc_len = d_join, join_len, d_rfc, rfc_len

    def free(self) -> None:
        for b in (self.d_join, self.d_rfc):
            if b is not None:
                b.free()
        self.d_join = self.d_rfc = None


class Run:
    """The passes over one scanned batch: q_* queues a pass, c_* compares what
    it left with the oracles (tables=False: its output bytes only -- the piece
    tables are the last form's).  check_passes runs each in turn; the pipelined
    tests queue all four, step on, and compare afterwards."""

    def __init__(self, eng, rx, data: bytes, segs, carries, how: str, st: Optional[State], prev: Optional[Prev]):
        import libhv_amd

        self.L = libhv_amd.lib()
        self.eng, self.rx, self.data, self.n, self.nseg = eng, rx, data, len(data), len(segs)
        self.masked = how == "scan"
        self.how = how
        # a fresh batch passes no state at all (NULL: all fresh), so no pass uploads one -- a second upload in a
        # row waits on the host for the first, which the pipelined tests must not do behind their stall
        self.st = st if st is not None else fresh(self.nseg)
        self.null = self.st.null
        self.prev = prev if prev is not None else Prev(None, 0, None, 0)
        self.e = expect(data, segs, carries, self.st)
        # out_cap = the batch and everything pending: no pass waits
        self.cap_m = self.n
        self.cap_j = self.n + int(self.st.join["pending"].sum())
        self.cap_r = self.n + int(self.st.rfc["data"]["pending"].sum()) + int(self.st.rfc["ctl"]["pending"].sum())
        self.out_m, self.out_j, self.out_r = (self._out(c) for c in (self.cap_m, self.cap_j, self.cap_r))
        self.got = {}

    def _out(self, cap: int):
        b = self.eng.alloc(cap + SLACK)
        assert self.L.hvws_memset(self.eng.ctx, b.ptr, SENTINEL, cap + SLACK) == 0
        return b

    def tag(self, what: str):
        return (what, self.how, "path", self.L.hvws_last_scan_path(self.eng.ctx))

    # 1. hvws_utf8
    def q_utf8(self) -> None:
        self.eng.utf8(self.rx, self.n, self.masked, None if self.null else self.st.u8)

    def c_utf8(self) -> None:
        e, tag = self.e, self.tag("hvws_utf8")
        assert self.L.hvws_utf8_count(self.eng.ctx) == len(e.words), tag
        words = self.eng.utf8_words()
        if not np.array_equal(words, e.words):
            k = int(np.flatnonzero(words != e.words)[0])
            raise AssertionError(f"{tag}: word of record {k}: got {int(words[k]):#x}, expected {int(e.words[k]):#x}")
        st, bad = self.eng.utf8_result(self.nseg)
        assert st.tolist() == e.u8.tolist(), tag
        assert bad.tolist() == e.bad.tolist(), tag
        self.got["u8"], self.got["bad"] = st.copy(), bad.copy()

    # 2. hvws_messages
    def q_messages(self) -> None:
        self.eng.messages(self.rx, self.n, self.masked, self.out_m, self.cap_m, None if self.null else self.st.msg)

    def _c_tables(self, want, tag) -> None:
        assert self.eng.msg_bytes() == len(want[0]), tag
        _same_table(self.eng.message_table(), want[1], tag)
        first, count = self.eng.segment_messages(self.nseg)
        assert first.tolist() == want[2][0].tolist() and count.tolist() == want[2][1].tolist(), tag

    def c_messages(self, tables: bool = True) -> None:
        tag = self.tag("hvws_messages")
        _same_bytes(self.out_m.download(self.cap_m + SLACK), self.e.msg[0], tag)
        if tables:
            self._c_tables(self.e.msg, tag)
            self.got["msg"] = self.eng.msg_state(self.nseg)
            _same_states(self.got["msg"], self.e.msg[3], tag)

    # 3. hvws_messages_joined
    def q_joined(self) -> None:
        self.eng.messages_joined(self.rx, self.n, self.masked, self.out_j, self.cap_j,
                                 None if self.null else self.st.join, self.prev.d_join, self.prev.join_len,
                                 None if self.null else self.st.join_off)

    def c_joined(self, tables: bool = True) -> None:
        tag = self.tag("hvws_messages_joined")
        _same_bytes(self.out_j.download(self.cap_j + SLACK), self.e.join[0], tag)
        if tables:
            self._c_tables(self.e.join, tag)
            self.got["join"] = self.eng.msg_state(self.nseg)
            _same_states(self.got["join"], self.e.join[3], tag)
            self.got["join_off"] = self.eng.msg_carry(self.nseg)
            assert self.got["join_off"].tolist() == self.e.join[4].tolist(), tag

    # 4. hvws_messages_rfc, then the server turn
    def q_rfc(self) -> None:
        self.eng.messages_rfc(self.rx, self.n, self.masked, self.out_r, self.cap_r, None if self.null else self.st.rfc,
                              self.prev.d_rfc, self.prev.rfc_len)

    def c_rfc(self) -> None:
        tag = self.tag("hvws_messages_rfc")
        _same_bytes(self.out_r.download(self.cap_r + SLACK), self.e.rfc[0], tag)
        self._c_tables(self.e.rfc, tag)
        self.got["rfc"] = self.eng.rfc_state(self.nseg)
        _same_states(self.got["rfc"], self.e.rfc[3], tag)

    def turn(self) -> None:
        """hvws_replies(SERVER | ECHO) and hvws_send_messages from the device table and count."""
        eng, e, tag = self.eng, self.e, self.tag("hvws_replies / hvws_send_messages")
        rep, answered, fc, flags = e.rep
        want, want_off, want_frames = e.sent
        eng.replies(POLICY, None if self.null else self.st.closed)
        table, d_n, cap = eng.replies_device()
        assert cap >= len(rep), tag
        tx = eng.alloc(len(want) + SLACK)
        moff = eng.alloc(8 * (cap + 1))
        try:
            assert self.L.hvws_memset(eng.ctx, tx.ptr, SENTINEL, len(want) + SLACK) == 0
            nbytes, nfr = eng.send_messages(tx, len(want), self.out_r, self.cap_r, table, cap, d_n, 0, False, moff)
            got_table, piece = eng.reply_table()
            assert [tuple(int(x) for x in r) for r in got_table.tolist()] == rep, tag
            assert piece.tolist() == answered, tag
            first, count = eng.segment_replies(self.nseg)
            assert (first.tolist(), count.tolist()) == (fc[0], fc[1]), tag
            got_flags = eng.reply_flags(self.nseg)
            assert got_flags.tolist() == flags, tag
            assert (nbytes, nfr) == (len(want), want_frames), tag
            assert moff.download(8 * (len(rep) + 1), np.uint64).tolist() == want_off, tag
            _same_bytes(tx.download(len(want) + SLACK), want, tag)
            self.got["closed"] = np.array([1 if f & S.RF_CLOSED else 0 for f in got_flags.tolist()], np.uint8)
        finally:
            eng.sync()
            tx.free()
            moff.free()

    # 5. hvws_msg.rec joined with bad[s], on what the device returned
    def join(self) -> None:
        self.got["pending"] = join_check(self.eng.message_table(), self.got["bad"], self.e.rfc[0], self.st.u8,
                                         self.st.pending, self.st.raw)
        assert self.got["pending"] == self.e.pending

    def c_buffer(self) -> None:
        """The batch as the scan (untouched) or the step (unmasked, gaps untouched) left it; the parser carries."""
        tag = self.tag("the batch")
        got = self.rx.download(self.n)
        want = np.frombuffer(self.data, np.uint8) if self.masked else self.e.plain
        assert np.array_equal(got, want), tag
        cout, _ = self.eng.carry(self.nseg)
        for s in range(self.nseg):
            assert cout[s].fields() == self.e.carry[s].fields(), (tag, s)
        self.got["parser"] = cout

    def finish(self):
        """-> (the engine's own carried state, its outputs as the next batch's prev); frees the rest."""
        g = self.got
        self.eng.sync()
        self.out_m.free()
        self.prev.free()
        st = State(g["parser"], g["u8"], g["msg"], g["join"], g["join_off"], g["rfc"], g["closed"], g["pending"],
                   self.e.join[0], self.e.rfc[0], self.st.raw)
        return st, Prev(self.out_j, len(self.e.join[0]), self.out_r, len(self.e.rfc[0]))

    def free(self) -> None:
        self.eng.sync()
        for b in (self.out_m, self.out_j, self.out_r):
            b.free()
        self.prev.free()


def check_passes(eng, rx, data: bytes, segs, carries, how: str, states: Optional[State] = None,
                 prev: Optional[Prev] = None):
    """After the caller's scan (how == "scan": payloads still masked, the buffer
    must come back unchanged) or step ("step": the buffer equals the oracle's
    unmasked bytes) of the batch `data` resident in rx: the four passes one
    after another behind that one scan, each compared exactly with its oracle;
    after hvws_messages_rfc the server turn; then the join of hvws_msg.rec with
    bad[s].  carries: the parser carries the scan was given; states, prev: what
    this function returned for the connections' previous batch (None, or
    fresh(nseg, raw) to name connections exempt from the join: fresh).
    Returns (states, prev) for the next batch: the engine's own carried state
    of every kind, and its output buffers (the caller frees the last prev)."""
    run = Run(eng, rx, data, segs, carries, how, states, prev)
    try:
        run.q_utf8()
        run.c_utf8()
        run.q_messages()
        run.c_messages()
        run.q_joined()
        run.c_joined()
        run.q_rfc()
        run.c_rfc()
        run.turn()
        run.join()
        run.c_buffer()
    except BaseException:
        run.free()
        raise
    return run.finish()
