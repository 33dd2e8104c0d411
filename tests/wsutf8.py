"""UTF-8 validation oracle for hvws_utf8 (include/hvws.h): the state machine
of RFC 3629 as the header numbers it, transition words and their composition,
the per-segment fold, a Python restatement of the decomposition the device
kernels use (libhv_amd/csrc/hvws_utf8.hip), and a seeded stream generator.

A helper, not a test module."""
from __future__ import annotations

import random
from typing import List, Optional, Sequence, Tuple

import numpy as np

ACCEPT, REJ = 0, 15
TEXT_OPEN = 1 << 4
IDENTITY = 0x76543210
NONE = (1 << 64) - 1
I_HDR, I_BODY, I_END = 1 << 10, 1 << 11, 1 << 12
FIN, MASK = 0x10, 0x20

# the bytes at which the machine's behaviour changes
ALPHA = bytes.fromhex("00417F808F909FA0BFC0C1C2DFE0E1ECEDEEEFF0F1F3F4F5FF")
assert len(ALPHA) == 25


def step(s: int, b: int) -> int:
    if s == 0:
        if b <= 0x7F:
            return 0
        if 0xC2 <= b <= 0xDF:
            return 1
        if b == 0xE0:
            return 3
        if b == 0xED:
            return 4
        if 0xE1 <= b <= 0xEF:
            return 2
        if b == 0xF0:
            return 5
        if 0xF1 <= b <= 0xF3:
            return 6
        if b == 0xF4:
            return 7
        return REJ
    if s > 7:
        return REJ
    lo = {3: 0xA0, 5: 0x90}.get(s, 0x80)
    hi = {4: 0x9F, 7: 0x8F}.get(s, 0xBF)
    if not lo <= b <= hi:
        return REJ
    return 0 if s == 1 else (1 if s <= 4 else 2)


_STEP = [[step(s, b) for b in range(256)] for s in range(16)]


def run(s: int, d: bytes) -> int:
    for b in d:
        s = _STEP[s][b]
    return s


def pack(states: Sequence[int]) -> int:
    return sum(int(s) << (4 * k) for k, s in enumerate(states))


def word(d: bytes) -> int:
    """Nibble k = exit state for entry state k, k = 0..7."""
    return pack(run(k, d) for k in range(8))


def nib(w: int, s: int) -> int:
    return REJ if s > 7 else (w >> (4 * s)) & 15


def compose(a: int, b: int) -> int:
    """The word of x + y from a = word(x), b = word(y)."""
    return pack(nib(b, nib(a, k)) for k in range(8))


def fold(infos: Sequence[int], words: Sequence[int], state_in: int = 0, first: int = 0) -> Tuple[int, int]:
    """One segment's records in order -> (state word out, index of the first
    rejecting record or NONE); `first` is the index of the segment's first record."""
    st, text = state_in & 15, (state_in >> 4) & 1
    if st > 7:
        return REJ, first
    for i, (info, w) in enumerate(zip(infos, words)):
        op, fin = info & 0xF, info & FIN
        if op >= 3:
            continue
        if op == 1 and info & I_HDR:
            text, st = 1, ACCEPT
        elif op == 2 and info & I_HDR:
            text, st = 0, ACCEPT
        if text and info & I_BODY:
            st = nib(w, st)
        if info & I_END and fin and text:
            if st != ACCEPT:
                st = REJ
            text = 0
        if st == REJ:
            return REJ, first + i
    return st | (text << 4), NONE


# ---- the decomposition k_u8_tiles / k_u8_words use ---------------------------

def blen(b: int) -> int:
    """0 continuation, 1 ASCII, 2 / 3 / 4 lead of that many bytes, 9 never legal."""
    if b < 0x80:
        return 1
    if b < 0xC0:
        return 0
    if b < 0xC2:
        return 9
    if b < 0xE0:
        return 2
    if b < 0xF0:
        return 3
    if b < 0xF5:
        return 4
    return 9


def ok2(p: int, q: int) -> bool:
    lo = 0xA0 if p == 0xE0 else 0x90 if p == 0xF0 else 0x80
    hi = 0x9F if p == 0xED else 0x8F if p == 0xF4 else 0xBF
    return lo <= q <= hi


def local(d: bytes, i: int) -> bool:
    """The predicate at byte i >= 3; reads d[i - 3 .. i] only."""
    b, p1, p2, p3 = d[i], d[i - 1], d[i - 2], d[i - 3]
    l0, l1, l2, l3 = blen(b), blen(p1), blen(p2), blen(p3)
    if l0 == 0:
        if l1:
            return 2 <= l1 <= 4 and ok2(p1, b)
        if l2:
            return 3 <= l2 <= 4 and ok2(p2, p1)
        if l3:
            return l3 == 4 and ok2(p3, p2)
        return False
    if l0 == 9:
        return False
    if l1:
        return l1 == 1
    if l2:
        return l2 == 2
    if l3:
        return l3 == 3 and ok2(p3, p2)
    return True


def word_fast(d: bytes) -> int:
    n = len(d)
    if n <= 6:   # short payloads: the plain machine in one lane
        return word(d)
    interior = all(local(d, i) for i in range(3, n))
    t0, t1, t2 = d[n - 3], d[n - 2], d[n - 1]
    if blen(t2):
        tail = step(0, t2)
    elif blen(t1):
        tail = run(0, bytes([t1, t2]))
    elif blen(t0):
        tail = run(0, bytes([t0, t1, t2]))
    else:
        tail = 0
    out = []
    for k in range(8):
        s = run(k, d[:3])
        out.append(REJ if s == REJ or not interior else tail)
    return pack(out)


# ---- seeded streams ----------------------------------------------------------

POOL = ["a", "Z", "0", " ", "~", "\x00", "\x7f", "\u0080", "\u00e9", "\u07ff", "\u0800", "\u20ac", "\ud7ff",
        "\ue000", "\uffff", "\U00010000", "\U0001f600", "\U0010ffff"]
MUTATIONS = [0x80, 0xBF, 0xC0, 0xC1, 0xE0, 0xED, 0xF0, 0xF4, 0xF5, 0xFF, 0x41]


def is_utf8(d: bytes) -> bool:
    try:
        d.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def gen_frames(seed: int, nmsg: int, max_bytes: int = 40, masked: bool = True, bad: float = 0.45):
    """-> (frames [(flags, payload, key or None)], text message validity [bool]).
    Text messages from POOL, some with one byte replaced from MUTATIONS or cut
    short, fragmented at random positions (0 and the end included, so empty
    fragments occur) with ping / pong frames between fragments; binary messages
    of random bytes mixed in."""
    r = random.Random(seed)
    frames: List[Tuple[int, bytes, Optional[bytes]]] = []
    valid: List[bool] = []
    m = MASK if masked else 0

    def key():
        return bytes(r.randrange(256) for _ in range(4)) if masked else None

    for _ in range(nmsg):
        if r.random() < 0.2:
            op, data = 2, bytes(r.randrange(256) for _ in range(r.randint(0, max_bytes)))
        else:
            op, data = 1, b""
            for _ in range(r.randint(0, 14)):
                ch = r.choice(POOL).encode("utf-8")
                if len(data) + len(ch) > max_bytes:
                    break
                data += ch
            u = r.random()
            if data and u < bad * 0.75:
                i = r.randrange(len(data))
                data = data[:i] + bytes([r.choice(MUTATIONS)]) + data[i + 1:]
            elif len(data) > 1 and u < bad:
                data = data[: r.randint(1, len(data) - 1)]
            valid.append(is_utf8(data))
        nfrag = r.choice([1, 1, 1, 2, 3, 4])
        cuts = sorted(r.randint(0, len(data)) for _ in range(nfrag - 1))
        parts = [data[a:b] for a, b in zip([0] + cuts, cuts + [len(data)])]
        for i, part in enumerate(parts):
            fl = (op if i == 0 else 0) | (FIN if i == len(parts) - 1 else 0) | m
            frames.append((fl, part, key()))
            if i < len(parts) - 1 and r.random() < 0.5:
                ctl = r.choice([9, 10])
                frames.append((ctl | FIN | m, bytes(r.randrange(256) for _ in range(r.randint(0, 10))), key()))
    return frames, valid


def balanced(valid: Sequence[bool]) -> bool:
    """At least a quarter of the text messages valid and a quarter invalid."""
    n = len(valid)
    good = sum(valid)
    return n >= 4 and 4 * good >= n and 4 * (n - good) >= n


def gen_stream(seed: int, nmsg: int, max_bytes: int = 40, masked: bool = True):
    """-> (wire bytes built by the reference's websocket_build_frame, validity)."""
    import wsharness as H

    frames, valid = gen_frames(seed, nmsg, max_bytes, masked)
    return H.build_frames_ref(frames), valid


def oracle_batch(data: bytes, segs, carry=None, state_in=None):
    """The oracle's view of one batch: per record (absolute offsets) the
    transition word of its plaintext, per segment the fold.  -> (records,
    words, state_out, bad, first, carry_out)."""
    import wsharness as H

    recs_all, words, state_out, bad, firsts, carry_out = [], [], [], [], [], []
    for s, (off, n) in enumerate(segs):
        recs, st, _, plain = H.scan_segment(data[off:off + n], carry[s] if carry is not None else None)
        w = [word(plain[int(r["pay_off"]): int(r["pay_off"]) + int(r["pay_len"])]) for r in recs]
        first = len(words)
        so, b = fold([int(r["info"]) for r in recs], w, int(state_in[s]) if state_in is not None else 0, first)
        recs = recs.copy()
        recs["pay_off"] += np.uint64(off)
        recs_all.append(recs)
        words += w
        state_out.append(so)
        bad.append(b)
        firsts.append(first)
        carry_out.append(st)
    recs_cat = np.concatenate(recs_all) if recs_all else np.zeros(0)
    return (recs_cat, np.array(words, dtype=np.uint32), np.array(state_out, dtype=np.uint32),
            np.array(bad, dtype=np.uint64), firsts, carry_out)
