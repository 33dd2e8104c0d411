"""CPU: the UTF-8 oracle of tests/wsutf8.py against Python's strict decoder,
transition-word composition, the fold rules on hand-written streams, and the
Python restatement of the device kernels' decomposition (head / interior
predicate / tail, libhv_amd/csrc/hvws_utf8.hip) against the plain machine."""
from __future__ import annotations

import itertools
import random

import wsutf8 as U

I_HDR, I_BODY, I_END = U.I_HDR, U.I_BODY, U.I_END
FIN = U.FIN


def test_known_answers():
    assert U.word(b"") == U.IDENTITY == 0x76543210
    assert U.word(b"abc") == 0xFFFFFFF0
    assert U.word(bytes([0x82, 0xAC])) == 0x11F0F0FF
    assert U.compose(U.word(bytes([0xE2])), U.word(bytes([0x82, 0xAC]))) == U.word("\u20ac".encode())


def test_machine_matches_strict_decoder_exhaustively():
    """run(0, d) == 0 iff d.decode('utf-8') succeeds, over the 25-byte boundary
    alphabet at lengths 0-4 (406,901 strings)."""
    n = 0
    for length in range(5):
        for t in itertools.product(U.ALPHA, repeat=length):
            d = bytes(t)
            assert (U.run(0, d) == 0) == U.is_utf8(d), d.hex()
            n += 1
    assert n == 406901


def _mutated(r: random.Random) -> bytes:
    d = "".join(r.choice(U.POOL) for _ in range(r.randint(0, 8))).encode()
    if d and r.random() < 0.6:
        i = r.randrange(len(d))
        d = d[:i] + bytes([r.choice(U.MUTATIONS + list(U.ALPHA))]) + d[i + 1:]
    if d and r.random() < 0.3:
        d = d[r.randint(0, 2): len(d) - r.randint(0, 2)]
    return d


def test_machine_matches_strict_decoder_on_mutated_text():
    r = random.Random(11)
    seen = [0, 0]
    for _ in range(20000):
        d = _mutated(r)
        ok = U.is_utf8(d)
        seen[ok] += 1
        assert (U.run(0, d) == 0) == ok, d.hex()
    assert min(seen) > 2000


def test_composition_at_random_cuts():
    r = random.Random(5)
    for _ in range(4000):
        d = _mutated(r) if r.random() < 0.7 else bytes(r.choice(U.ALPHA) for _ in range(r.randint(0, 9)))
        cuts = sorted(r.randint(0, len(d)) for _ in range(r.randint(1, 3)))
        w = U.IDENTITY
        for a, b in zip([0] + cuts, cuts + [len(d)]):
            w = U.compose(w, U.word(d[a:b]))
        assert w == U.word(d), (d.hex(), cuts)
    # associativity on words themselves
    ws = [U.word(bytes(r.choice(U.ALPHA) for _ in range(r.randint(0, 3)))) for _ in range(300)]
    for _ in range(2000):
        a, b, c = r.choice(ws), r.choice(ws), r.choice(ws)
        assert U.compose(U.compose(a, b), c) == U.compose(a, U.compose(b, c))


def _rec(op, payload: bytes, fin=True, hdr=True, end=True):
    info = op | (FIN if fin else 0) | (I_HDR if hdr else 0) | (I_BODY if payload else 0) | (I_END if end else 0)
    return info, U.word(payload)


def _fold(recs, state_in=0, first=0):
    return U.fold([r[0] for r in recs], [r[1] for r in recs], state_in, first)


def test_fold_character_over_three_fragments_with_ping():
    e = "\u20ac".encode()   # E2 82 AC
    recs = [_rec(1, e[:1], fin=False), _rec(9, b"\xff\xfe"), _rec(0, e[1:2], fin=False), _rec(0, e[2:])]
    assert _fold(recs) == (0, U.NONE)
    # the same with the last byte wrong: the third fragment rejects
    recs[3] = _rec(0, b"\x41")
    assert _fold(recs, first=7) == (U.REJ, 10)
    # state after the first fragment only: text open, two continuations due
    assert _fold(recs[:1]) == (U.TEXT_OPEN | 2, U.NONE)


def test_fold_lone_continuation_and_binary_are_ignored():
    assert _fold([_rec(0, b"\xff\xff")]) == (0, U.NONE)
    assert _fold([_rec(2, b"\xc0\xff", fin=False), _rec(0, b"\x80")]) == (0, U.NONE)
    # a binary message after an unfinished text message closes it unchecked
    assert _fold([_rec(1, b"\xe2", fin=False), _rec(2, b"\xff")]) == (0, U.NONE)


def test_fold_truncation_at_fin():
    assert _fold([_rec(1, b"ab\xe2\x82")]) == (U.REJ, 0)
    assert _fold([_rec(1, b"ab\xe2\x82", fin=False)]) == (U.TEXT_OPEN | 1, U.NONE)
    assert _fold([_rec(1, b"ab", fin=False), _rec(0, b"", fin=True)]) == (0, U.NONE)
    assert _fold([_rec(1, b"\xf0\x90", fin=False), _rec(0, b"", fin=True)], first=3) == (U.REJ, 4)


def test_fold_payload_pieces_across_batches():
    """A frame whose payload continues in the next batch: records without
    HVWS_I_HDR keep what is open, and END comes with the last piece."""
    a = _rec(1, b"x\xf0\x9f", fin=True, end=False)
    b = _rec(1, b"\x98", fin=True, hdr=False, end=False)
    c = _rec(1, b"\x80", fin=True, hdr=False, end=True)
    s1, bad = _fold([a])
    assert (s1, bad) == (U.TEXT_OPEN | 2, U.NONE)   # F0 9F: two more due
    s2, bad = _fold([b], s1)
    assert (s2, bad) == (U.TEXT_OPEN | 1, U.NONE)   # F0 9F 98: one more due
    assert _fold([c], s2) == (0, U.NONE)
    assert _fold([a, b, c]) == (0, U.NONE)


def test_fold_carried_in_reject_is_sticky():
    assert _fold([], U.REJ, first=42) == (U.REJ, 42)
    assert _fold([_rec(1, b"ok")], U.REJ | U.TEXT_OPEN, first=3) == (U.REJ, 3)
    # after a rejection later records change nothing
    recs = [_rec(1, b"\xff"), _rec(1, b"fine")]
    assert _fold(recs) == (U.REJ, 0)


def test_kernel_decomposition_equals_plain_machine():
    """word_fast (head over 3 bytes, a 4-byte-window predicate from byte 3 on,
    tail from the last 3 bytes) == word on strings of 7-8 bytes over the
    boundary alphabet, and on mutated multi-byte text of every length."""
    r = random.Random(2024)
    seen = set()
    for _ in range(120000):
        d = bytes(r.choice(U.ALPHA) for _ in range(r.randint(7, 8)))
        assert U.word_fast(d) == U.word(d), d.hex()
        seen.add(U.word(d))
    assert len(seen) > 20   # not all REJECT
    for _ in range(40000):
        d = _mutated(r) + _mutated(r)
        assert U.word_fast(d) == U.word(d), d.hex()


def test_generator_is_balanced_and_uses_the_boundary_characters():
    frames, valid = U.gen_frames(3, 200)
    assert U.balanced(valid)
    text = b"".join(p for _, p, _ in frames)
    for ch in ("\u07ff", "\u0800", "\ud7ff", "\ue000", "\uffff", "\U00010000", "\U0010ffff"):
        assert ch.encode() in text
    assert any(len(p) == 0 and (fl & 0xF) == 0 for fl, p, _ in frames)       # empty fragments
    assert any((fl & 0xF) in (9, 10) for fl, _, _ in frames)                 # control frames between fragments
    assert any((fl & 0xF) == 2 for fl, _, _ in frames)
