"""CPU: tests/wssequence.py against itself -- the sequential numbering against
the closed form on random turns, the line and its parser, two turns chained."""
from __future__ import annotations

import random

import pytest

import wsenvelope as E
import wsroute as T
import wssequence as Q

M64 = (1 << 64) - 1
KINDS = (T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED)
SEEDS = (0, 9, 99, 10 ** 10 - 1, M64 - 1)


class Seeded(dict):
    """Counters of every topic without storing ntopics of them: topic t starts at seed(t)."""

    def __init__(self, seed):
        super().__init__()
        self.seed = seed

    def __missing__(self, t):
        return self.seed(t)


def random_turn(rng, n, ntopics, skew):
    hot = [rng.randrange(ntopics) for _ in range(3)]
    topics = [rng.choice(hot) if rng.random() < skew else rng.randrange(ntopics) for _ in range(n)]
    kinds = [T.RK_PUB if rng.random() < 0.6 else rng.choice(KINDS) for _ in range(n)]
    return topics, kinds


@pytest.mark.parametrize("ntopics", [1, 300, 70000])
@pytest.mark.parametrize("seed", SEEDS)
def test_sequential_against_the_closed_form(ntopics, seed):
    rng = random.Random(ntopics * 131 + seed % 1000)
    seen = set()
    for k in range(12):
        topics, kinds = random_turn(rng, rng.choice((0, 1, 7, 400, 3000)), ntopics, (0.0, 0.5, 0.95)[k % 3])
        ctr = Seeded(lambda t: (seed + t) & M64 if k % 2 else seed)
        a, b = Q.sequential(ctr, topics, kinds), Q.closed_form(ctr, topics, kinds)
        assert a == b
        seq, after, (pubs, distinct) = a
        seen |= set(kinds)
        assert pubs == sum(kd == T.RK_PUB for kd in kinds) and distinct == len(after)
        assert all(q == 0 for q, kd in zip(seq, kinds) if kd != T.RK_PUB)
        for t, v in after.items():
            mine = [q for q, tt, kd in zip(seq, topics, kinds) if kd == T.RK_PUB and tt == t]
            assert mine == [(ctr[t] + 1 + r) & M64 for r in range(len(mine))] and v == mine[-1]
    assert seen == set(KINDS)


def test_the_wrap_goes_through_the_last_number_to_zero():
    topics, kinds = [0, 0, 1, 0], [T.RK_PUB, T.RK_PUB, T.RK_SUB, T.RK_PUB]
    seq, after, totals = Q.sequential([M64 - 1, 5], topics, kinds)
    assert seq == [M64, 0, 0, 1] and after == {0: 1} and totals == (3, 1)
    assert Q.closed_form([M64 - 1, 5], topics, kinds) == (seq, after, totals)


def test_two_turns_chained_give_consecutive_numbers_and_quiet_topics_keep_their_seed():
    rng = random.Random(5)
    ctr = [9, 99, 10 ** 10 - 1, M64 - 2, 1234]
    seen = {t: [] for t in range(4)}
    for _ in range(2):
        topics, kinds = random_turn(rng, 200, 4, 0.3)         # topic 4 is never published to
        seq, after, _ = Q.sequential(ctr, topics, kinds)
        assert Q.closed_form(ctr, topics, kinds)[:2] == (seq, after)
        for q, t, kd in zip(seq, topics, kinds):
            if kd == T.RK_PUB:
                seen[t].append(q)
        for t, v in after.items():
            ctr[t] = v
    for t, first in zip(range(4), (9, 99, 10 ** 10 - 1, M64 - 2)):
        assert len(seen[t]) > 10 and seen[t] == [(first + 1 + r) & M64 for r in range(len(seen[t]))]
        assert ctr[t] == seen[t][-1]
    assert ctr[4] == 1234 and 0 in seen[3]


@pytest.mark.parametrize("flags", [0, E.ENV_SENDER])
def test_the_line_round_trips_through_the_parser(flags):
    ids = (0, 7, 42, 4294967295)
    seqs = (0, 1, 9, 10, 99, 10 ** 10 - 1, 10 ** 10, 10 ** 19 - 1, 10 ** 19, M64)
    longest = 0
    for t in ids:
        for s in ids:
            for q in seqs:
                ln = Q.line(t, s, q, flags)
                longest = max(longest, len(ln))
                for body in (b"", b"x", b"M1 #2\nnested", b"\n"):
                    assert Q.parse(ln + body) == (t, s if flags else None, q, body)
                    assert Q.parse_any(ln + body) == (t, s if flags else None, q, body)
                assert E.parse(ln) is None                     # hvws_envelope's parser refuses the sequenced line
                plain = E.line(t, s, flags)
                assert Q.parse(plain + b"body") is None        # ... and the sequenced parser the plain one
                assert Q.parse_any(plain + b"body") == (t, s if flags else None, None, b"body")
    assert longest == (Q.HDR_MAX if flags else Q.HDR_MAX - 11)
    assert Q.HDR_MAX == len(b"M4294967295 4294967295 #18446744073709551615\n")


def test_the_parser_refuses_what_is_no_line():
    for bad in (b"", b"M", b"M7", b"M7 #\n", b"M7 #01\n", b"M07 #1\n", b"M7  #1\n", b"M7 #1", b"M7 1 2 #3\n", b"m7 #1\n",
                b"M7 #123456789012345678901\n", b"M7#1\n", b"M7 # 1\n", b"P7\n"):
        assert Q.parse(bad) is None, bad


def test_the_enveloped_bytes_are_the_plain_ones_with_the_number_on_the_line():
    out = bytes(range(256)) * 2
    rows = [(0, 10, 0x81, 0), (16, 0, 0x81, 0), (20, 300, 0x82, 0), (330, 5, 0x8A, 7), (0, 0, 0x81, 0), (340, 33, 0x81, 0)]
    topics = [3, 3, 12345, 0, 9, 3]
    kinds = [T.RK_PUB, T.RK_PUB, T.RK_PUB, T.RK_OTHER, T.RK_SUB, T.RK_PUB]
    sender, dest_of = [0, 0, 1, 1, 1, 0], [2147483646, 5]
    seq, _, _ = Q.sequential({3: 98, 12345: M64}, topics, kinds)
    assert seq == [99, 100, 0, 0, 0, 101]
    for flags in (0, E.ENV_SENDER):
        rows2, env, placed, totals = Q.envelope_sequential(rows, topics, kinds, sender, dest_of, out, seq, flags)
        assert (rows2, totals) == Q.envelope_closed_form(rows, topics, kinds, sender, dest_of, out, seq, flags)
        plain = E.sequential(rows, topics, kinds, sender, dest_of, out, flags)
        assert totals[:2] == plain[3][:2] == (4, 1) and len(placed) == len(plain[2])
        for (a, b), (_, pb), k in zip(placed, plain[2], [kd for kd in kinds if kd in (T.RK_PUB, T.RK_OTHER)]):
            assert a % 16 == 0 and bytes(env[a:a + len(b)]) == b
            if k == T.RK_PUB:
                t, s, q, body = Q.parse(b)
                assert E.parse(pb) == (t, s, body) and q in (99, 100, 0, 101)
            else:
                assert b == pb
        assert totals[3] <= Q.bound(len(out), len(rows))
