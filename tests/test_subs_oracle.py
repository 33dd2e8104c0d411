"""CPU: the model of hvws_subs_update (tests/wssubs.py) -- the sequential rule
of include/hvws.h against the closed form over stamps that the device computes,
on random and on hand-written cases, and what the updated table means for
hvws_fanout's model (tests/wsfan.py): a dropped destination receives nothing."""
from __future__ import annotations

import random

import pytest

import wsfan as W
import wssubs as U

JOIN, LEAVE, DROP = U.JOIN, U.LEAVE, U.DROP


def small_case(rng):
    nt, nd = rng.randint(1, 4), rng.randint(1, 6)
    topics = [[rng.randrange(nd) for _ in range(rng.choice((0, 1, 3, 6)))] for _ in range(nt)]
    closed = rng.sample(range(nd), rng.randint(0, min(2, nd)))
    events = [(rng.choice((JOIN, JOIN, LEAVE, DROP)), rng.randrange(nt), rng.randrange(nd))
              for _ in range(rng.randint(0, 10))]
    return topics, closed, events


def test_sequential_equals_closed_form_on_4000_random_cases():
    rng = random.Random(1)
    for _ in range(4000):
        topics, closed, events = small_case(rng)
        for flags in (0, U.UNIQUE):
            a, b = U.sequential(topics, closed, events, flags), U.closed_form(topics, closed, events, flags)
            assert a == b, (topics, closed, events, flags, a, b)


def test_sequential_equals_closed_form_on_turn_sized_cases():
    rng = random.Random(2)
    for _ in range(300):
        _, topics, ndest, _, dest_of, _, events, flags = U.random_case(rng)
        closed = rng.sample(dest_of, rng.randint(0, len(dest_of)))
        assert U.sequential(topics, closed, events, flags) == U.closed_form(topics, closed, events, flags)


@pytest.mark.parametrize("case", U.HAND_CASES, ids=[c[0] for c in U.HAND_CASES])
def test_hand_cases(case):
    _, topics, closed, events, flags, want = case
    assert U.sequential(topics, closed, events, flags) == want
    assert U.closed_form(topics, closed, events, flags) == want
    first, member, cnt, rows = U.update(topics, closed, events, flags)
    assert rows == want and first[0] == 0 and first[-1] == len(member) == cnt[0] + cnt[1]
    assert cnt[0] + cnt[2] == sum(len(m) for m in topics) and cnt[3] == len(set(closed))


def test_counts_on_a_known_case():
    topics = [[1, 2, 2], [3], []]
    rows = U.sequential(topics, [3, 3], [(JOIN, 2, 1), (LEAVE, 0, 2), (JOIN, 0, 2), (DROP, 0, 7)])
    assert rows == [[1, 2], [], [1]]
    assert U.counts(topics, rows, [3, 3], [(JOIN, 2, 1), (LEAVE, 0, 2), (JOIN, 0, 2), (DROP, 0, 7)]) == (1, 2, 3, 1)


def test_unique_leaves_old_duplicates_and_adds_none():
    rng = random.Random(3)
    for _ in range(500):
        topics, closed, events = small_case(rng)
        rows = U.sequential(topics, closed, events, U.UNIQUE)
        for t, m in enumerate(rows):
            for d in set(m):
                assert m.count(d) <= max(1, topics[t].count(d)), (topics, closed, events, rows)


def test_fanout_over_the_updated_lists_reaches_no_dropped_destination():
    """A publication to every topic, through the lists after the update: nothing
    for a closed connection or a DROPped id unless a later JOIN listed it again."""
    rng = random.Random(4)
    for _ in range(300):
        topics, closed, events = small_case(rng)
        nd = 7
        rows = U.sequential(topics, closed, events, rng.choice((0, U.UNIQUE)))
        replies = [(0, 1, 0x11, 0)] * len(topics)          # one TEXT reply per sender, sender s publishes to topic s
        sender = list(range(len(topics)))
        dest_of = [nd + s for s in sender]                  # no sender is a subscriber
        _, _, _, count = W.fanout(replies, sender, rows, nd + len(topics), sender, dest_of)
        gone = set(closed) | {d for op, _, d in events if op == DROP}
        for d in gone:
            last = max([-1] + [e for e, (op, _, x) in enumerate(events) if op == DROP and x == d])
            if not any(op == JOIN and x == d and e > last for e, (op, _, x) in enumerate(events)):
                assert count[d] == 0, (topics, closed, events, rows)
        assert sum(count) == sum(len(m) for m in rows)
