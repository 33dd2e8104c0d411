"""Oracle for hvws_subs_update (include/hvws.h): the contract in plain Python,
twice -- the sequential rule as the header states it (`sequential`), and the
closed form over stamps that the device computes (`closed_form`: old listings
stamp 0, the drops of closed connections stamp 1, event e stamp e + 2; a listing
survives iff no LEAVE of its pair and no DROP of its destination has a stamp at
or above its own).  tests/test_subs_oracle.py holds the two against each other.

topics: [[destination ids] per topic]; closed: the destination ids of the
connections the reply call closed (any iterable, repeats allowed); events:
[(op, topic, dest)].

A helper, not a test module."""
from __future__ import annotations

from typing import Iterable, List, Sequence, Tuple

import wsfan as W

JOIN, LEAVE, DROP = 1, 2, 3
UNIQUE = 1
RF_CLOSED = 1


def sequential(topics, closed: Iterable[int], events, flags: int = 0) -> List[List[int]]:
    """The rule of the header, step by step."""
    gone = set(closed)
    rows = [[(d, None) for d in m if d not in gone] for m in topics]      # (id, joining event or None)
    for e, (op, t, d) in enumerate(events):
        if op == JOIN:
            if not flags & UNIQUE or all(x != d for x, _ in rows[t]):
                rows[t].append((d, e))
        elif op == LEAVE:
            rows[t] = [(x, s) for x, s in rows[t] if x != d]
        elif op == DROP:
            rows = [[(x, s) for x, s in m if x != d] for m in rows]
        else:
            raise ValueError(op)
    out = []
    for m in rows:
        old = [x for x, s in m if s is None]
        new = sorted((x, s) for x, s in m if s is not None)
        out.append(old + [x for x, _ in new])
    return out


def closed_form(topics, closed: Iterable[int], events, flags: int = 0) -> List[List[int]]:
    """The same table from stamps alone: no state is walked through the events."""
    drop = {}
    for d in closed:
        drop[d] = max(drop.get(d, 0), 1)
    groups = {}
    for e, (op, t, d) in enumerate(events):
        if op == DROP:
            drop[d] = max(drop.get(d, 0), e + 2)
        else:
            groups.setdefault((t, d), []).append((e, op))
    out = []
    for t, m in enumerate(topics):
        def kill(d):
            return max([drop.get(d, 0)] + [e + 2 for e, op in groups.get((t, d), []) if op == LEAVE])

        row = [d for d in m if kill(d) == 0]
        for (tt, d), g in sorted(groups.items()):
            if tt != t:
                continue
            k = kill(d)
            eff = [e for e, op in g if op == JOIN and e + 2 > k]
            if flags & UNIQUE:
                eff = [] if k == 0 and d in m else eff[:1]
            row += [d] * len(eff)
        out.append(row)
    return out


def counts(topics, new_topics, closed: Iterable[int], events, flags: int = 0) -> Tuple[int, int, int, int]:
    """(old listings kept, listings added, old listings removed, distinct
    destinations dropped as closed) -- hvws_get_subs_counts."""
    gone = set(closed)
    for op, t, d in events:
        if op == DROP:
            gone.add(d)
    left = {(t, d) for op, t, d in events if op == LEAVE}
    kept = sum(1 for t, m in enumerate(topics) for d in m if d not in gone and (t, d) not in left)
    old = sum(len(m) for m in topics)
    new = sum(len(m) for m in new_topics)
    return kept, new - kept, old - kept, len(set(closed))


def update(topics, closed: Iterable[int], events, flags: int = 0):
    """-> (topic_first, member, (kept, added, removed, dropped), rows) of the new table."""
    closed = list(closed)
    rows = sequential(topics, closed, events, flags)
    first, member = W.flatten(rows)
    return first, member, counts(topics, rows, closed, events, flags), rows


def closed_dests(flags: Sequence[int], dest_of: Sequence[int]) -> List[int]:
    """dest_of[s] of every segment whose reply flags hold RF_CLOSED."""
    return [int(dest_of[s]) for s, f in enumerate(flags) if f & RF_CLOSED]


def random_events(rng, ntopics: int, ndest: int, pool: Sequence[int], n: int):
    ev = []
    for _ in range(n):
        op = rng.choice((JOIN, JOIN, JOIN, LEAVE, LEAVE, DROP)) if ntopics else DROP
        d = rng.choice(pool) if pool and rng.random() < 0.7 else rng.randrange(ndest)
        ev.append((op, rng.randrange(ntopics) if ntopics else 0, d))
    return ev


def random_case(rng, **kw):
    """wsfan.random_case's turn with events for hvws_subs_update: (reads,
    topics, ndest, pub, dest_of, fanout flags, events, update flags).  The events
    favour the ids the topics list and the connections of the turn, so that
    kills, re-joins and duplicates all occur."""
    reads, topics, ndest, pub, dest_of, fflags = W.random_case(rng, **kw)
    pool = sorted({d for m in topics for d in m} | set(dest_of))
    events = random_events(rng, len(topics), ndest, pool, rng.choice((0, 1, 3, 8, 20)))
    return reads, topics, ndest, pub, dest_of, fflags, events, rng.choice((0, UNIQUE))


# (name, topics, closed, events, flags, the new rows) -- one per pair history
HAND_CASES = [
    ("kill then join", [[4, 5], [5]], [], [(LEAVE, 0, 5), (JOIN, 0, 5)], 0, [[4, 5], [5]]),
    ("join then kill", [[4], []], [], [(JOIN, 0, 5), (JOIN, 1, 5), (LEAVE, 0, 5)], 0, [[4], [5]]),
    ("join then drop", [[4], []], [], [(JOIN, 0, 5), (DROP, 9, 5), (JOIN, 1, 4)], 0, [[4], [4]]),
    ("join join", [[4]], [], [(JOIN, 0, 5), (JOIN, 0, 5)], 0, [[4, 5, 5]]),
    ("join join, unique, not listed", [[4]], [], [(JOIN, 0, 5), (JOIN, 0, 5)], UNIQUE, [[4, 5]]),
    ("join join, unique, listed", [[5, 4]], [], [(JOIN, 0, 5), (JOIN, 0, 5)], UNIQUE, [[5, 4]]),
    ("unique, listed, leave between", [[5, 4]], [], [(JOIN, 0, 5), (LEAVE, 0, 5), (JOIN, 0, 5), (JOIN, 0, 5)], UNIQUE,
     [[4, 5]]),
    ("unique, a join before the drop and two after", [[4]], [], [(JOIN, 0, 5), (DROP, 0, 5), (JOIN, 0, 5), (JOIN, 0, 5)],
     UNIQUE, [[4, 5]]),
    ("old duplicates and a leave", [[5, 4, 5, 5], [5, 5]], [], [(LEAVE, 0, 5)], 0, [[4], [5, 5]]),
    ("old duplicates stay under unique", [[5, 4, 5]], [], [(JOIN, 0, 4), (JOIN, 0, 6)], UNIQUE, [[5, 4, 5, 6]]),
    ("a drop across many rows", [[1, 2], [], [2], [3, 2, 2], [1]], [], [(DROP, 0, 2)], 0, [[1], [], [], [3], [1]]),
    ("a closed id joined again", [[1, 2], [2, 3]], [2], [(JOIN, 1, 2)], 0, [[1], [3, 2]]),
    ("a closed id joined again, unique", [[1, 2], [2, 3]], [2, 2], [(JOIN, 1, 2), (JOIN, 1, 2)], UNIQUE, [[1], [3, 2]]),
    ("joins ordered by destination, then event", [[9]], [], [(JOIN, 0, 7), (JOIN, 0, 3), (JOIN, 0, 7), (JOIN, 0, 1)], 0,
     [[9, 1, 3, 7, 7]]),
    ("a compacting copy", [[], [1, 1], [], [0]], [], [], 0, [[], [1, 1], [], [0]]),
]
