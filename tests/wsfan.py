"""Oracle for hvws_fanout (include/hvws.h): the contract in plain Python -- the
edge list of a reply table under a subscription table, the sort by the
four-part key (destination, opcode == 8, reply, listing), and first / count per
destination.  It takes a reply table as tests/wssend.py (replies_of_pieces) and
tests/wsrfc.py / tests/wscheck.py (replies_of, replies_checked_of) produce it:
replies [(off, len, flags, key)] and the piece each answers, beside the piece
table whose `seg` says who sent it.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

FAN_NONE, FAN_SELF = 0xFFFFFFFF, 1


def flatten(topics: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """[[member ids] per topic] -> (topic_first [ntopics + 1], member [nmember])."""
    first = np.zeros(len(topics) + 1, np.uint64)
    for t, m in enumerate(topics):
        first[t + 1] = first[t] + len(m)
    member = np.array([d for m in topics for d in m], np.uint32)
    return first, member


def senders(pieces, answered: Sequence[int]) -> List[int]:
    """The segment of the piece each reply answers."""
    return [int(pieces[p]["seg"]) for p in answered]


def edges(replies, sender: Sequence[int], topics: Sequence[Sequence[int]], pub: Optional[Sequence[int]],
          dest_of: Sequence[int], flags: int = 0) -> List[Tuple[int, int, int, int]]:
    """[(destination, opcode == 8, reply i, listing j)] in (i, j) order."""
    out = []
    for i, (r, s) in enumerate(zip(replies, sender)):
        op = r[2] & 0xF
        if op in (1, 2):
            t = pub[s] if pub is not None else FAN_NONE
            if t == FAN_NONE:
                continue
            for j, d in enumerate(topics[t]):
                if d == dest_of[s] and not flags & FAN_SELF:
                    continue
                out.append((int(d), 0, i, j))
        else:
            out.append((int(dest_of[s]), 1 if op == 8 else 0, i, 0))
    return out


def fanout(replies, sender: Sequence[int], topics: Sequence[Sequence[int]], ndest: int,
           pub: Optional[Sequence[int]], dest_of: Sequence[int], flags: int = 0):
    """-> (deliveries [(off, len, flags, key)], reply of each delivery, first
    [ndest], count [ndest])."""
    es = sorted(edges(replies, sender, topics, pub, dest_of, flags))
    table = [tuple(int(x) for x in replies[i]) for _, _, i, _ in es]
    reply = [i for _, _, i, _ in es]
    count = [0] * ndest
    for d, _, _, _ in es:
        count[d] += 1
    first, at = [0] * ndest, 0
    for d in range(ndest):
        first[d] = at
        at += count[d]
    return table, reply, first, count


def random_case(rng, max_conn: int = 8, max_topics: int = 6, max_dest: int = 40):
    """A small turn: (reads [one bytes per connection], topics, ndest, pub,
    dest_of, flags).  Every opcode occurs: whole and fragmented text / binary
    messages, PINGs (between fragments too), PONGs, CLOSEs and frames after them,
    empty reads; topics with repeated, foreign and no members; connections that
    publish nowhere."""
    import wsharness as H

    FIN, MASK = 0x10, 0x20
    key = lambda: bytes(rng.randrange(256) for _ in range(4))
    body = lambda: bytes(rng.randrange(256) for _ in range(rng.randint(0, 20)))
    nconn = rng.randint(1, max_conn)
    ndest = rng.randint(nconn, max_dest)
    dest_of = rng.sample(range(ndest), nconn)
    reads = []
    for _ in range(nconn):
        frames = []
        for _ in range(rng.randint(0, 6)):
            kind = rng.random()
            if kind < 0.35:
                frames.append((rng.choice((1, 2)) | FIN | MASK, body(), key()))
            elif kind < 0.55:
                frames.append((rng.choice((1, 2)) | MASK, body(), key()))
                if rng.random() < 0.5:
                    frames.append((9 | FIN | MASK, body(), key()))
                if rng.random() < 0.3:
                    frames.append((0 | MASK, body(), key()))
                frames.append((0 | FIN | MASK, body(), key()))
            elif kind < 0.75:
                frames.append((9 | FIN | MASK, body(), key()))
            elif kind < 0.85:
                frames.append((10 | FIN | MASK, body(), key()))
            elif kind < 0.93:
                frames.append((8 | FIN | MASK, b"\x03\xe8" + body(), key()))
            else:
                frames.append((0 | FIN | MASK, body(), key()))
        reads.append(H.build_frames_ref(frames) if frames else b"")
    ntopics = rng.randint(0, max_topics)
    topics = []
    for _ in range(ntopics):
        pool = dest_of if rng.random() < 0.5 else list(range(ndest))
        topics.append([rng.choice(pool) for _ in range(rng.choice((0, 1, 2, 5, 12)))])
    pub = [rng.randrange(ntopics) if ntopics and rng.random() < 0.8 else FAN_NONE for _ in range(nconn)]
    return reads, topics, ndest, pub, dest_of, rng.choice((0, FAN_SELF))


def destination_frames(out: bytes, table, first: Sequence[int], count: Sequence[int], fragment: int = 0) -> List[bytes]:
    """Per destination, the bytes a send of the delivery table over `out` (the
    message call's output) must put in its range: its deliveries' frames, back
    to back, as the reference builds them (tests/wssend.py expected)."""
    import wssend as S

    res = []
    for d in range(len(first)):
        msgs = [(fl, out[o:o + ln], 0) for o, ln, fl, _ in table[first[d]:first[d] + count[d]]]
        res.append(S.expected(msgs, fragment, False)[0])
    return res
