"""Oracle for hvws_budget (include/hvws.h): the contract in plain Python -- every
destination's deliveries of a tests/wsfan.py fanout() result cut at that
destination's byte budget by hio_write's rule (reference event/nio.c:554-560) at
message granularity, the dense table of what is kept, and every destination's
byte range in the send that follows.  Wire sizes are wssend.closed_form.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import wssend as S

BF_OVER = 1
UNLIMITED = (1 << 64) - 1


def wire(length: int, fragment: int, masked: bool) -> int:
    """The bytes hvws_send_messages emits for one message of `length` bytes."""
    return S.closed_form(length, fragment, masked)[1]


def sizes(table, fragment: int = 0, masked: bool = False) -> List[int]:
    return [wire(r[1], fragment, masked) for r in table]


def prefix_sums(fan, fragment: int = 0, masked: bool = False) -> List[List[int]]:
    """Per destination, c_k of its deliveries in table order."""
    table, _, first, count = fan
    w = sizes(table, fragment, masked)
    out = []
    for d in range(len(first)):
        c, run = [], 0
        for k in range(first[d], first[d] + count[d]):
            run += w[k]
            c.append(run)
        out.append(c)
    return out


def budget(fan, budgets: Optional[Sequence[int]], budget_all: int = UNLIMITED, fragment: int = 0,
           masked: bool = False):
    """fan: (table, reply, first, count) of wsfan.fanout; budgets: one per
    destination, or None: budget_all for all.  -> (kept table, reply_out, first2,
    count2, byte_off [ndest + 1], flags, totals (kept deliveries, kept bytes,
    dropped deliveries, destinations over))."""
    table, reply, first, count = fan
    ndest = len(first)
    w = sizes(table, fragment, masked)
    kept, reply_out = [], []
    first2, count2, byte_off, flags = [], [], [0], []
    for d in range(ndest):
        b = budget_all if budgets is None else budgets[d]
        c, m = 0, 0
        for k in range(first[d], first[d] + count[d]):
            if c + w[k] > b:          # the first that does not fit: nothing at or behind it goes out
                break
            c += w[k]
            m += 1
        first2.append(len(kept))
        count2.append(m)
        flags.append(BF_OVER if m < count[d] else 0)
        kept += table[first[d]:first[d] + m]
        reply_out += reply[first[d]:first[d] + m]
        byte_off.append(byte_off[-1] + c)
    totals = (len(kept), byte_off[-1], len(table) - len(kept), sum(1 for f in flags if f))
    return kept, reply_out, first2, count2, byte_off, flags, totals


def simulate(fan, budgets: Sequence[int], fragment: int = 0, masked: bool = False) -> Tuple[List[int], List[int]]:
    """hio_write's rule, one write per message, walked over the table as a
    server would: a running write_bufsize per destination (the budget is
    max_write_bufsize less what was queued before the turn), the first write that
    would exceed the limit fails and closes the channel, nothing goes out after
    it.  -> (indices of the deliveries written, the destinations closed)."""
    table, _, first, count = fan
    ndest = len(first)
    dest_of = [0] * len(table)
    for d in range(ndest):
        for k in range(first[d], first[d] + count[d]):
            dest_of[k] = d
    queued = [0] * ndest
    closed = [False] * ndest
    written = []
    for k, row in enumerate(table):
        d = dest_of[k]
        if closed[d]:
            continue
        n = wire(row[1], fragment, masked)
        if queued[d] + n > budgets[d]:   # nio.c:556: write_bufsize + len > max_write_bufsize
            closed[d] = True             # ERR_OVER_LIMIT, hio_close
            continue
        queued[d] += n
        written.append(k)
    return written, [d for d in range(ndest) if closed[d]]


def random_budgets(rng, fan, fragment: int = 0, masked: bool = False) -> List[int]:
    """Each non-empty destination's budget a random fraction of its own uncut
    total: 0, the total itself, a prefix sum, one byte less than one, or anything
    between; an empty destination's is arbitrary."""
    out = []
    for c in prefix_sums(fan, fragment, masked):
        if not c:
            out.append(rng.choice((0, 1, UNLIMITED, rng.randrange(1 << 20))))
            continue
        kind = rng.random()
        if kind < 0.15:
            out.append(0)
        elif kind < 0.40:
            out.append(c[-1])
        elif kind < 0.50:
            out.append(UNLIMITED)
        elif kind < 0.65:
            out.append(rng.choice(c))
        elif kind < 0.80:
            out.append(rng.choice(c) - 1)
        else:
            out.append(rng.randint(0, c[-1]))
    return out
