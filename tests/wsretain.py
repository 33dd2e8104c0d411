"""Oracle for hvws_retain (include/hvws.h): the contract in plain Python.  A
sequential server -- a dict topic -> (bytes, flags) walked reply by reply --
gives the store, the d_ret entries, the snapshot rows with topic and reply, the
per-segment ranges and the five totals; beside it the closed form, the largest
publishing reply per topic.  The inputs are what tests/wsroute.py's route()
returns for a turn: the routed rows, topics, kinds and events, with the segment
that sent each reply.

The store is kept sparse -- what the caller seeded it with (`seed`, a byte, for
every slot byte; `entry` for every d_ret entry) and, per topic, what turns wrote
over that -- so a store of a million slots costs what its touched topics cost.

A helper, not a test module."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

from wsroute import JOIN, RK_PUB, RK_SUB, RK_UNSUB

NOTHING = (0, 0, 0)


def is_retained(entry, slot: int) -> bool:
    ln, _, st = entry
    return st == 1 and 0 < ln <= slot


class Store:
    """ntopics slots of `slot` bytes and ntopics (len, flags, set) entries."""

    def __init__(self, ntopics: int, slot: int, seed: int = 0, entry=NOTHING):
        assert slot > 0 and slot % 16 == 0
        self.ntopics, self.slot, self.seed, self.entry = ntopics, slot, seed, tuple(entry)
        self.written: Dict[int, bytes] = {}    # topic -> the bytes written over the front of its slot
        self.ret: Dict[int, Tuple[int, int, int]] = {}   # topic -> its entry, where a turn wrote one

    def copy(self) -> "Store":
        s = Store(self.ntopics, self.slot, self.seed, self.entry)
        s.written, s.ret = dict(self.written), dict(self.ret)
        return s

    def entry_of(self, t: int):
        return self.ret.get(t, self.entry)

    def slot_bytes(self, t: int) -> bytes:
        w = self.written.get(t, b"")
        return w + bytes([self.seed]) * (self.slot - len(w))

    def store_bytes(self) -> bytes:
        return b"".join(self.slot_bytes(t) for t in range(self.ntopics))

    def entries(self) -> List[Tuple[int, int, int]]:
        return [self.entry_of(t) for t in range(self.ntopics)]

    def value(self, t: int):
        """(body, flags) topic t retains, or None."""
        e = self.entry_of(t)
        return (self.slot_bytes(t)[:e[0]], e[1]) if is_retained(e, self.slot) else None

    def values(self) -> dict:
        """topic -> (body, flags) over the topics a turn touched or the seed retains."""
        ts = range(self.ntopics) if is_retained(self.entry, self.slot) else sorted(set(self.ret) | set(self.written))
        return {t: v for t in ts if (v := self.value(t)) is not None}

    def _apply(self, outcome: Dict[int, Tuple[bytes, int]]):
        """The turn's winning (body, flags) per topic into the store; -> (stored,
        cleared empty, cleared oversize, bytes copied)."""
        stored = empty = over = copied = 0
        for t, (body, fl) in outcome.items():
            if 0 < len(body) <= self.slot:
                old = self.written.get(t, b"")
                self.written[t] = body + old[len(body):]   # no byte at or beyond len is written
                self.ret[t] = (len(body), fl, 1)
                stored, copied = stored + 1, copied + len(body)
            else:
                self.ret[t] = NOTHING
                empty, over = empty + (len(body) == 0), over + (len(body) > self.slot)
        return stored, empty, over, copied


def _snapshot(store: Store, kinds, events, sender, nseg: int):
    """The snapshot over the updated store: rows, topic, reply, first / count per segment."""
    rows, topic, reply = [], [], []
    count = [0] * nseg
    ev = iter(events)
    for i, k in enumerate(kinds):
        if k not in (RK_SUB, RK_UNSUB):
            continue
        op, t, _ = next(ev)                  # the events are the SUB / UNSUB replies in reply order
        assert (op == JOIN) == (k == RK_SUB)
        if k == RK_SUB and is_retained(store.entry_of(t), store.slot):
            ln, fl, _ = store.entry_of(t)
            rows.append((t * store.slot, ln, fl, 0))
            topic.append(t)
            reply.append(i)
            count[sender[i]] += 1
    first, at = [0] * nseg, 0
    for s in range(nseg):                    # replies are ordered by segment: a prefix sum
        first[s] = at
        at += count[s]
    assert sorted(reply, key=lambda i: sender[i]) == reply
    return rows, topic, reply, first, count


def sequential(store: Store, rows, topics: Sequence[int], kinds: Sequence[int], events, sender: Sequence[int],
               nseg: int, out: bytes):
    """One turn of the sequential server on `store` (updated in place) -> (snapshot
    rows [(off, len, flags, key)], topic, reply, first [nseg], count [nseg],
    totals (stored, cleared empty, cleared oversize, bytes copied, snapshot rows))."""
    said: Dict[int, Tuple[bytes, int]] = {}
    for r, t, k in zip(rows, topics, kinds):          # the update: every publication replaces its topic's value
        if k == RK_PUB:
            off, ln, fl, _ = (int(x) for x in r)
            said[t] = (bytes(out[off:off + ln]), fl)
    totals = store._apply(said)
    snap = _snapshot(store, kinds, events, sender, nseg)
    return snap + (totals + (len(snap[0]),),)


def winners(topics: Sequence[int], kinds: Sequence[int]) -> Dict[int, int]:
    """topic -> the largest reply index of kind PUB that names it."""
    return {t: max(i for i, (u, k) in enumerate(zip(topics, kinds)) if k == RK_PUB and u == t)
            for t in {u for u, k in zip(topics, kinds) if k == RK_PUB}}


def closed_form(store: Store, rows, topics, kinds, events, sender, nseg: int, out: bytes):
    """sequential(), from the winners alone."""
    said = {}
    for t, i in winners(topics, kinds).items():
        off, ln, fl, _ = (int(x) for x in rows[i])
        said[t] = (bytes(out[off:off + ln]), fl)
    totals = store._apply(said)
    snap = _snapshot(store, kinds, events, sender, nseg)
    return snap + (totals + (len(snap[0]),),)
