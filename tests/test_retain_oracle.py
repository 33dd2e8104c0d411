"""CPU: the two forms of hvws_retain's contract in tests/wsretain.py agree -- the
sequential server and the closed form over the largest publishing reply per
topic -- on random turns built with tests/wsroute.py, and a turn split in two
leaves the store the whole turn leaves.  The generator counts the cases the
contract names and the test asserts each occurred, so that random inputs cannot
hide one."""
from __future__ import annotations

import collections
import random

import wsretain as R
import wsroute as T

FIN = 0x10
SLOT = 16          # random_message's bodies are 0 .. 20 bytes: five lengths are oversize
NTOPICS = 5


def turn(rng, max_conn: int = 5):
    """(replies, sender, out, dest_of): connections each sending a few routed
    messages, a PONG now and then, their bytes laid out as a message call leaves
    them (gaps between messages, replies ordered by segment)."""
    nconn = rng.randint(1, max_conn)
    dest_of = rng.sample(range(3 * max_conn), nconn)
    out, replies, sender = bytearray(), [], []
    for s in range(nconn):
        for _ in range(rng.randint(0, 6)):
            out += bytes(rng.randrange(256) for _ in range(rng.randint(0, 3)))
            if rng.random() < 0.1:
                msg, fl = b"ping", 10 | FIN
            else:
                msg, fl = T.random_message(rng, NTOPICS), rng.choice((1, 2)) | FIN
            replies.append((len(out), len(msg), fl, 0))
            sender.append(s)
            out += msg
    return replies, sender, bytes(out), dest_of


def routed(replies, sender, out, dest_of):
    rows, topics, kinds, events, _, _, _ = T.route(replies, sender, out, NTOPICS, dest_of)
    return rows, topics, kinds, events


def count_cases(seen, store, replies, sender, out, rows, topics, kinds, events, after):
    """Which of the contract's cases this turn holds; `store` is the store before it, `after` the one behind it."""
    pubs = collections.defaultdict(list)
    for i, (t, k) in enumerate(zip(topics, kinds)):
        if k == T.RK_PUB:
            pubs[t].append(i)
    for t, idx in pubs.items():
        who = [sender[i] for i in idx]
        seen["twice by one segment"] += any(who.count(s) > 1 for s in who)
        seen["by two segments"] += len(set(who)) > 1
        ln = rows[idx[-1]][1]
        was = store.value(t) is not None
        seen["empty clears a set topic"] += was and ln == 0
        seen["oversize clears a set topic"] += was and ln > SLOT
    for i, k in enumerate(kinds):
        if k == T.RK_STOPPED:
            off, ln, _, _ = replies[i]
            seen["publication behind a BAD reply"] += T.parse(out[off:off + ln], NTOPICS)[0] == T.RK_PUB
    for op, t, _ in events:
        if op == T.JOIN:
            seen["JOIN of a retained topic"] += after.value(t) is not None
            seen["JOIN of an unretained topic"] += after.value(t) is None
            seen["JOIN and publication of one topic"] += t in pubs


CASES = ("twice by one segment", "by two segments", "publication behind a BAD reply", "empty clears a set topic",
         "oversize clears a set topic", "JOIN of a retained topic", "JOIN of an unretained topic",
         "JOIN and publication of one topic")


def test_the_two_forms_agree_on_3000_random_turns():
    rng = random.Random(416)
    seen = collections.Counter()
    a = b = None
    for n in range(3000):
        if n % 6 == 0:      # a fresh store now and then, seeded with garbage that retains nothing
            a = R.Store(NTOPICS, SLOT, seed=0xA5, entry=(0xA5A5, 7, 0xA5A5A5A5))
            b = a.copy()
        replies, sender, out, dest_of = turn(rng)
        rows, topics, kinds, events = routed(replies, sender, out, dest_of)
        before = a.copy()
        got = R.sequential(a, rows, topics, kinds, events, sender, len(dest_of), out)
        want = R.closed_form(b, rows, topics, kinds, events, sender, len(dest_of), out)
        assert got == want
        assert a.store_bytes() == b.store_bytes() and a.entries() == b.entries()
        count_cases(seen, before, replies, sender, out, rows, topics, kinds, events, a)
        # what the snapshot rows say is what the store holds; nothing outside a stored body moved
        snap, topic, reply, first, count, totals = got
        for (off, ln, fl, key), t, i in zip(snap, topic, reply):
            assert kinds[i] == T.RK_SUB and off == t * SLOT and key == 0 and (a.store_bytes()[off:off + ln], fl) == a.value(t)
        assert sum(count) == len(snap) == totals[4] and all(f == sum(count[:s]) for s, f in enumerate(first))
        for t in range(NTOPICS):
            if not any(k == T.RK_PUB and u == t for u, k in zip(topics, kinds)):
                assert (a.slot_bytes(t), a.entry_of(t)) == (before.slot_bytes(t), before.entry_of(t))
            elif a.value(t) is None:
                assert a.entry_of(t) == R.NOTHING and a.slot_bytes(t) == before.slot_bytes(t)
            else:
                ln = a.entry_of(t)[0]
                assert a.slot_bytes(t)[ln:] == before.slot_bytes(t)[ln:]
    for c in CASES:
        assert seen[c] > 0, c


def test_a_turn_split_in_two_leaves_the_same_store():
    """The replies' kinds are the whole turn's (a STOPPED reply stays STOPPED in
    its half).  The same values are retained; only slot bytes beyond a value's
    length may differ, where the first half stored a longer body."""
    rng = random.Random(17)
    for _ in range(500):
        replies, sender, out, dest_of = turn(rng)
        rows, topics, kinds, events = routed(replies, sender, out, dest_of)
        whole = R.Store(NTOPICS, SLOT)
        R.sequential(whole, rows, topics, kinds, events, sender, len(dest_of), out)
        halves = R.Store(NTOPICS, SLOT)
        cut = rng.randint(0, len(rows))
        nev = sum(k in (T.RK_SUB, T.RK_UNSUB) for k in kinds[:cut])
        R.sequential(halves, rows[:cut], topics[:cut], kinds[:cut], events[:nev], sender[:cut], len(dest_of), out)
        R.sequential(halves, rows[cut:], topics[cut:], kinds[cut:], events[nev:], sender[cut:], len(dest_of), out)
        assert halves.values() == whole.values()
        assert [R.is_retained(e, SLOT) for e in halves.entries()] == [R.is_retained(e, SLOT) for e in whole.entries()]


def test_the_oracle_s_entry_is_the_binding_s():
    """(len, flags, set), 16 bytes: what Engine.retain()'s `ret` holds per topic."""
    import numpy as np

    import libhv_amd

    e = np.array([(5, 0x12, 1)], libhv_amd.RETAINED_DTYPE)
    assert libhv_amd.RETAINED_DTYPE.names == ("len", "flags", "set") and e.nbytes == 16
    assert R.is_retained(tuple(int(x) for x in e[0]), 16) and not R.is_retained(tuple(int(x) for x in e[0]), 4)
    assert np.zeros(1, libhv_amd.RETAINED_DTYPE).tobytes() == bytes(16) and R.NOTHING == (0, 0, 0)
    assert callable(libhv_amd.Engine.retain)


def test_the_retained_rule_on_an_entry():
    assert R.is_retained((1, 0, 1), 16) and R.is_retained((16, 0x11, 1), 16)
    for e in ((0, 0, 1), (17, 0, 1), (5, 0, 0), (5, 0, 2), (0, 0, 0)):
        assert not R.is_retained(e, 16), e


def test_a_resubscribe_gets_a_snapshot_again_and_a_clear_gets_none():
    s = R.Store(3, 16)
    out = b"P1\nlast valueS1\nP1\n"
    rows, topics, kinds, events = routed([(0, 13, 1 | FIN, 0), (13, 3, 1 | FIN, 0)], [0, 1], out, [4, 5])
    snap = R.sequential(s, rows, topics, kinds, events, [0, 1], 2, out)
    assert snap[:5] == ([(16, 10, 1 | FIN, 0)], [1], [1], [0, 0], [0, 1]) and snap[5] == (1, 0, 0, 10, 1)
    assert s.value(1) == (b"last value", 1 | FIN)
    rows, topics, kinds, events = routed([(13, 3, 2 | FIN, 0)], [1], out, [4, 5])     # the member subscribes again
    assert R.sequential(s, rows, topics, kinds, events, [1], 2, out)[0] == [(16, 10, 1 | FIN, 0)]
    rows, topics, kinds, events = routed([(13, 3, 1 | FIN, 0), (16, 3, 1 | FIN, 0)], [0, 0], out, [4, 5])
    snap = R.sequential(s, rows, topics, kinds, events, [0, 0], 2, out)              # a JOIN, then an empty publication
    assert snap[0] == [] and snap[5] == (0, 1, 0, 0, 0) and s.value(1) is None and s.entry_of(1) == R.NOTHING
