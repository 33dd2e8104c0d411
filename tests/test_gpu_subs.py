"""GPU: hvws_subs_update (include/hvws.h) against the contract restated in
tests/wssubs.py, field for field: both output arrays, *out_nmember,
hvws_subs_count and the four counts of hvws_get_subs_counts.  Where the call
takes dest_of, the closed connections come from a real turn -- scan,
hvws_messages_rfc, hvws_check, hvws_replies_checked (tests/test_gpu_fanout.py's
`replied`) -- so the implicit drops are read from the device's own flags.

Shapes are the smallest that can still go wrong: listing and event counts around
the 64-lane wave, the 256-thread block and the sort's 2048-pair tile; ndest and
ntopics at which the number of 8-bit sort passes changes (the largest
destination key is ndest - 1: 256 | 257 and 65536 | 65537; the largest topic key
is ntopics, a DROP's: 255 | 256 and 65535 | 65536) and the ones either side."""
from __future__ import annotations

import contextlib
import ctypes
import random

import numpy as np
import pytest

import libhv_amd
import test_gpu_fanout as F
import wsfan as W
import wsrfc as R
import wssubs as U

pytestmark = pytest.mark.gpu

JOIN, LEAVE, DROP, UNIQUE = U.JOIN, U.LEAVE, U.DROP, U.UNIQUE
FIN, MASK = F.FIN, F.MASK
B, text = F.B, F.text
SENT = 0xA5
PAD = 64
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]


class Out:
    """The second table, sentinel-filled: first_out with PAD bytes behind it,
    member_out of member_cap ids with PAD bytes behind them."""

    def __init__(self, eng, ntopics: int, member_cap: int):
        self.eng, self.nt, self.cap = eng, ntopics, member_cap
        self.fbytes, self.mbytes = 8 * (ntopics + 1) + PAD, 4 * member_cap + PAD
        self.first, self.member = eng.alloc(self.fbytes), eng.alloc(self.mbytes)
        self.fill()

    def fill(self):
        self.first.upload(np.full(self.fbytes, SENT, np.uint8))
        self.member.upload(np.full(self.mbytes, SENT, np.uint8))

    def read(self, newn: int):
        """(topic_first_out, member_out[0 .. newn)); everything else must still be the sentinel."""
        f, m = self.first.download(self.fbytes), self.member.download(self.mbytes)
        assert (f[8 * (self.nt + 1):] == SENT).all(), "a write behind d_topic_first_out"
        assert (m[4 * newn:] == SENT).all(), "a write at or beyond the new nmember"
        return f[:8 * (self.nt + 1)].view(np.uint64).copy(), m[:4 * newn].view(np.uint32).copy()

    def untouched(self) -> bool:
        return bool((self.first.download(self.fbytes) == SENT).all() and (self.member.download(self.mbytes) == SENT).all())

    def free(self):
        self.eng.sync()
        self.first.free()
        self.member.free()


@contextlib.contextmanager
def out_table(eng, ntopics: int, member_cap: int):
    o = Out(eng, ntopics, member_cap)
    try:
        yield o
    finally:
        o.free()


def none_yet(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 4)()
    return L.hvws_subs_count(eng.ctx) == -1 and L.hvws_get_subs_counts(eng.ctx, out) != 0


def compare(eng, topics, ndest: int, events, flags: int = 0, dest_of=None, closed=(), slack: int = 3, sub=None):
    """One call on the device against the model; returns (the model's result, the two arrays as bytes)."""
    want_first, want_member, want_counts, rows = U.update(topics, closed, events, flags)
    newn = len(want_member)
    with contextlib.ExitStack() as st:
        df, dm, nt, nm = sub if sub is not None else st.enter_context(F.subscriptions(eng, topics))
        o = st.enter_context(out_table(eng, nt, newn + slack))
        n = eng.subs_update(df, dm, nt, nm, ndest, events, dest_of, o.first, o.member, o.cap, flags)
        assert n == newn == eng.last_subs_nmember == libhv_amd.lib().hvws_subs_count(eng.ctx)
        assert eng.subs_counts() == want_counts
        first, member = o.read(newn)
        assert first.tolist() == want_first.tolist()
        assert member.tolist() == want_member.tolist()
    return rows, (first.tobytes(), member.tobytes())


def table_of(rng, nlist: int, ntopics: int, ndest: int):
    """nlist listings over ntopics rows, most rows empty."""
    rows = [[] for _ in range(ntopics)]
    full = sorted(rng.sample(range(ntopics), min(ntopics, 5)))
    for _ in range(nlist):
        rows[rng.choice(full)].append(rng.randrange(ndest))
    return rows


def events_of(rng, n: int, topics, ndest: int):
    pool = sorted({d for m in topics for d in m})[:40]
    live = [t for t, m in enumerate(topics) if m] or [0]
    ev = []
    for _ in range(n):
        op = rng.choice((JOIN, JOIN, JOIN, LEAVE, LEAVE, DROP))
        if op == DROP and rng.random() < 0.9:
            op = JOIN                       # few DROPs: each one empties a destination for good
        t = rng.choice(live) if rng.random() < 0.8 else rng.randrange(len(topics))
        d = rng.choice(pool) if pool and rng.random() < 0.6 else rng.randrange(ndest)
        ev.append((op, t, d))
    return ev


# ---- counts around the wave, the block and the sort's tile ---------------------------------

@pytest.mark.parametrize("nlist", SIZES)
def test_listing_counts(eng, nlist):
    rng = random.Random(1000 + nlist)
    topics = table_of(rng, nlist, 9, 50)
    compare(eng, topics, 50, events_of(rng, 65, topics, 50), rng.choice((0, UNIQUE)))


@pytest.mark.parametrize("nev", SIZES)
def test_event_counts(eng, nev):
    rng = random.Random(2000 + nev)
    topics = table_of(rng, 300, 9, 50)
    events = events_of(rng, nev, topics, 50)
    compare(eng, topics, 50, events, 0)
    compare(eng, topics, 50, events, UNIQUE)


def test_nothing_at_all(eng):
    """No listing, no event, no closed connection: NULL member arrays are allowed."""
    with F.subscriptions(eng, [[], []]) as (df, dm, nt, nm), out_table(eng, 2, 0) as o:
        assert eng.subs_update(df, None, nt, 0, 1, [], None, o.first, None, 0) == 0
        first, member = o.read(0)
        assert first.tolist() == [0, 0, 0] and eng.subs_counts() == (0, 0, 0, 0)
    compare(eng, [], 3, [(DROP, 0, 2)])          # no topics either: only a DROP is a valid event


# ---- rows ---------------------------------------------------------------------------------

def test_one_topic(eng):
    rng = random.Random(5)
    topics = [[rng.randrange(30) for _ in range(700)]]
    compare(eng, topics, 30, [(rng.choice((JOIN, LEAVE)), 0, rng.randrange(30)) for _ in range(90)] + [(DROP, 0, 3)])


def test_empty_rows_before_between_and_after_full_ones(eng):
    rng = random.Random(6)
    topics = [[] for _ in range(40)]
    for t in (7, 8, 20, 33):
        topics[t] = [rng.randrange(100) for _ in range(rng.choice((1, 70, 300)))]
    events = [(JOIN, 0, 5), (JOIN, 39, 6), (JOIN, 19, 7), (LEAVE, 8, topics[8][0]), (JOIN, 21, 1), (DROP, 0, topics[20][0]),
              (LEAVE, 3, 9)]
    compare(eng, topics, 100, events)


def test_one_row_of_5000_beside_empty_ones(eng):
    rng = random.Random(7)
    huge = [rng.randrange(8, 500) for _ in range(5000)]
    topics = [[], [], [], huge, [], [], [9], []]
    events = [(LEAVE, 3, huge[0]), (LEAVE, 3, huge[4999]), (DROP, 0, huge[2500]), (JOIN, 3, 2), (JOIN, 0, 2), (JOIN, 7, 2),
              (LEAVE, 6, 9)]
    rows, _ = compare(eng, topics, 500, events)
    assert len(rows[3]) < 5000 and rows[6] == []


# ---- the number of sort passes --------------------------------------------------------------

@pytest.mark.parametrize("ndest", [1, 255, 256, 257, 65535, 65536, 65537])
def test_sort_passes_by_destination(eng, ndest):
    """Destinations that differ only in one digit of the key, for every digit:
    the joined listings of a row come out in destination order."""
    rng = random.Random(ndest)
    pool = sorted({0, 1 % ndest, 255 % ndest, 256 % ndest, 257 % ndest, 65535 % ndest, 65536 % ndest, ndest - 1,
                   (ndest - 1) & ~0xFF, (ndest - 1) & 0xFF})
    topics = [[rng.choice(pool) for _ in range(20)], [], [pool[-1]]]
    events = [(rng.choice((JOIN, JOIN, LEAVE)), rng.randrange(3), rng.choice(pool)) for _ in range(70)] + [(DROP, 0, pool[0])]
    rng.shuffle(events)
    rows, _ = compare(eng, topics, ndest, events)
    compare(eng, topics, ndest, events, UNIQUE)


@pytest.mark.parametrize("ntopics", [1, 254, 255, 256, 257, 65534, 65535, 65536, 65537])
def test_sort_passes_by_topic(eng, ntopics):
    rng = random.Random(ntopics)
    pool = sorted({0, 1 % ntopics, 255 % ntopics, 256 % ntopics, 65535 % ntopics, 65536 % ntopics, ntopics - 1,
                   (ntopics - 1) & ~0xFF, (ntopics - 1) & 0xFF})
    topics = [[] for _ in range(ntopics)]
    for t in pool:
        topics[t] = [rng.randrange(12) for _ in range(6)]
    events = [(rng.choice((JOIN, JOIN, LEAVE)), rng.choice(pool), rng.randrange(12)) for _ in range(70)]
    events += [(DROP, ntopics + 5, 3), (DROP, 0, 4)]
    rng.shuffle(events)
    compare(eng, topics, 12, events)


# ---- pair histories ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", U.HAND_CASES, ids=[c[0] for c in U.HAND_CASES])
def test_hand_cases(eng, case):
    """Every hand case of tests/test_subs_oracle.py; `closed` there comes from a
    turn here when there is one to close."""
    _, topics, closed, events, flags, want = case
    ndest = 10
    if not closed:
        rows, _ = compare(eng, topics, ndest, events, flags)
    else:
        # connection 0 CLOSEs, connection 1 does not; both sit on the closed id's neighbours
        row = [B([text(b"bye"), (8 | FIN | MASK, b"\x03\xe8", F.K2)]), B([text(b"stay")])]
        dest_of = [closed[0], 9]
        with F.replied(eng, row, classes=F.CLASSES) as t:
            assert U.closed_dests(t.flags, dest_of) == [closed[0]]
            rows, _ = compare(eng, topics, ndest, events, flags, dest_of, [closed[0]])
    assert rows == want


@pytest.mark.parametrize("op", [JOIN, LEAVE, DROP])
def test_every_op_first_and_last(eng, op):
    topics = [[1, 2, 3], [2, 2, 4]]
    mid = [(JOIN, 1, 1), (LEAVE, 0, 2), (JOIN, 0, 2), (JOIN, 1, 3)]
    compare(eng, topics, 6, [(op, 0, 2)] + mid + [(op, 1, 2)])
    compare(eng, topics, 6, [(op, 1, 3)] + mid + [(op, 0, 3)], UNIQUE)


@pytest.mark.parametrize("nev", [64, 2049])
def test_all_events_on_one_pair(eng, nev):
    rng = random.Random(nev)
    events = [(rng.choice((JOIN, JOIN, JOIN, LEAVE)), 1, 4) for _ in range(nev)]
    assert any(op == LEAVE for op, _, _ in events)
    tail = 0                                   # the JOINs behind the last LEAVE
    while events[nev - 1 - tail][0] == JOIN:
        tail += 1
    rows, _ = compare(eng, [[4], [4, 5, 4]], 6, events)
    assert rows[1].count(4) == tail and rows[0] == [4]
    compare(eng, [[4], [4, 5, 4]], 6, events, UNIQUE)
    joins = [(JOIN, 1, 4)] * nev
    rows, _ = compare(eng, [[4], [5]], 6, joins)
    assert rows[1] == [5] + [4] * nev
    assert compare(eng, [[4], [5]], 6, joins, UNIQUE)[0][1] == [5, 4]


def test_all_events_drops(eng):
    rng = random.Random(9)
    topics = [[rng.randrange(40) for _ in range(100)] for _ in range(3)]
    rows, _ = compare(eng, topics, 40, [(DROP, rng.randrange(1 << 32), rng.randrange(20)) for _ in range(300)])
    assert all(d >= 20 for m in rows for d in m) or not any(rows)


# ---- behind a real turn -------------------------------------------------------------------------

def test_random_cases_behind_a_turn(eng):
    """hvws_check + hvws_replies_checked decide who is closed (CLOSE frames and
    failing connections are in the reads); the update runs with and without
    dest_of, before and after hvws_fanout in the turn, and leaves the fanout's
    tables standing."""
    rng = random.Random(4242)
    some_closed = some_failed = 0
    for case in range(40):
        reads, topics, ndest, pub, dest_of, fflags, events, flags = U.random_case(rng)
        with F.replied(eng, reads, classes=F.CLASSES) as t, F.subscriptions(eng, topics) as sub:
            closed = U.closed_dests(t.flags, dest_of)
            some_closed += bool(closed)
            some_failed += any(f & libhv_amd.RF_FAILED for f in t.flags)
            a = compare(eng, topics, ndest, events, flags, dest_of, closed, sub=sub)
            b = compare(eng, topics, ndest, events, flags, None, (), sub=sub)
            want = F.compare(eng, t, topics, ndest, pub, dest_of, fflags, sub=sub)
            assert compare(eng, topics, ndest, events, flags, dest_of, closed, sub=sub) == a
            assert compare(eng, topics, ndest, events, flags, None, (), sub=sub) == b
            table, reply = eng.fanout_table()       # the fanout's tables still stand
            assert [tuple(int(x) for x in r) for r in table.tolist()] == want[0] and reply.tolist() == want[1]
    assert some_closed >= 5 and some_failed >= 1


def test_two_turns(eng):
    """Turn 1 delivers through table A and updates it into B; connection 1 closed
    in turn 1 and connection 2 failed, so turn 2's fanout over B -- the device's
    arrays, never seen by the host -- gives them nothing."""
    row1 = [B([text(b"hello room")]), B([text(b"last words"), (8 | FIN | MASK, b"\x03\xe8", F.K2)]),
            B([text(b"ok"), (0 | FIN | MASK, b"stray", F.K2)]), b""]
    dest1 = [0, 1, 2, 3]
    A = [[0, 1, 2, 3, 5], [1, 2], [3, 1, 1]]
    ndest = 8
    events = [(JOIN, 1, 6), (LEAVE, 0, 5), (JOIN, 2, 0), (JOIN, 0, 7)]
    with F.subscriptions(eng, A) as subA, out_table(eng, 3, 16) as o:
        with F.replied(eng, row1, classes=F.CLASSES) as t:
            assert t.flags[1] & libhv_amd.RF_CLOSED and t.flags[2] & libhv_amd.RF_FAILED and not t.flags[0] & 1
            closed = U.closed_dests(t.flags, dest1)
            assert closed == [1, 2]
            F.compare(eng, t, A, ndest, [0, 0, 1, F.NONE], dest1, 0, sub=subA)
            rows = U.sequential(A, closed, events, UNIQUE)
            newn = eng.subs_update(subA[0], subA[1], 3, subA[3], ndest, events, dest1, o.first, o.member, 16, UNIQUE)
            assert newn == sum(len(m) for m in rows) and rows == [[0, 3, 7], [6], [3, 0]]
            assert eng.subs_counts() == (3, 3, 7, 2)
        row2 = [B([text(b"turn two")]), B([text(b"to topic 2", 2), (9 | FIN | MASK, b"p", F.K2)])]
        with F.replied(eng, row2) as t:
            want = F.compare(eng, t, rows, ndest, [0, 2], [3, 4], 0, sub=(o.first, o.member, 3, newn))
            assert want[3][1] == 0 and want[3][2] == 0 and want[3][5] == 0
            assert want[3][0] == 2 and want[3][7] == 1 and want[3][3] == 1 and want[3][4] == 1


# ---- determinism, the timed span ---------------------------------------------------------------

def test_the_same_call_twice_gives_identical_bytes(eng):
    rng = random.Random(77)
    topics = [[rng.randrange(64) for _ in range(900)] for _ in range(5)]
    events = [(rng.choice((JOIN, JOIN, LEAVE, DROP)), rng.randrange(5), rng.randrange(64)) for _ in range(2500)]
    seen = [compare(eng, topics, 64, events, UNIQUE)[1] for _ in range(2)]
    assert seen[0] == seen[1] and len(seen[0][0]) == 8 * 6
    ms = ctypes.c_float(-1.0)
    assert libhv_amd.lib().hvws_last_kernel_ms(eng.ctx, ctypes.byref(ms)) == 0 and 0.0 < ms.value < 1000.0


# ---- errors ---------------------------------------------------------------------------------

def test_every_einval_of_the_contract(eng):
    L = libhv_amd.lib()
    topics = [[0, 1, 2], [2], [1, 3]]
    first, member = W.flatten(topics)
    good = [(JOIN, 0, 3), (LEAVE, 1, 2), (DROP, 99, 1)]
    with F.subscriptions(eng, topics) as (df, dm, nt, nm), out_table(eng, 3, 8) as o:
        def call(**kw):
            a = dict(topic_first=df, member=dm, ntopics=nt, nmember=nm, ndest=4, events=good, dest_of=None,
                     topic_first_out=o.first, member_out=o.member, member_cap=8, flags=0)
            a.update(kw)
            return eng.subs_update(**a)

        def fails(**kw) -> int:
            with pytest.raises(libhv_amd.HvwsError):
                call(**kw)
            assert none_yet(eng) and o.untouched()
            return eng.last_subs_nmember

        want = U.update(topics, [], good)
        need = len(want[1])
        assert call() == need == 4 and not none_yet(eng)
        assert o.read(need)[1].tolist() == want[1].tolist()
        o.fill()
        # events
        for bad in ((0, 0, 0), (4, 0, 0), (JOIN, 3, 0), (LEAVE, 3, 0), (JOIN, 0, 4), (LEAVE, 0, 4), (DROP, 0, 4)):
            fails(events=good + [bad])
            fails(events=[bad] + good)
        # arguments
        fails(flags=2)
        fails(flags=UNIQUE | 4)
        fails(ndest=0, events=[])
        fails(ndest=1 << 31)
        fails(nmember=(1 << 32) - 1)
        n = ctypes.c_uint64(0)
        ev = np.zeros(4, libhv_amd.SUB_EVENT_DTYPE)
        assert L.hvws_subs_update(eng.ctx, df.ptr, dm.ptr, nt, nm, 4, ev.ctypes.data, (1 << 32) - 1, None, 0,
                                  o.first.ptr, o.member.ptr, 8, ctypes.byref(n)) == -2
        assert none_yet(eng) and o.untouched()
        # NULL tables where they are needed
        fails(topic_first=None)
        fails(member=None)
        fails(topic_first_out=None)
        fails(member_out=None)
        assert L.hvws_subs_update(eng.ctx, df.ptr, dm.ptr, nt, nm, 4, None, 1, None, 0, o.first.ptr, o.member.ptr, 8,
                                  ctypes.byref(n)) == -2
        # an output over an input, an output over the other output, a misaligned output
        fails(topic_first_out=df)
        fails(member_out=dm)
        fails(member_out=df)
        fails(topic_first_out=dm)
        fails(member_out=o.first)
        fails(topic_first_out=o.first.ptr + 8)
        fails(member_out=o.member.ptr + 4)
        # member_cap: the need passes, one below fails and still reports the need
        assert call(member_cap=need) == need
        o.fill()
        assert fails(member_cap=need - 1) == need
        assert call(events=[(DROP, 0, d) for d in range(4)], member_out=None, member_cap=0) == 0
        o.fill()
        # dest_of: an entry >= ndest; a scan since the reply call
        row = [B([text(b"a"), (8 | FIN | MASK, b"\x03\xe8", F.K2)]), B([text(b"b")])]
        data, segs, _, _, _ = R.Chain(2).inputs(row)
        with F.replied(eng, row, classes=F.CLASSES) as t:
            assert call(dest_of=[2, 0]) == len(U.update(topics, [2], good)[1])
            o.fill()
            fails(dest_of=[2, 4])
            rx = eng.to_device(np.frombuffer(data, np.uint8))
            try:
                eng.scan(rx, len(data), segs)
                fails(dest_of=[2, 0])
                assert call() == need                # without dest_of no reply call is needed
                o.fill()
            finally:
                eng.sync()
                rx.free()
    # dest_of on a context that never ran a reply call
    with libhv_amd.Engine(0) as fresh, F.subscriptions(fresh, topics) as (df, dm, nt, nm), out_table(fresh, 3, 8) as o:
        with pytest.raises(libhv_amd.HvwsError):
            fresh.subs_update(df, dm, nt, nm, 4, good, [0], o.first, o.member, 8)
        assert none_yet(fresh) and o.untouched()
        assert fresh.subs_update(df, dm, nt, nm, 4, good, None, o.first, o.member, 8) == 4
    # tables that are not dense, and a member id outside the destinations: found on the device
    for bad_first, bad_member in (([1, 3, 4, 6], member), ([0, 4, 3, 6], member), ([0, 3, 4, 5], member),
                                  ([0, 3, 4, 7], member), (first, [0, 1, 2, 2, 1, 4])):
        df, dm = eng.to_device(np.array(bad_first, np.uint64)), eng.to_device(np.array(bad_member, np.uint32))
        with out_table(eng, 3, 8) as o:
            try:
                for ev in (good, []):
                    with pytest.raises(libhv_amd.HvwsError):
                        eng.subs_update(df, dm, 3, 6, 4, ev, None, o.first, o.member, 8)
                    assert none_yet(eng) and o.untouched()
            finally:
                eng.sync()
                df.free()
                dm.free()
