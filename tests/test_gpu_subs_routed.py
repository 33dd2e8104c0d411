"""GPU: hvws_subs_update_routed (include/hvws.h) behind real turns -- scan, a
message call, the reply call, hvws_route, hvws_fanout_routed and hvws_budget as
tests/test_gpu_route.py sets them up.  Three comparisons per case: the merged
event array and its four counts against tests/wsturn.py `merged` over the
device's own flags; both output arrays and all counts against tests/wssubs.py
`update` on that array; the same arrays against hvws_subs_update fed the array
from the host, in the same context.

Shapes are the smallest that can still go wrong: route-event, segment and
destination counts around the 64-lane wave, the 256-thread block and the
scan's 1024-element tile, with a closed or malformed connection and an OVER
destination on those edges; each of the four parts empty in turn."""
from __future__ import annotations

import ctypes
import random

import numpy as np
import pytest

import libhv_amd
import test_gpu_route as Q
import wsfan as W
import wsrfc as R
import wsroute as T
import wssubs as U
import wsturn as N
from test_gpu_subs import none_yet, out_table

pytestmark = pytest.mark.gpu

JOIN, LEAVE, DROP = N.JOIN, N.LEAVE, N.DROP
UNIQUE, OVER = libhv_amd.SUBS_UNIQUE, libhv_amd.SUBS_OVER
SELF = libhv_amd.FAN_SELF
B, text, CLOSE, PING = Q.B, Q.text, Q.CLOSE, Q.PING
EDGES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def triples(a) -> list:
    return [tuple(int(x) for x in e) for e in a.tolist()]


def merged_none(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 4)()
    return L.hvws_get_subs_merged(eng.ctx, out) == -2 and L.hvws_get_subs_events(eng.ctx, None, 0, 0) == -2


def passes(eng, sub, ntopics, ndest, dest_of, budgets=None, fan_flags=0):
    """hvws_route, hvws_fanout_routed and (budgets given) hvws_budget behind the
    reply call; returns what they left for the merge, read from the device:
    (route events, reply flags, route flags, budget flags or None)."""
    df, dm, nm = sub
    eng.route(ntopics, ndest, dest_of)
    eng.fanout_routed(df, dm, nm, fan_flags)
    over = None
    if budgets is not None:
        db = eng.to_device(np.array(budgets, np.uint64))
        try:
            eng.budget(db, 0)
            over = eng.dest_budget(ndest)[3].tolist()
        finally:
            eng.sync()
            db.free()
    n = len(dest_of)
    return triples(eng.route_events()), eng.reply_flags(n).tolist(), eng.route_flags(n)[0].tolist(), over


def update(eng, sub, topics, ndest, dest_of, left, host=(), flags=0, slack=3):
    """hvws_subs_update_routed behind passes() against the three references;
    returns (the merged events, the new rows, the two arrays as bytes)."""
    df, dm, nm = sub
    nt = len(topics)
    ev, rflags, rtflags, over = left
    m = N.merged(ev, rflags, rtflags, dest_of, over, host, flags)
    want_first, want_member, want_counts, rows = U.update(topics, (), m, flags & UNIQUE)
    newn = len(want_member)
    with out_table(eng, nt, newn + slack) as o, out_table(eng, nt, newn + slack) as o2:
        n = eng.subs_update_routed(df, dm, nm, host, o.first, o.member, o.cap, flags)
        # 1. the merged array and its parts
        assert eng.subs_merged() == N.parts(ev, rflags, rtflags, dest_of, over, host, flags)
        assert triples(eng.subs_events()) == m
        L = libhv_amd.lib()
        if m:
            one = np.zeros(1, libhv_amd.SUB_EVENT_DTYPE)
            assert L.hvws_get_subs_events(eng.ctx, one.ctypes.data, len(m) - 1, 1) == 0 and triples(one) == m[-1:]
        assert L.hvws_get_subs_events(eng.ctx, None, 0, len(m) + 1) == -2
        assert L.hvws_get_subs_events(eng.ctx, None, len(m), 0) == 0
        # 2. the table and the counts: hvws_subs_update's contract over M
        assert n == newn == eng.last_subs_nmember == L.hvws_subs_count(eng.ctx)
        assert eng.subs_counts() == want_counts and want_counts[3] == 0
        first, member = o.read(newn)
        assert first.tolist() == want_first.tolist()
        assert member.tolist() == want_member.tolist()
        # 3. hvws_subs_update fed M from the host
        assert eng.subs_update(df, dm, nt, nm, ndest, m, None, o2.first, o2.member, o2.cap, flags & UNIQUE) == newn
        assert eng.subs_counts() == want_counts and merged_none(eng)
        f2, m2 = o2.read(newn)
        assert (f2.tobytes(), m2.tobytes()) == (first.tobytes(), member.tobytes())
    return m, rows, (first.tobytes(), member.tobytes())


def case(eng, row, topics, ndest, dest_of, host=(), flags=0, budgets=None, fan_flags=0, form="rfc", classes=0):
    with Q.replied(eng, row, form, classes) as t, Q.subscriptions(eng, topics) as sub:
        left = passes(eng, sub, len(topics), ndest, dest_of, budgets, fan_flags)
        return update(eng, sub, topics, ndest, dest_of, left, host, flags) + (left,)


# ---- route-event counts on the wave, block and scan-tile edges -------------------------------------

@pytest.mark.parametrize("nev", EDGES)
def test_route_event_counts(eng, nev):
    """nev subscribe / unsubscribe messages over three connections, the last of which also closes."""
    rng = random.Random(nev)
    nt, ndest, dest_of = 5, 40, [5, 39, 0]
    per = [nev // 3 + (1 if c < nev % 3 else 0) for c in range(3)]
    row, at = [], 0
    for c, k in enumerate(per):
        frames = [text(T.header("S" if rng.random() < 0.6 else "U", (i * 7 + c) % nt), 1 + i % 2) for i in range(at, at + k)]
        frames.insert(len(frames) // 2, text(b"P1\nbody"))
        row.append(B(frames + ([CLOSE] if c == 2 else [])))
        at += k
    topics = [[rng.choice(dest_of + [7, 8]) for _ in range(rng.choice((0, 3, 9)))] for _ in range(nt)]
    host = [(JOIN, 2, 0), (LEAVE, 1, 5)]
    m, _, _, left = case(eng, row, topics, ndest, dest_of, host, rng.choice((0, UNIQUE)))
    assert len(left[0]) == nev and m[nev:] == [(DROP, 0, 0)] + host


# ---- segment counts on the same edges, a closed or malformed segment on each -------------------------

@pytest.mark.parametrize("nseg", EDGES[1:])
def test_segment_counts(eng, nseg):
    """One message per connection; the first, the last and every connection on an
    edge closes or sends a malformed message, the others subscribe or publish."""
    rng = random.Random(nseg)
    nt, ndest = 3, nseg + 2
    dest_of = list(range(1, nseg + 1))
    rng.shuffle(dest_of)
    marked = {s for e in EDGES for s in (e - 1, e) if 0 <= s < nseg} | {nseg - 1}
    row, kinds = [], []
    for s in range(nseg):
        if s in marked:
            kinds.append(("close", "bad", "both")[len(kinds) % 3] if nseg > 1 else "close")
        else:
            kinds.append("sub" if rng.random() < 0.5 else "pub")
    for s, k in enumerate(kinds):
        frames = {"close": [text(b"S1\n"), CLOSE], "bad": [text(b"S2\n"), text(b"junk")],
                  "both": [text(b"s1\n"), CLOSE], "sub": [text(b"S%d\n" % (s % nt))], "pub": [text(b"P0\nx")]}[k]
        row.append(B(frames))
    topics = [[rng.choice(dest_of) for _ in range(40)] for _ in range(nt)]
    m, rows, _, left = case(eng, row, topics, ndest, dest_of)
    drops = [e for e in m if e[0] == DROP]
    assert drops == [(DROP, 0, dest_of[s]) for s in range(nseg) if kinds[s] in ("close", "bad", "both")]
    assert len(drops) == len(marked) and (DROP, 0, dest_of[0]) in drops and (DROP, 0, dest_of[nseg - 1]) in drops
    gone = {d for _, _, d in drops}
    assert not any(d in gone for r in rows for d in r)      # their subscribes of this turn went with them


# ---- destination counts, OVER on the first and the last ----------------------------------------------

@pytest.mark.parametrize("ndest", [1, 1024, 1025])
def test_destination_counts_with_over_on_both_ends(eng, ndest):
    last = ndest - 1
    mid = ndest // 2
    topics = [[0, last, mid] if ndest > 1 else [0], [mid]]
    dest_of = [mid] if ndest > 1 else [0]
    row = [B([text(b"P0\n" + b"x" * 30), text(b"S1\n")])]
    budgets = [1 << 40] * ndest
    budgets[0] = budgets[last] = 10
    m, rows, _, left = case(eng, row, topics, ndest, dest_of, [], OVER | UNIQUE, budgets, SELF)
    over = sorted({0, last})
    assert [d for d, f in enumerate(left[3]) if f] == over
    assert m == [(JOIN, 1, dest_of[0])] + [(DROP, 0, d) for d in over]
    assert rows == ([[mid], [mid]] if ndest > 1 else [[], []])
    # without the flag the budget's verdict is not read
    m2, rows2, _, _ = case(eng, row, topics, ndest, dest_of, [], UNIQUE, budgets, SELF)
    assert m2 == m[:1] and rows2[0] == topics[0]


# ---- each part empty in turn ---------------------------------------------------------------------------

FULL = [B([text(b"S0\n"), text(b"P1\n" + b"y" * 40)]), B([text(b"U1\n"), CLOSE]), B([PING])]
QUIET = [B([text(b"P1\n" + b"y" * 40)]), B([PING]), b""]


@pytest.mark.parametrize("empty", ["none", "route", "drops", "over", "host", "all"])
def test_each_part_empty(eng, empty):
    topics = [[3, 1], [1, 2, 0]]
    ndest, dest_of = 4, [0, 1, 2]
    host = [] if empty in ("host", "all") else [(JOIN, 0, 1), (DROP, 0, 3)]
    row = {"none": FULL, "host": FULL, "over": FULL, "all": QUIET,
           "route": [B([text(b"P1\n" + b"y" * 40)]), B([CLOSE]), b""],
           "drops": [B([text(b"S0\n"), text(b"P1\n" + b"y" * 40)]), B([text(b"U1\n")]), b""]}[empty]
    budgets = [1 << 40, 1 << 40, 0 if empty not in ("over", "all") else 1 << 40, 1 << 40]
    m, rows, _, left = case(eng, row, topics, ndest, dest_of, host, OVER, budgets)
    got = N.parts(left[0], left[1], left[2], dest_of, left[3], host, OVER)
    want_zero = {"none": (), "route": (0,), "drops": (1,), "over": (2,), "host": (3,), "all": (0, 1, 2, 3)}[empty]
    assert [k for k in range(4) if got[k] == 0] == list(want_zero), got
    if empty == "all":
        assert m == [] and rows == topics       # a compacting copy


# ---- failures (hvws_replies_checked) ----------------------------------------------------------------------

def test_a_failed_connection_is_dropped(eng):
    s0 = B([text(b"S1\n"), (0 | Q.FIN | Q.MASK, b"stray", Q.K2), text(b"S0\n")])
    m, rows, _, left = case(eng, [s0, B([text(b"S1\n")])], [[0], [0]], 2, [0, 1], classes=Q.CLASSES)
    assert left[1][0] & libhv_amd.RF_FAILED and m == [(JOIN, 1, 0), (JOIN, 1, 1), (DROP, 0, 0)]
    assert rows == [[], [1]]


def test_join_then_close_in_one_read(eng):
    m, rows, _, _ = case(eng, [B([text(b"S7\n"), CLOSE]), B([text(b"S7\n")])], [[] for _ in range(8)], 6, [4, 5],
                         host=[(JOIN, 3, 4)])
    assert m == [(JOIN, 7, 4), (JOIN, 7, 5), (DROP, 0, 4), (JOIN, 3, 4)]
    assert rows[7] == [5] and rows[3] == [4]


# ---- random turns, determinism --------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_random_small_turns(eng, form):
    rng = random.Random(515)
    parts = [0, 0, 0, 0]
    for _ in range(40):
        row, nt, dest_of, ndest = T.random_turn(rng)
        pool = sorted(set(dest_of))
        topics = [[rng.choice(pool) if rng.random() < 0.7 else rng.randrange(ndest) for _ in range(rng.choice((0, 1, 2, 5)))]
                  for _ in range(nt)]
        host = U.random_events(rng, nt, ndest, pool, rng.choice((0, 1, 3, 8)))
        flags = rng.choice((0, UNIQUE, OVER, UNIQUE | OVER))
        budgets = [rng.choice((0, 20, 1 << 40)) for _ in range(ndest)] if flags & OVER or rng.random() < 0.3 else None
        fan_flags = rng.choice((0, SELF))
        with Q.replied(eng, row, form) as t, Q.subscriptions(eng, topics) as sub:
            left = passes(eng, sub, nt, ndest, dest_of, budgets, fan_flags)
            m, rows, _ = update(eng, sub, topics, ndest, dest_of, left, host, flags)
        # the sequential server over the same reads
        srv = N.Server(nt, topics, bool(flags & UNIQUE), bool(fan_flags & SELF))
        _, closed = srv.turn([(dest_of[c], N.messages_of_read(row[c])) for c in range(len(row))], host,
                             budgets if flags & OVER else None)
        assert rows == srv.rows()
        if flags & OVER:
            assert closed == [d for d, f in enumerate(left[3]) if f]
        for k, v in enumerate(N.parts(left[0], left[1], left[2], dest_of, left[3], host, flags)):
            parts[k] += v
    assert all(parts), parts


def test_the_same_case_twice_gives_identical_arrays(eng):
    rng = random.Random(78)
    def fine():   # a well-formed command; connection 0 sends whatever comes and soon stops
        verb = rng.choice("SSUP")
        return T.header(verb, rng.randrange(3)) + (b"body" if verb == "P" else b"")

    row = [B([text(fine() if c else T.random_message(rng, 3)) for _ in range(120)] + ([CLOSE] if c == 1 else []))
           for c in range(4)]
    topics = [[rng.randrange(64) for _ in range(90)] for _ in range(3)]
    host = U.random_events(rng, 3, 64, [0, 1, 2, 3], 30)
    budgets = [rng.choice((0, 200, 1 << 40)) for _ in range(64)]
    seen = []
    for _ in range(2):
        m, _, arrays, _ = case(eng, row, topics, 64, [0, 1, 2, 3], host, OVER, budgets)
        seen.append((m, arrays))
    assert seen[0] == seen[1] and len(seen[0][0]) > 100


# ---- errors -------------------------------------------------------------------------------------------------------

def test_every_einval_of_the_contract(eng):
    L = libhv_amd.lib()
    topics = [[0, 1, 2], [2], [1, 3]]
    first, member = W.flatten(topics)
    ndest, dest_of = 4, [0, 1]
    row = [B([text(b"S1\n"), text(b"P0\nabc")]), B([text(b"U2\n"), CLOSE])]
    good = [(JOIN, 0, 3), (LEAVE, 1, 2), (DROP, 99, 1)]
    data, segs, _, _, _ = R.Chain(2).inputs(row)
    with Q.session(eng, 2) as s, Q.subscriptions(eng, topics) as (df, dm, nm), out_table(eng, 3, 8) as o:
        def call(**kw):
            a = dict(topic_first=df, member=dm, nmember=nm, events=good, topic_first_out=o.first, member_out=o.member,
                     member_cap=8, flags=0)
            a.update(kw)
            return eng.subs_update_routed(**a)

        def fails(**kw) -> int:
            with pytest.raises(libhv_amd.HvwsError):
                call(**kw)
            assert none_yet(eng) and o.untouched()
            return eng.last_subs_nmember

        s.turn(row)
        fails()                                         # no hvws_route yet
        assert merged_none(eng)
        left = passes(eng, (df, dm, nm), 3, ndest, dest_of)
        m = N.merged(left[0], left[1], left[2], dest_of, None, good, 0)
        want = U.update(topics, (), m)
        need = len(want[1])
        assert call() == need and not none_yet(eng) and not merged_none(eng)
        assert o.read(need)[1].tolist() == want[1].tolist()
        o.fill()
        # the host's events, checked before anything is launched
        for bad in ((0, 0, 0), (4, 0, 0), (JOIN, 3, 0), (LEAVE, 3, 0), (JOIN, 0, 4), (LEAVE, 0, 4), (DROP, 0, 4)):
            fails(events=good + [bad])
            fails(events=[bad] + good)
            assert merged_none(eng)
        # flags; HVWS_SUBS_OVER without a budget, and with one over other destinations
        fails(flags=4)
        fails(flags=UNIQUE | OVER | 8)
        fails(flags=OVER)
        db = eng.to_device(np.array([1 << 40] * 8, np.uint64))
        try:
            eng.budget(db, 0)
            assert call(flags=OVER) == need
            o.fill()
            eng.fanout(df, dm, 3, nm, 8, [libhv_amd.FAN_NONE] * 2, dest_of)     # a plain fan-out over 8 destinations
            fails(flags=OVER)                              # its budget is gone
            eng.budget(db, 0)
            fails(flags=OVER)                              # ... and the new one is over 8, the route over 4
            assert call() == need
            o.fill()
        finally:
            eng.sync()
            db.free()
        # the tables
        fails(nmember=(1 << 32) - 1)
        n = ctypes.c_uint64(0)
        ev = np.zeros(4, libhv_amd.SUB_EVENT_DTYPE)
        assert L.hvws_subs_update_routed(eng.ctx, df.ptr, dm.ptr, nm, ev.ctypes.data, (1 << 32) - 1, 0, o.first.ptr,
                                         o.member.ptr, 8, ctypes.byref(n)) == -2
        assert L.hvws_subs_update_routed(eng.ctx, df.ptr, dm.ptr, nm, None, 1, 0, o.first.ptr, o.member.ptr, 8,
                                         ctypes.byref(n)) == -2
        assert none_yet(eng) and o.untouched()
        fails(topic_first=None)
        fails(member=None)
        fails(topic_first_out=None)
        fails(member_out=None)
        fails(topic_first_out=df)
        fails(member_out=dm)
        fails(member_out=df)
        fails(topic_first_out=dm)
        fails(member_out=o.first)
        fails(topic_first_out=o.first.ptr + 8)
        fails(member_out=o.member.ptr + 4)
        # member_cap: the need passes, one below fails, still reports the need and keeps the merged array
        assert call(member_cap=need) == need
        o.fill()
        assert fails(member_cap=need - 1) == need
        assert triples(eng.subs_events()) == m
        # tables that are not dense, a member id outside the destinations: found on the device
        for bad_first, bad_member in (([1, 3, 4, 6], member), ([0, 4, 3, 6], member), ([0, 3, 4, 5], member),
                                      (first, [0, 1, 2, 2, 1, 4])):
            bf, bm = eng.to_device(np.array(bad_first, np.uint64)), eng.to_device(np.array(bad_member, np.uint32))
            try:
                fails(topic_first=bf, member=bm)
            finally:
                eng.sync()
                bf.free()
                bm.free()
        # what ends the route's tables ends this call: a refused second route, a reply call, a scan
        assert call() == need
        o.fill()
        with pytest.raises(libhv_amd.HvwsError):
            eng.route(3, ndest, [0, 4])
        fails()
        eng.route(3, ndest, dest_of)                       # a second route that stands: its events are merged
        assert call() == need
        o.fill()
        eng.replies(Q.POLICY)
        fails()
        eng.route(3, ndest, dest_of)
        assert call() == need
        o.fill()
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        try:
            eng.scan(rx, len(data), segs)
            fails()
            # the plain call needs none of it, and ends the merged getters
            assert eng.subs_update(df, dm, 3, nm, ndest, good, None, o.first, o.member, 8) == len(U.update(topics, (), good)[1])
            assert merged_none(eng)
        finally:
            eng.sync()
            rx.free()
    with libhv_amd.Engine(0) as fresh:
        assert merged_none(fresh)


# ---- three-turn sessions against the sequential server ---------------------------------------------------------------

def deliveries(eng, t, ndest, budget: bool):
    """{destination: [(opcode, body)]} of the turn's fan-out (budget: of what the budget kept)."""
    if budget:
        table, _ = eng.budget_table()
        first, count, _, _ = eng.dest_budget(ndest)
    else:
        table, _ = eng.fanout_table()
        first, count = eng.dest_fanout(ndest)
    rows = Q.rows_of(table)
    out = {}
    for d in range(ndest):
        mine = rows[int(first[d]):int(first[d]) + int(count[d])]
        if mine:
            out[d] = [(fl & 0xF, bytes(t.out[o:o + ln])) for o, ln, fl, _ in mine]
    return out


@pytest.mark.parametrize("form", ["rfc", "joined"])
@pytest.mark.parametrize("budget", [False, True])
def test_three_turns_alternating_two_tables(eng, form, budget):
    """Turn 0: connections 0 and 1 subscribe to room 1, 1 also publishes there: to
    nobody yet.  Turn 1: connection 2 publishes and both receive; 0 unsubscribes
    (budget: sends nothing and is put over instead), 1 sends a malformed message.
    Turn 2: the publication reaches nobody."""
    nt, ndest, dest_of = 2, 4, [0, 1, 2]
    news = b"P1\n" + b"n" * 60
    turns = [[B([text(b"S1\n")]), B([text(b"S1\n"), text(b"P1\nearly")]), b""],
             [b"" if budget else B([text(b"U1\n")]), B([text(b"junk")]), B([text(news)])],
             [b"", b"", B([text(b"P1\nlate")])]]
    limits = [None, [0 if d == 0 else 1 << 40 for d in range(ndest)], None] if budget else [None] * 3
    srv = N.Server(nt)
    free = N.Server(nt)     # the same server without write limits
    tabs = [(eng.alloc(8 * (nt + 1) + 64), eng.alloc(4 * 16 + 64)) for _ in range(2)]
    try:
        tabs[0][0].upload(np.zeros(nt + 1, np.uint64))
        nm, got_boxes = 0, []
        with Q.session(eng, 3, form) as s:
            for k, row in enumerate(turns):
                (df, dm), (of, om) = tabs[k % 2], tabs[(k + 1) % 2]
                t = s.turn(row)
                eng.route(nt, ndest, dest_of)
                eng.fanout_routed(df, dm, nm)
                db = None
                if budget:
                    lim = limits[k] if limits[k] is not None else [1 << 40] * ndest
                    db = eng.to_device(np.array(lim, np.uint64))
                    eng.budget(db, 0)
                try:
                    box = deliveries(eng, t, ndest, budget)
                    nm = eng.subs_update_routed(df, dm, nm, [], of, om, 16, OVER if budget else 0)
                finally:
                    eng.sync()
                    if db is not None:
                        db.free()
                conns = [(dest_of[c], N.messages_of_read(row[c])) for c in range(3)]
                want_box, closed = srv.turn(conns, (), limits[k])
                free.turn(conns)
                assert box == want_box, k
                want_first, want_member = W.flatten(srv.rows())
                assert nm == len(want_member)
                assert of.download(8 * (nt + 1), np.uint64).tolist() == want_first.tolist()
                assert om.download(4 * nm, np.uint32).tolist() == want_member.tolist() if nm else True
                got_boxes.append(box)
                if k == 1:
                    assert closed == ([0] if budget else [])
        assert got_boxes[0] == {} and got_boxes[2] == {}
        assert got_boxes[1] == ({1: [(1, b"n" * 60)]} if budget else {0: [(1, b"n" * 60)], 1: [(1, b"n" * 60)]})
        assert srv.rows() == [[], []]
        if budget:
            assert free.rows() == [[], [0]]     # only the limit took connection 0 out
    finally:
        eng.sync()
        for a, b in tabs:
            a.free()
            b.free()
