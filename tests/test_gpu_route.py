"""GPU: hvws_route and hvws_fanout_routed (include/hvws.h) against the contract
restated in tests/wsroute.py, field for field: the routed rows, topic and kind
per reply, the event table and its count words, flags and bad_reply per
segment, the totals, the delivery table, reply[], first / count per destination
and *out_deliveries.  The reply table comes from a real turn -- scan, a message
call, hvws_replies or hvws_replies_checked -- and is itself compared with the
oracles of tests/wssend.py, tests/wsrfc.py and tests/wscheck.py.

Shapes are the smallest that can still go wrong: reply counts around the
64-lane wave, the 256-thread block and the scan's 1024-element tile, with
events on those edges; every header length 3 .. 12; every message start
alignment mod 16; a short last message ending at the output's end."""
from __future__ import annotations

import contextlib
import ctypes
import random

import numpy as np
import pytest

import libhv_amd
import wsbudget as G
import wscheck as K
import wsfan as W
import wsharness as H
import wsjoin as J
import wsmsg as M
import wsrfc as R
import wsroute as T
import wssend as S
import wssubs as U

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
K2 = bytes([9, 8, 7, 6])
POLICY = S.R_SERVER | S.R_ECHO
NONE, SELF = libhv_amd.FAN_NONE, libhv_amd.FAN_SELF
CAP = 1 << 16
CLASSES = libhv_amd.C_HEADER | libhv_amd.C_SEQUENCE | libhv_amd.C_CLOSE_BODY | libhv_amd.C_CLOSE_UTF8
NT = (1 << 32) - 1
B = H.build_frames_ref
PING = (9 | FIN | MASK, b"ping", K2)
CLOSE = (8 | FIN | MASK, b"\x03\xe8", K2)


def text(body: bytes, op: int = 1):
    return (op | FIN | MASK, body, KEY)


def rows_of(a) -> list:
    return [tuple(int(x) for x in r) for r in a.tolist()]


class Replied:
    def __init__(self, out, pieces, rep, flags, dev_out, cap):
        self.out, self.pieces = out, pieces
        self.rep, self.answered = rep[0], rep[1]
        self.sender = W.senders(pieces, rep[1])
        self.flags, self.dev_out, self.cap = flags, dev_out, cap


class Session:
    """`n` connections over turns of one message form: scan, the message call,
    the reply call; every turn's device reply table is the oracle's.  fill: the
    byte the output buffers hold before the message call writes them; exact: the
    message call gets out_cap = the bytes it writes."""

    def __init__(self, eng, n: int, form: str = "rfc", cap: int = CAP, fill: int = 0, exact: bool = False):
        self.eng, self.n, self.form, self.cap, self.exact = eng, n, form, cap, exact
        self.ch = J.Chain(n) if form == "joined" else R.Chain(n)
        self.outs = [eng.alloc(cap + 64), eng.alloc(cap + 64)]
        for b in self.outs:
            assert libhv_amd.lib().hvws_memset(eng.ctx, b.ptr, fill, cap + 64) == 0
        self.k, self.prev_len, self.rx = 0, 0, None

    def turn(self, row, classes: int = 0, state_in=None) -> Replied:
        eng, n, ch = self.eng, self.n, self.ch
        cur, old = self.outs[self.k % 2], self.outs[(self.k + 1) % 2]
        if self.rx is not None:
            eng.sync()
            self.rx.free()
        if self.form == "rfc":
            data, segs, _, carries, st = ch.inputs(row)
            res = ch.oracle(row)
            cap = len(res[0]) if self.exact else self.cap
            self.rx = rx = eng.to_device(np.frombuffer(data, np.uint8))
            eng.scan(rx, len(data), segs, carries)
            eng.messages_rfc(rx, len(data), True, cur, cap, st, old if self.k else None, self.prev_len)
            if classes:
                assert self.k == 0
                want = K.Checked(n, classes).oracle(row)
                eng.check(classes, 0, None)
                eng.replies_checked(POLICY)
                rep = K.replies_checked_of(res[1], n, POLICY, want.verdict[1])
            else:
                eng.replies(POLICY)
                rep = R.replies_of(res[1], n, POLICY)
            ch.take(res, row)
        elif self.form == "joined":
            data, segs = ch.inputs(row)
            res = ch.oracle(row)
            cap = len(res[0]) if self.exact else self.cap
            self.rx = rx = eng.to_device(np.frombuffer(data, np.uint8))
            eng.scan(rx, len(data), segs, ch.carry)
            eng.messages_joined(rx, len(data), True, cur, cap, ch.state, old if self.k else None, self.prev_len, ch.off)
            eng.replies(POLICY)
            rep = S.replies_of_pieces(res[1], n, POLICY)
            ch.take(res)
        else:   # plain: one turn, state_in as given
            data, segs, _, _, _ = R.Chain(n).inputs(row)
            res = M.oracle_batch(data, segs, None, state_in)
            cap = len(res[0]) if self.exact else self.cap
            self.rx = rx = eng.to_device(np.frombuffer(data, np.uint8))
            eng.scan(rx, len(data), segs)
            eng.messages(rx, len(data), True, cur, cap, state_in)
            eng.replies(POLICY)
            rep = S.replies_of_pieces(res[1], n, POLICY)
        assert eng.message_table().tolist() == res[1].tolist()
        got, piece = eng.reply_table()
        assert rows_of(got) == rep[0] and piece.tolist() == rep[1]
        assert eng.reply_flags(n).tolist() == rep[3]
        self.k += 1
        self.prev_len = len(res[0])
        return Replied(res[0], res[1], rep, rep[3], cur, cap)

    def free(self):
        self.eng.sync()
        for b in self.outs + ([self.rx] if self.rx is not None else []):
            b.free()


@contextlib.contextmanager
def session(eng, n, form="rfc", **kw):
    s = Session(eng, n, form, **kw)
    try:
        yield s
    finally:
        s.free()


@contextlib.contextmanager
def replied(eng, row, form="rfc", classes=0, state_in=None, **kw):
    with session(eng, len(row), form, **kw) as s:
        yield s.turn(row, classes, state_in)


@contextlib.contextmanager
def subscriptions(eng, topics):
    first, member = W.flatten(topics)
    df, dm = eng.to_device(first), eng.to_device(member if len(member) else np.zeros(1, np.uint32))
    try:
        yield df, dm, len(member)
    finally:
        eng.sync()
        df.free()
        dm.free()


def word(eng, addr) -> int:
    assert addr
    v = np.zeros(1, np.uint64)
    assert libhv_amd.lib().hvws_d2h(eng.ctx, v.ctypes.data, addr, 8) == 0
    eng.sync()
    return int(v[0])


def route(eng, t: Replied, ntopics: int, ndest: int, dest_of):
    """hvws_route on the device against the model, field for field; returns the model's result."""
    L = libhv_amd.lib()
    want = T.route(t.rep, t.sender, t.out, ntopics, dest_of)
    eng.route(ntopics, ndest, dest_of)
    rows, topic, kind = eng.route_table()
    assert kind.tolist() == want[2]
    assert topic.tolist() == want[1]
    assert rows_of(rows) == want[0]
    ev = eng.route_events()
    assert [tuple(int(x) for x in e) for e in ev.tolist()] == want[3]
    assert L.hvws_route_event_count(eng.ctx) == len(want[3]) == word(eng, L.hvws_route_event_count_device(eng.ctx))
    flags, bad = eng.route_flags(len(dest_of))
    assert flags.tolist() == want[4] and bad.tolist() == want[5]
    assert eng.route_totals() == want[6]
    assert L.hvws_route_device(eng.ctx) and L.hvws_route_topics_device(eng.ctx) and L.hvws_route_events_device(eng.ctx)
    n = len(want[0])
    if n:   # a sub-range, any output alone, a range beyond the count
        a = n // 2
        one = np.zeros(n - a, np.uint8)
        assert L.hvws_get_route(eng.ctx, None, None, one.ctypes.data, a, n - a) == 0 and one.tolist() == want[2][a:]
        assert L.hvws_get_route(eng.ctx, None, None, None, a, n - a + 1) == -2
    assert L.hvws_get_route_events(eng.ctx, None, 0, len(want[3]) + 1) == -2
    # the reply table is untouched
    got, _ = eng.reply_table()
    assert rows_of(got) == t.rep
    return want


def fan(eng, t: Replied, routed, subs, ndest: int, dest_of, flags: int = 0, sub=None):
    """hvws_fanout_routed on the device against the model; returns the model's result."""
    want = T.fanout_routed(routed[0], routed[1], t.sender, subs, ndest, dest_of, flags)
    with contextlib.ExitStack() as st:
        df, dm, nm = sub if sub is not None else st.enter_context(subscriptions(eng, subs))
        n = eng.fanout_routed(df, dm, nm, flags)
        assert n == len(want[0]) == eng.last_deliveries
        L = libhv_amd.lib()
        assert L.hvws_fanout_count(eng.ctx) == n and word(eng, L.hvws_fanout_count_device(eng.ctx)) == n
        table, reply = eng.fanout_table()
        assert rows_of(table) == want[0]
        assert reply.tolist() == want[1]
        first, count = eng.dest_fanout(ndest)
        assert first.tolist() == want[2] and count.tolist() == want[3]
    return want


def route_none(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 4)()
    return (not L.hvws_route_device(eng.ctx) and not L.hvws_route_topics_device(eng.ctx)
            and not L.hvws_route_events_device(eng.ctx) and not L.hvws_route_event_count_device(eng.ctx)
            and L.hvws_get_route(eng.ctx, None, None, None, 0, 0) == -2 and L.hvws_route_event_count(eng.ctx) == -1
            and L.hvws_get_route_events(eng.ctx, None, 0, 0) == -2 and L.hvws_get_route_flags(eng.ctx, None, None) == -2
            and L.hvws_get_route_totals(eng.ctx, out) == -2)


def fan_none(eng) -> bool:
    L = libhv_amd.lib()
    return (not L.hvws_fanout_device(eng.ctx) and not L.hvws_fanout_count_device(eng.ctx)
            and L.hvws_fanout_count(eng.ctx) == -1 and L.hvws_get_fanout(eng.ctx, None, None, 0, 0) != 0
            and L.hvws_get_dest_fanout(eng.ctx, None, None) != 0)


# ---- reply counts on the wave, block and scan-tile edges -----------------------------------

EDGES = (0, 62, 63, 64, 65, 254, 255, 256, 257, 1022, 1023, 1024)
IDS = (0, 7, 42, 123, 4567, 89012, 345678, 9012345, 67890123, 456789012, 4294967294)   # header lengths 3 .. 12


def message(i: int, n: int) -> bytes:
    """Reply i of n: commands on the edges (so events start and end there) and
    every seventh reply, publications elsewhere; bodies of 0 .. 15 bytes, so the
    message starts take every alignment mod 16."""
    tid = IDS[i % len(IDS)]
    if i in EDGES or i == n - 1 or i % 7 == 3:
        return T.header("S" if i % 2 == 0 else "U", tid)
    return T.header("P", tid) + bytes((i * 31 + k) & 0xFF for k in range(i % 16))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_reply_counts_on_every_edge(eng, n):
    per = [n // 3 + (1 if c < n % 3 else 0) for c in range(3)]
    at, row = 0, []
    for k in per:
        row.append(B([text(message(i, n), 1 + i % 2) for i in range(at, at + k)]) if k else b"")
        at += k
    with replied(eng, row) as t:
        assert len(t.rep) == n
        want = route(eng, t, NT, 40, [5, 39, 0])
        assert want[6][3] == 0 and want[6][1] + want[6][2] == len(want[3]) > 0
        if n >= 65:
            assert {len(T.header("P", i)) for i in IDS} == set(range(3, 13))
            assert {r[0] % 16 for r in t.rep} == set(range(16))
            assert {want[2][0], want[2][n - 1]} <= {T.RK_SUB, T.RK_UNSUB}


# ---- the grammar on the device ---------------------------------------------------------------

def test_every_boundary_case_of_the_oracle_test(eng):
    """One message per connection, so no malformed one stops another."""
    by_nt = {}
    for msg, nt, want in T.BOUNDARY:
        by_nt.setdefault(nt, []).append((msg, want))
    for nt, cases in by_nt.items():
        row = [B([text(msg, 1 + c % 2)]) for c, (msg, _) in enumerate(cases)]
        with replied(eng, row) as t:
            assert len(t.rep) == len(cases)
            want = route(eng, t, nt, len(cases), list(range(len(cases))))
            for c, (msg, (kind, topic, h)) in enumerate(cases):
                assert (want[2][c], want[1][c]) == (kind, topic if kind == T.RK_PUB else NONE), msg
                assert want[0][c][1] == len(msg) - (h if kind == T.RK_PUB else 0)


def test_a_short_last_message_ends_where_the_output_ends(eng):
    """The output holds LFs beyond the message call's bytes and out_cap is exactly
    those bytes: a read past the last message's L < 12 bytes would find the LF
    that "P1" and "S12" lack."""
    for last, kind in ((b"P1", T.RK_BAD), (b"S12", T.RK_BAD), (b"U4\n", T.RK_UNSUB), (b"P", T.RK_BAD)):
        row = [B([text(b"P3\nbody")]), B([text(last)])]
        with replied(eng, row, fill=0x0A, exact=True) as t:
            o, ln, _, _ = t.rep[-1]
            assert o + ln == len(t.out) == t.cap and ln < 12
            want = route(eng, t, 20, 2, [0, 1])
            assert want[2] == [T.RK_PUB, kind]


# ---- headers the message call assembles ---------------------------------------------------------

FRAG = [(1 | MASK, b"P1", KEY), (0 | FIN | MASK, b"2\nbody", KEY)]


@pytest.mark.parametrize("form", ["rfc", "joined", "plain"])
def test_a_header_in_two_fragments(eng, form):
    with replied(eng, [B(FRAG), B([text(b"S3\n")])], form) as t:
        want = route(eng, t, 20, 2, [0, 1])
        assert want[2] == [T.RK_PUB, T.RK_SUB] and want[1][0] == 12
        o, ln, _, _ = want[0][0]
        assert t.out[o:o + ln] == b"body"


def test_a_ping_between_the_fragments_does_not_land_in_the_header(eng):
    frames = [FRAG[0], (9 | FIN | MASK, b"\n\n", K2), FRAG[1]]
    with replied(eng, [B(frames)], "rfc") as t:
        want = route(eng, t, 20, 1, [0])
        assert want[2] == [T.RK_PUB, T.RK_OTHER] and want[1] == [12, NONE]
        assert t.out[want[0][0][0]:][:want[0][0][1]] == b"body"


@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_a_header_cut_between_two_batches(eng, form):
    with session(eng, 2, form) as s:
        t = s.turn([B([text(b"P2\nfirst"), FRAG[0]]), B([PING])])
        assert route(eng, t, 20, 2, [0, 1])[2] == [T.RK_PUB, T.RK_OTHER]
        t = s.turn([B([FRAG[1], text(b"U2\n")]), b""])
        want = route(eng, t, 20, 2, [0, 1])
        assert want[2] == [T.RK_PUB, T.RK_UNSUB] and want[1] == [12, NONE]
        o, ln, _, _ = want[0][0]
        assert t.out[o - 4:o + ln] == b"P12\nbody"   # the carried bytes stand in front of it in this turn's output


def test_the_plain_form_does_not_route_a_deferred_piece(eng):
    row = [B([(0 | FIN | MASK, b"1\nrest", KEY), text(b"P1\nwhole")]), B([text(b"S1\n")])]
    st = M.states([(2, 1, 1), M.FRESH])
    with replied(eng, row, "plain", state_in=st) as t:
        assert t.flags[0] & S.RF_DEFERRED and len(t.rep) == 2
        want = route(eng, t, 20, 2, [0, 1])
        assert want[2] == [T.RK_PUB, T.RK_SUB] and want[6] == (1, 1, 0, 0)


# ---- the rules inherited from the reply pass ------------------------------------------------------

def test_after_replies_checked_a_failed_connection_publishes_nothing_more(eng):
    s0 = B([text(b"P0\nbefore"), (0 | FIN | MASK, b"stray", K2), text(b"P0\nafter")])
    with replied(eng, [s0, B([text(b"P0\nfine")])], classes=CLASSES) as t:
        assert t.flags[0] & libhv_amd.RF_FAILED
        want = route(eng, t, 1, 2, [0, 1])
        assert want[2] == [T.RK_PUB, T.RK_PUB] and not any(want[4])
        got = fan(eng, t, want, [[0, 1]], 2, [0, 1], SELF)
        assert sorted(t.out[o:o + ln] for o, ln, _, _ in got[0]) == [b"before", b"before", b"fine", b"fine"]


def test_a_publication_behind_a_close_is_no_reply(eng):
    with replied(eng, [B([text(b"P0\nheard"), CLOSE, text(b"P0\nunheard")])]) as t:
        want = route(eng, t, 1, 1, [0])
        assert want[2] == [T.RK_PUB, T.RK_OTHER]


def test_bad_then_stopped_beside_a_clean_connection(eng):
    s0 = B([text(b"P1\nok"), PING, text(b"S1\n"), text(b"P1\r\n"), text(b"P1\nlate"), text(b"U1\n", 2), text(b"junk"), CLOSE])
    s1 = B([text(b"P0\nclean"), text(b"S1\n"), PING])
    with replied(eng, [s0, s1]) as t:
        want = route(eng, t, 2, 2, [1, 0])
        kinds = dict(zip(range(len(t.rep)), want[2]))
        mine = [kinds[i] for i in range(len(t.rep)) if t.sender[i] == 0 and t.rep[i][2] & 0xF in (1, 2)]
        assert mine == [T.RK_PUB, T.RK_SUB, T.RK_BAD, T.RK_STOPPED, T.RK_STOPPED, T.RK_STOPPED]
        assert want[4] == [T.RT_BAD, 0] and want[5][1] == T.ROUTE_NONE and want[2][want[5][0]] == T.RK_BAD
        assert want[3] == [(T.JOIN, 1, 1), (T.JOIN, 1, 0)] and want[6] == (2, 2, 0, 4)
        # the failed connection's PONG and CLOSE still go out, to itself
        got = fan(eng, t, want, [[0, 1], [0]], 2, [1, 0], SELF)
        ops = [fl & 0xF for _, _, fl, _ in got[0][got[2][1]:got[2][1] + got[3][1]]]
        assert ops == [10, 1, 8]


# ---- the routed fan-out ---------------------------------------------------------------------------

def test_one_connection_two_topics_self_counts_differ_per_publication(eng):
    """Connection 0 (destination 0) publishes to topics 0 and 1 in one read and is
    listed in topic 0 twice, in topic 1 not at all."""
    row = [B([text(b"P0\nto zero"), text(b"P1\nto one", 2), text(b"P0\n")]), B([text(b"P1\nfrom one")])]
    subs = [[0, 1, 0, 2], [2, 1, 1], []]
    with replied(eng, row) as t:
        r = route(eng, t, 3, 3, [0, 1])
        drop = fan(eng, t, r, subs, 3, [0, 1])
        keep = fan(eng, t, r, subs, 3, [0, 1], SELF)
        assert drop[3] == [0, 2 + 2, 3 + 1] and keep[3] == [4, 2 + 2 + 2, 3 + 1]   # a destination listed twice: twice
        assert [t.out[o:o + ln] for o, ln, _, _ in keep[0][:4]] == [b"to zero", b"to zero", b"", b""]


def test_an_empty_row_and_one_of_5000_beside_rows_of_one(eng):
    rng = random.Random(11)
    huge = [rng.randrange(8, 500) for _ in range(5000)]
    subs = [[], [3], huge, [9]]
    row = [B([text(b"P0\na"), text(b"P2\nbig"), text(b"P1\nb")]), B([text(b"P3\nc"), text(b"P1\nd")])]
    with replied(eng, row) as t:
        r = route(eng, t, 4, 500, [0, 1])
        assert len(fan(eng, t, r, subs, 500, [0, 1])[0]) == 5000 + 3


@pytest.mark.parametrize("ndest", [127, 128])
def test_sort_passes(eng, ndest):
    rng = random.Random(ndest)
    senders = [0, ndest // 2, ndest - 1]
    subs = [[rng.randrange(ndest) for _ in range(12)] + senders, [ndest - 1, 0]]
    row = [B([text(b"P0\na%d" % c), PING, text(b"P1\nb%d" % c, 2)]) for c in senders]
    with replied(eng, row) as t:
        r = route(eng, t, 2, ndest, senders)
        fan(eng, t, r, subs, ndest, senders)


def fails(eng, *a) -> int:
    with pytest.raises(libhv_amd.HvwsError):
        eng.fanout_routed(*a)
    assert fan_none(eng)
    return eng.last_deliveries


def test_the_einval_cases_of_the_routed_fanout(eng):
    row = [B([text(b"P0\na"), text(b"P1\nb")]), B([text(b"P0\nc"), PING])]
    subs = [[0, 1, 2], [2], [1, 7]]            # topic 2 holds a member id outside 3 destinations
    with session(eng, 2) as s, subscriptions(eng, subs) as (df, dm, nm):
        t = s.turn(row)
        with pytest.raises(libhv_amd.HvwsError):
            eng.fanout_routed(df, dm, nm)       # no hvws_route yet
        r = route(eng, t, 3, 3, [0, 1])
        E = len(fan(eng, t, r, subs, 3, [0, 1], 0, (df, dm, nm))[0])
        assert E == 2 + 1 + 2 + 1
        assert eng.fanout_routed(df, dm, nm, 0, E) == E
        assert fails(eng, df, dm, nm, 0, E - 1) == E       # max_deliveries one short: still reported
        fails(eng, df, dm, nm, 2)                          # an unknown flag bit
        fails(eng, None, dm, nm)                           # a NULL table with topics to publish to
        assert eng.fanout_routed(df, dm, nm) == E and not fan_none(eng)
        # the bad member id: unreached above, reached by a publication to topic 2
        t = s.turn([B([text(b"P2\nreach")]), b""])
        route(eng, t, 3, 3, [0, 1])
        fails(eng, df, dm, nm)
    # a topic row outside the member table: first[1] > first[2], reached and not
    with replied(eng, row) as t:
        df, dm = eng.to_device(np.array([0, 2, 1, 3], np.uint64)), eng.to_device(np.array([0, 1, 2], np.uint32))
        try:
            route(eng, t, 3, 3, [0, 1])
            fails(eng, df, dm, 3)
        finally:
            eng.sync()
            df.free()
            dm.free()
    with replied(eng, [B([text(b"P0\na"), text(b"P2\nb")])]) as t:
        df, dm = eng.to_device(np.array([0, 2, 1, 3], np.uint64)), eng.to_device(np.array([0, 1, 2], np.uint32))
        try:
            route(eng, t, 3, 3, [0])
            assert eng.fanout_routed(df, dm, 3, SELF) == 2 + 2
        finally:
            eng.sync()
            df.free()
            dm.free()


def test_the_einval_cases_of_route_and_what_ends_its_tables(eng):
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh:
        with pytest.raises(libhv_amd.HvwsError):
            fresh.route(1, 1, [0])                 # no reply call on the context
        assert route_none(fresh)
    row = [B([text(b"P0\na")])]
    data, segs, _, _, _ = R.Chain(1).inputs(row)
    with replied(eng, row) as t, subscriptions(eng, [[0]]) as (df, dm, nm):
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        try:
            for args in ((1, 1, None), (1, 1, [1]), (1, 0, [0]), (1, 1 << 31, [0])):
                with pytest.raises(libhv_amd.HvwsError):
                    eng.route(*args)
                assert route_none(eng)
            route(eng, t, 1, 1, [0])
            assert not route_none(eng)
            # a plain hvws_fanout after hvws_route gives what it gives without it
            plain = W.fanout(t.rep, t.sender, [[0]], 1, [0], [0], SELF)
            assert eng.fanout(df, dm, 1, nm, 1, [0], [0], SELF) == 1
            table, reply = eng.fanout_table()
            assert rows_of(table) == plain[0] == [t.rep[0]] and not route_none(eng)
            assert eng.fanout_routed(df, dm, nm, SELF) == 1
            assert rows_of(eng.fanout_table()[0]) == [(t.rep[0][0] + 3, 1, t.rep[0][2], t.rep[0][3])]
            eng.replies(POLICY)                    # a reply call: the tables are gone
            assert route_none(eng)
            with pytest.raises(libhv_amd.HvwsError):
                eng.fanout_routed(df, dm, nm, SELF)
            eng.route(1, 1, [0])
            assert not route_none(eng)
            eng.scan(rx, len(data), segs)          # a scan
            assert route_none(eng)
            with pytest.raises(libhv_amd.HvwsError):
                eng.route(1, 1, [0])
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)
            with pytest.raises(libhv_amd.HvwsError):
                eng.route(1, 1, [0])               # a message call and no reply call
            eng.replies(POLICY)
            eng.route(1, 1, [0])
            assert not route_none(eng)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)   # a message call
            assert route_none(eng)
        finally:
            eng.sync()
            rx.free()
    assert L.hvws_route_event_count(None) == -1


# ---- behind it: the budget and the send -------------------------------------------------------------

def test_budget_and_send_behind_the_routed_fanout(eng):
    rng = random.Random(3)
    bodies = [rng.randbytes(n) for n in (0, 125, 126, 700)]
    row = [B([text(b"P%d\n" % (k % 2) + b, 2) for k, b in enumerate(bodies)] + [PING]),
           B([text(b"P1\n" + b"x" * 126), text(b"S0\n"), CLOSE]), b""]
    subs = [[0, 1, 2, 3], [3, 0]]
    ndest, dest_of = 5, [0, 1, 2]
    with replied(eng, row) as t, subscriptions(eng, subs) as sub:
        r = route(eng, t, 2, ndest, dest_of)
        want = fan(eng, t, r, subs, ndest, dest_of, SELF, sub)
        per = W.destination_frames(t.out, want[0], want[2], want[3])   # over the trimmed bodies
        sizes = [len(b) for b in per]
        assert sizes[3] > 700 and sizes[4] == 0
        # a tight budget: destination 3 one byte short of everything it gets
        budgets = [1 << 40, 1 << 40, 1 << 40, sizes[3] - 1, 0]
        db = eng.to_device(np.array(budgets, np.uint64))
        tx = moff = None
        try:
            eng.budget(db, 0)
            wb = G.budget(want, budgets, 0, 0, False)
            kept, kreply = eng.budget_table()
            first2, count2, byte_off, bflags = eng.dest_budget(ndest)
            assert (rows_of(kept), kreply.tolist(), first2.tolist(), count2.tolist(), byte_off.tolist(),
                    bflags.tolist()) == tuple(wb[:6]) and eng.budget_totals() == wb[6]
            assert bflags[3] == libhv_amd.BF_OVER and not any(bflags[:3])
            assert count2.tolist() == want[3][:3] + [want[3][3] - 1, 0]
            keptper = W.destination_frames(t.out, rows_of(kept), first2.tolist(), count2.tolist())
            assert keptper[:3] == per[:3] and per[3].startswith(keptper[3]) and len(keptper[3]) < sizes[3]
            table, d_n, n = eng.budget_device()
            total = eng.budget_totals()[1]
            assert total == sum(len(b) for b in keptper) == int(byte_off[ndest])
            tx, moff = eng.alloc(total + 64), eng.alloc(8 * (n + 2))
            nbytes, _ = eng.send_messages(tx, total, t.dev_out, t.cap, table, n, d_n, 0, False, moff)
            assert nbytes == total
            got = bytes(tx.download(total))
            for d in range(ndest):
                assert got[int(byte_off[d]):int(byte_off[d + 1])] == keptper[d], d
        finally:
            eng.sync()
            for b in (db, tx, moff):
                if b is not None:
                    b.free()


# ---- a two-turn session ----------------------------------------------------------------------------

def test_two_turns_the_events_of_one_are_the_table_of_the_next(eng):
    """Turn 1: connection 2 joins topic 0, connection 1 leaves it.  Turn 2: a
    publication to topic 0 reaches 2 and no longer 1."""
    ndest, dest_of = 4, [0, 1, 2]
    subs = [[0, 1], [3]]
    with session(eng, 3) as s:
        first, member = W.flatten(subs)
        df, dm = eng.to_device(first), eng.to_device(member)
        df2, dm2 = eng.alloc(8 * 3 + 16), eng.alloc(4 * 16)
        try:
            t = s.turn([B([text(b"P0\nturn one")]), B([text(b"U0\n")]), B([text(b"S0\n"), text(b"S1\n")])])
            r = route(eng, t, 2, ndest, dest_of)
            one = fan(eng, t, r, subs, ndest, dest_of, 0, (df, dm, len(member)))
            assert one[3] == [0, 1, 0, 0]
            ev = eng.route_events()
            assert [tuple(int(x) for x in e) for e in ev.tolist()] == [(T.LEAVE, 0, 1), (T.JOIN, 0, 2), (T.JOIN, 1, 2)]
            nf, nmem, _, new = U.update(subs, U.closed_dests(t.flags, dest_of), r[3])
            assert eng.subs_update(df, dm, 2, len(member), ndest, ev, dest_of, df2, dm2, 16) == len(nmem) == 4
            assert new == [[0, 2], [3, 2]]
            t = s.turn([B([text(b"P0\nturn two")]), b"", B([PING])])
            r = route(eng, t, 2, ndest, dest_of)
            two = fan(eng, t, r, new, ndest, dest_of, 0, (df2, dm2, 4))
            assert two[3] == [0, 0, 2, 0] and t.out[two[0][0][0]:][:two[0][0][1]] == b"turn two"
        finally:
            eng.sync()
            for b in (df, dm, df2, dm2):
                b.free()


# ---- random turns, determinism ------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined", "plain"])
def test_random_small_turns(eng, form):
    rng = random.Random(2025)
    seen = set()
    for _ in range(60):
        row, nt, dest_of, ndest = T.random_turn(rng)
        subs = [[rng.randrange(ndest) for _ in range(rng.choice((0, 1, 2, 5)))] for _ in range(nt)]
        with replied(eng, row, form) as t:
            r = route(eng, t, nt, ndest, dest_of)
            seen |= set(r[2])
            fan(eng, t, r, subs, ndest, dest_of, rng.choice((0, SELF)))
    assert seen == {T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED}


def test_the_same_turn_twice_gives_identical_tables(eng):
    rng = random.Random(77)
    row = [B([text(T.random_message(rng, 3)) for _ in range(120)]) for _ in range(4)]
    subs = [[rng.randrange(64) for _ in range(90)] for _ in range(3)]
    seen = []
    for _ in range(2):
        with replied(eng, row) as t, subscriptions(eng, subs) as (df, dm, nm):
            eng.route(3, 64, [0, 1, 2, 3])
            rt = eng.route_table()
            eng.fanout_routed(df, dm, nm)
            seen.append(tuple(a.tobytes() for a in rt + (eng.route_events(),) + eng.route_flags(4) + eng.fanout_table()
                              + eng.dest_fanout(64)))
    assert seen[0] == seen[1]
