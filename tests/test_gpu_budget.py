"""GPU: hvws_budget (include/hvws.h) against the contract restated in
tests/wsbudget.py, field for field: the kept table, reply[], first / count /
byte_off / flags per destination, the totals and the count word.  The delivery
table it cuts comes from a real turn -- scan, a message call, a reply call,
hvws_fanout -- built as tests/test_gpu_fanout.py builds it and compared with
tests/wsfan.py, so the model and the device start from the same rows.

Shapes are the smallest that can still go wrong: delivery counts around the
64-lane wave, the 256-thread block and the scan's 1024-element tile, with the cut
on, before and after each of those edges; one destination holding everything;
many destinations of one delivery around the block and the tile; budgets of 0,
UINT64_MAX, exactly a prefix sum and one byte less; the header-size edges of the
wire size."""
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
import wssend as S

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
K2 = bytes([9, 8, 7, 6])
POLICY = S.R_SERVER | S.R_ECHO
NONE, SELF = libhv_amd.FAN_NONE, libhv_amd.FAN_SELF
OVER, UNL = libhv_amd.BF_OVER, G.UNLIMITED
CAP = 16384
CLASSES = libhv_amd.C_HEADER | libhv_amd.C_SEQUENCE | libhv_amd.C_CLOSE_BODY | libhv_amd.C_CLOSE_UTF8
B = H.build_frames_ref


def text(body: bytes, op: int = 1):
    return (op | FIN | MASK, body, KEY)


def texts(n: int, tag: bytes = b"m"):
    return B([text(tag + str(i).encode()) for i in range(n)])


class Replied:
    """One turn up to its reply call: the oracle's output bytes and pieces, the
    reply table (replies, the piece each answers), the sender of each reply."""

    def __init__(self, out, pieces, rep, flags, dev_out, cap):
        self.out, self.pieces = out, pieces
        self.rep, self.answered = rep[0], rep[1]
        self.sender = W.senders(pieces, rep[1])
        self.flags, self.dev_out, self.cap = flags, dev_out, cap


@contextlib.contextmanager
def replied(eng, row, form: str = "rfc", cap: int = CAP, classes: int = 0, state_in=None, prev: bytes = b""):
    """scan, the message call of `form`, the reply call; the device's reply table
    is the oracle's.  classes != 0: hvws_check and hvws_replies_checked."""
    n = len(row)
    data, segs, _, _, _ = R.Chain(n).inputs(row)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = eng.alloc(cap + 64)
    pv = eng.to_device(np.frombuffer(prev, np.uint8)) if prev else None
    try:
        eng.scan(rx, len(data), segs)
        if form == "rfc":
            res = R.rfc_batch(data, segs)
            eng.messages_rfc(rx, len(data), True, out, cap)
            if classes:
                want = K.Checked(n, classes).oracle(row)
                eng.check(classes, 0, None)
                eng.replies_checked(POLICY)
                rep = K.replies_checked_of(res[1], n, POLICY, want.verdict[1])
            else:
                eng.replies(POLICY)
                rep = R.replies_of(res[1], n, POLICY)
        elif form == "plain":
            res = M.oracle_batch(data, segs, None, state_in)
            eng.messages(rx, len(data), True, out, cap, state_in)
            eng.replies(POLICY)
            rep = S.replies_of_pieces(res[1], n, POLICY)
        else:
            po = np.zeros(n, np.uint64)
            res = J.joined_batch(data, segs, None, state_in, prev, po)
            eng.messages_joined(rx, len(data), True, out, cap, state_in, pv, len(prev), po)
            eng.replies(POLICY)
            rep = S.replies_of_pieces(res[1], n, POLICY)
        got, piece = eng.reply_table()
        assert [tuple(int(x) for x in r) for r in got.tolist()] == rep[0]
        assert piece.tolist() == rep[1]
        yield Replied(res[0], res[1], rep, rep[3], out, cap)
    finally:
        eng.sync()
        rx.free()
        out.free()
        if pv is not None:
            pv.free()


@contextlib.contextmanager
def fanned(eng, t: Replied, topics, ndest: int, pub, dest_of, flags: int = 0):
    """hvws_fanout over the turn; the device's delivery table is the model's.
    Yields the model's (table, reply, first, count)."""
    want = W.fanout(t.rep, t.sender, topics, ndest, pub, dest_of, flags)
    first, member = W.flatten(topics)
    df, dm = eng.to_device(first), eng.to_device(member)
    try:
        assert eng.fanout(df, dm, len(topics), len(member), ndest, pub, dest_of, flags) == len(want[0])
        same_fanout(eng, want)
        yield want
    finally:
        eng.sync()
        df.free()
        dm.free()


def rows(a) -> list:
    return [tuple(int(x) for x in r) for r in a.tolist()]


def same_fanout(eng, fan) -> None:
    """hvws_fanout's own getters give the model's result (before and after the pass)."""
    table, reply = eng.fanout_table()
    assert rows(table) == fan[0] and reply.tolist() == fan[1]
    first, count = eng.dest_fanout(len(fan[2]))
    assert first.tolist() == fan[2] and count.tolist() == fan[3]
    assert libhv_amd.lib().hvws_fanout_device(eng.ctx) and libhv_amd.lib().hvws_fanout_count(eng.ctx) == len(fan[0])


def word(eng, addr) -> int:
    assert addr
    v = np.zeros(1, np.uint64)
    assert libhv_amd.lib().hvws_d2h(eng.ctx, v.ctypes.data, addr, 8) == 0
    eng.sync()
    return int(v[0])


def compare(eng, fan, budgets, budget_all: int = 0x5A5A, fragment: int = 0, masked: bool = False):
    """hvws_budget on the device against the model, field for field; returns the
    model's result.  budgets: a list (uploaded; budget_all must then be ignored)
    or None (budget_all for every destination)."""
    ndest = len(fan[2])
    want = G.budget(fan, budgets, budget_all, fragment, masked)
    db = eng.to_device(np.array(budgets, np.uint64)) if budgets is not None else None
    try:
        eng.budget(db, budget_all, fragment, masked)
        L = libhv_amd.lib()
        table, reply = eng.budget_table()
        assert rows(table) == want[0]
        assert reply.tolist() == want[1]
        first2, count2, off, flags = eng.dest_budget(ndest)
        assert first2.tolist() == want[2]
        assert count2.tolist() == want[3]
        assert off.tolist() == want[4]
        assert flags.tolist() == want[5]
        assert eng.budget_totals() == want[6]
        assert L.hvws_budget_count(eng.ctx) == want[6][0] == word(eng, L.hvws_budget_count_device(eng.ctx))
        dev = eng.budget_device()
        assert dev[0] and dev[1] and dev[2] == len(fan[0])
        # a sub-range, and either output alone
        if want[0]:
            a = len(want[0]) // 2
            one = np.zeros(len(want[0]) - a, dtype=libhv_amd.TX_MSG_DTYPE)
            assert L.hvws_get_budget(eng.ctx, one.ctypes.data, None, a, len(one)) == 0 and rows(one) == want[0][a:]
            assert L.hvws_get_budget(eng.ctx, None, None, a, len(one) + 1) != 0
    finally:
        eng.sync()
        if db is not None:
            db.free()
    return want


def none_yet(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 4)()
    return (not L.hvws_budget_device(eng.ctx) and not L.hvws_budget_count_device(eng.ctx)
            and L.hvws_budget_count(eng.ctx) == -1 and L.hvws_get_budget(eng.ctx, None, None, 0, 0) != 0
            and L.hvws_get_dest_budget(eng.ctx, None, None, None, None) != 0
            and L.hvws_get_budget_totals(eng.ctx, out) != 0)


def keep(c, m: int) -> int:
    """The budget that keeps exactly the first m deliveries of a destination whose prefix sums are c."""
    return c[m - 1] if m else 0


# ---- delivery counts around the wave, the block and the scan's tile ---------------------------

EDGES = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_delivery_counts_and_the_cut_on_every_edge(eng, n):
    """Two senders publish one short and one long message to destinations 1 and
    2: exactly n deliveries of two sizes.  Destination 2's first dropped delivery
    is put at every table index of EDGES inside its range (and at its first and
    behind its last); destination 1 is cut, whole or empty beside it."""
    x, z = n // 5, n // 7
    y = (n - x - z) // 2
    w = n - x - z - y
    topics = [[1] * x + [2] * y, [2] * w + [1] * z]
    row = [B([text(b"abc")]), B([text(b"L" * 200, 2)])]
    with replied(eng, row) as t, fanned(eng, t, topics, 4, [0, 1], [0, 3]) as fan:
        assert len(fan[0]) == n and fan[3] == [0, x + z, y + w, 0]
        c = G.prefix_sums(fan)
        a = fan[2][2]
        cuts = sorted({p for p in EDGES + (a, a + 1, n - 1, n) if a <= p <= n})
        for i, p in enumerate(cuts):
            b1 = (UNL, 0, keep(c[1], (x + z) // 2))[i % 3]
            want = compare(eng, fan, [7, b1, keep(c[2], p - a), 0])
            assert want[3][2] == p - a and bool(want[5][2]) == (p < n)
            assert want[5][0] == want[5][3] == 0
        same_fanout(eng, fan)


# ---- one destination holding everything -----------------------------------------------------

def test_one_destination_holds_all_deliveries_beside_many_empty_ones(eng):
    row = [texts(10, b"x"), texts(10, b"yy")]
    ndest = 500
    with replied(eng, row) as t, fanned(eng, t, [[7] * 250], ndest, [0, 0], [0, 1]) as fan:
        assert fan[3][7] == 5000 == len(fan[0])
        c = G.prefix_sums(fan)[7]
        for m in (2500, 0, 5000, 1, 4999, 1024, 1025):
            b = [3] * ndest
            b[7] = keep(c, m)
            want = compare(eng, fan, b)
            assert want[3][7] == m and want[6] == (m, keep(c, m), 5000 - m, 1 if m < 5000 else 0)
        same_fanout(eng, fan)


# ---- many destinations of one delivery each ---------------------------------------------------

@pytest.mark.parametrize("ndest", [1, 255, 256, 257, 1025])
def test_many_destinations_of_one_delivery(eng, ndest):
    """Destinations without deliveries before, between and behind the others;
    every second receiver one byte short, next to an untouched one."""
    body = b"one message for all"
    if ndest == 1:
        members = [0]
    else:
        members = [d for d in range(2, ndest - 1) if d % 7 != 3] or [1]
    with replied(eng, [B([text(body)])]) as t, fanned(eng, t, [members], ndest, [0], [0], SELF) as fan:
        assert len(fan[0]) == len(members) and max(fan[3]) == 1
        size = G.wire(len(body), 0, False)
        budgets = [0] * ndest
        for j, d in enumerate(members):
            budgets[d] = size - 1 if j % 2 else size
        want = compare(eng, fan, budgets)
        assert [want[5][d] for d in members] == [OVER if j % 2 else 0 for j in range(len(members))]
        assert want[6] == ((len(members) + 1) // 2, size * ((len(members) + 1) // 2), len(members) // 2,
                           len(members) // 2)
        assert all(want[5][d] == 0 for d in range(ndest) if d not in members)
        compare(eng, fan, None, size)            # everybody fits exactly
        compare(eng, fan, None, size - 1)        # nobody does
        compare(eng, fan, [size] * ndest, 0)     # the array given: budget_all is ignored


# ---- the budget values ----------------------------------------------------------------------

def test_budgets_of_zero_unlimited_a_prefix_sum_and_one_byte_less(eng):
    row = [B([text(b"a" * 10), text(b"b" * 130, 2), text(b"")]), B([text(b"c" * 7), (9 | FIN | MASK, b"p", K2)])]
    topics = [[0, 1, 2, 2], [2, 0]]
    with replied(eng, row) as t, fanned(eng, t, topics, 4, [0, 1], [0, 1], SELF) as fan:
        c = G.prefix_sums(fan)
        assert len(c[2]) == 7 and c[3] == []
        for d in range(3):
            for j in range(len(c[d])):
                b = [UNL] * 4
                b[d] = c[d][j]
                want = compare(eng, fan, b)
                assert want[3][d] == j + 1 and bool(want[5][d]) == (j + 1 < len(c[d]))
                b[d] = c[d][j] - 1
                want = compare(eng, fan, b)
                assert want[3][d] == j and want[5][d] == OVER
        none = compare(eng, fan, [0, 0, 0, 0])
        assert none[0] == [] and none[5] == [OVER, OVER, OVER, 0] and none[4] == [0] * 5   # no deliveries: never OVER
        all_ = compare(eng, fan, [UNL] * 4)
        assert all_[0] == fan[0] and all_[2] == fan[2] and all_[5] == [0] * 4
        # d_budget NULL: budget_all for everybody; given: budget_all is ignored
        assert compare(eng, fan, None, UNL, 0, False)[0] == fan[0]
        assert compare(eng, fan, None, 0)[0] == []
        assert compare(eng, fan, None, c[2][2])[3][2] == 3
        assert compare(eng, fan, [c[0][0], UNL, 0, 5], 0)[3] == [1, len(c[1]), 0, 0]
        same_fanout(eng, fan)


# ---- header-size edges through the wire size --------------------------------------------------

@pytest.mark.parametrize("fragment,masked", [(0, False), (0, True), (5, False), (126, False), (126, True)])
def test_header_size_edges(eng, fragment, masked):
    """Lengths 0, 125 / 126 and 65535 / 65536: the 2-, 4- and 10-byte headers, the
    default fragment size, and fragments of 5 and 126 bytes."""
    rng = random.Random(3)
    bodies = [rng.randbytes(n) for n in (125, 126, 0, 65535, 65536, 127)]
    row = [B([text(b, 2) for b in bodies]), B([text(b"x" * 126)])]
    cap = 1 << 18
    with replied(eng, row, cap=cap) as t, fanned(eng, t, [[1, 0], [1]], 2, [0, 1], [0, 1], SELF) as fan:
        c = G.prefix_sums(fan, fragment, masked)
        assert len(c[1]) == 7 and len(c[0]) == 6
        sizes = G.sizes(fan[0], fragment, masked)
        if fragment == 0:
            hdr = 4 if masked else 0
            assert sorted(set(sizes)) == sorted({2 + hdr, 127 + hdr, 130 + hdr, 131 + hdr, 65539 + hdr,
                                                 65539 + hdr + 1 + 2 + hdr})
        for j in range(len(c[1])):
            assert compare(eng, fan, [UNL, c[1][j]], 0, fragment, masked)[3] == [6, j + 1]
            assert compare(eng, fan, [c[0][-1], c[1][j] - 1], 0, fragment, masked)[3] == [6, j]


# ---- the rules inherited from the reply pass ------------------------------------------------------

def test_after_replies_checked_a_close_behind_the_cut_is_not_received(eng):
    s0 = B([(1 | MASK, b"frag", KEY), (9 | FIN | MASK, b"ping", K2), (0 | FIN | MASK, b"ment", KEY),
            (8 | FIN | MASK, b"\x03\xe8bye", K2), text(b"after the close")])
    row = [s0, B([text(b"from 1")]), B([text(b"from 2", 2)])]
    with replied(eng, row, classes=CLASSES) as t, fanned(eng, t, [[0, 1, 2]], 3, [0, 0, 0], [0, 1, 2]) as fan:
        mine = fan[0][fan[2][0]: fan[2][0] + fan[3][0]]
        assert [r[2] & 0xF for r in mine] == [10, 1, 2, 8]
        c = G.prefix_sums(fan)
        want = compare(eng, fan, [c[0][2], UNL, UNL])           # everything but its own CLOSE
        got = want[0][want[2][0]: want[2][0] + want[3][0]]
        assert [r[2] & 0xF for r in got] == [10, 1, 2] and want[5] == [OVER, 0, 0]
        want = compare(eng, fan, [c[0][3], UNL, c[2][0] - 1])   # the CLOSE fits exactly
        assert want[3][0] == 4 and want[5] == [0, 0, OVER]
        # a smaller delivery behind the cut is not kept either: "from 1" (6 bytes) is cut, the CLOSE is shorter
        want = compare(eng, fan, [c[0][0] + 7, UNL, UNL])
        assert want[3][0] == 1


@pytest.mark.parametrize("form", ["plain", "joined"])
def test_after_the_plain_and_joined_message_forms(eng, form):
    row = [B([(0 | FIN | MASK, b" tail", KEY), text(b"whole")]), B([text(b"other"), (9 | FIN | MASK, b"pp", K2)])]
    st = M.states([(5, 1, 1), M.FRESH])
    with replied(eng, row, form=form, state_in=st, prev=b"first" if form == "joined" else b"") as t:
        with fanned(eng, t, [[0, 1]], 2, [0, 0], [0, 1], SELF) as fan:
            c = G.prefix_sums(fan)
            assert len(c[0]) == (3 if form == "joined" else 2)
            for b in ([c[0][0], c[1][1]], [c[0][1] - 1, UNL], [0, c[1][0] - 1], [UNL, UNL]):
                compare(eng, fan, b)


# ---- the send -----------------------------------------------------------------------------------

@pytest.mark.parametrize("fragment,masked", [(0, False), (5, False), (126, False), (0, True), (126, True)])
def test_send_from_the_budget_table(eng, fragment, masked):
    """hvws_send_messages from hvws_budget_device / hvws_budget_count_device with
    n = the fan-out's count and out_cap = the totals' kept bytes exactly: every
    destination's bytes at byte_off[d] .. byte_off[d + 1] are the frames the
    reference builds for the model's kept deliveries."""
    rng = random.Random(4)
    bodies = [rng.randbytes(n) for n in (0, 125, 126, 700)]
    row = [B([text(b, 2) for b in bodies] + [(9 | FIN | MASK, b"ping", K2)]),
           B([text(b"x" * 126), (8 | FIN | MASK, b"\x03\xe8", K2)]), b""]
    topics = [[0, 1, 2, 3], [3, 0]]
    ndest = 5
    with replied(eng, row) as t, fanned(eng, t, topics, ndest, [0, 1, NONE], [0, 1, 2], SELF) as fan:
        c = G.prefix_sums(fan, fragment, masked)
        budgets = [c[0][2], UNL, c[2][1] + 1, 0, 9]
        want = compare(eng, fan, budgets, 0, fragment, masked)
        kept, _, first2, count2, byte_off, flags, totals = want
        assert flags == [OVER, 0, OVER, OVER, 0] and 0 < totals[0] < len(fan[0])
        per = []
        for d in range(ndest):
            msgs = [(fl, t.out[o:o + ln], key) for o, ln, fl, key in kept[first2[d]:first2[d] + count2[d]]]
            per.append(S.expected(msgs, fragment, masked)[0])
        if not masked:
            assert per == W.destination_frames(t.out, kept, first2, count2, fragment)
        assert [len(b) for b in per] == [byte_off[d + 1] - byte_off[d] for d in range(ndest)]
        table, d_n, n = eng.budget_device()
        assert n == len(fan[0])
        total = totals[1]
        tx, moff = eng.alloc(total + 64), eng.alloc(8 * (n + 2))
        try:
            nbytes, nfr = eng.send_messages(tx, total, t.dev_out, t.cap, table, n, d_n, fragment, masked, moff)
            assert nbytes == total
            assert nfr == sum(S.closed_form(r[1], fragment, masked)[0] for r in kept)
            offs = moff.download(8 * (totals[0] + 1), np.uint64).tolist()
            got = bytes(tx.download(total))
            for d in range(ndest):
                assert offs[first2[d]] == byte_off[d] and offs[first2[d] + count2[d]] == byte_off[d + 1]
                assert got[byte_off[d]:byte_off[d + 1]] == per[d], d
            # one byte less does not hold it
            with pytest.raises(libhv_amd.HvwsError):
                eng.send_messages(tx, total - 1, t.dev_out, t.cap, table, n, d_n, fragment, masked, moff)
            assert eng.last_send_len == total
        finally:
            eng.sync()
            tx.free()
            moff.free()


# ---- validity ---------------------------------------------------------------------------------

def test_none_before_any_call_and_after_what_ends_the_tables(eng):
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh:
        assert none_yet(fresh)
        with pytest.raises(libhv_amd.HvwsError):
            fresh.budget(None, 5)                      # no hvws_fanout on the context
        assert none_yet(fresh)
    row = [B([text(b"a"), text(b"bb")])]
    data, segs, _, _, _ = R.Chain(1).inputs(row)
    with replied(eng, row) as t:
        first, member = W.flatten([[0, 0]])
        df, dm = eng.to_device(first), eng.to_device(member)
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        fan = W.fanout(t.rep, t.sender, [[0, 0]], 1, [0], [0], SELF)
        size = G.wire(1, 0, False)

        def fanout():
            assert eng.fanout(df, dm, 1, 2, 1, [0], [0], SELF) == 4

        def refused(*a):
            with pytest.raises(libhv_amd.HvwsError):
                eng.budget(*a)
            assert none_yet(eng)

        try:
            fanout()
            assert none_yet(eng)                       # a fan-out alone is no budget
            compare(eng, fan, None, 2 * size)
            assert not none_yet(eng)
            refused(None, 5, 0, 2)                     # masked is not 0 or 1 ...
            refused(None, 5, 0, -1)
            compare(eng, fan, None, 2 * size)          # ... and a good call follows
            fanout()                                   # a later hvws_fanout
            assert none_yet(eng)
            compare(eng, fan, None, size)
            eng.replies(POLICY)                        # a reply call: the fan-out is gone, and the budget with it
            assert none_yet(eng)
            refused(None, 5)
            fanout()
            compare(eng, fan, None, size)
            eng.scan(rx, len(data), segs)              # a scan
            assert none_yet(eng)
            refused(None, 5)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)     # a message call
            assert none_yet(eng)
            refused(None, 5)
            eng.replies(POLICY)
            refused(None, 5)                           # a reply call and no fan-out
            fanout()
            compare(eng, fan, None, UNL)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)     # a message call since the pass
            assert none_yet(eng)
        finally:
            eng.sync()
            for b in (df, dm, rx):
                b.free()
    assert L.hvws_budget_count(None) == -1


def test_two_calls_over_one_fanout_each_give_their_own_result_and_time(eng):
    row = [texts(30, b"s%d-" % c) for c in range(3)]
    rng = random.Random(5)
    topics = [[rng.randrange(40) for _ in range(50)] for _ in range(2)]
    with replied(eng, row) as t, fanned(eng, t, topics, 40, [0, 1, 0], [0, 1, 2]) as fan:
        b1, b2 = G.random_budgets(rng, fan), G.random_budgets(rng, fan)
        w1 = compare(eng, fan, b1)
        w2 = compare(eng, fan, b2)
        assert w1 != w2
        assert compare(eng, fan, b1) == w1            # and the same budgets the same result
        db = eng.to_device(np.array(b1, np.uint64))
        try:
            eng.budget(db)
            assert eng.last_kernel_ms() > 0.0         # hvws_last_kernel_ms reports the pass
            seen = []
            for _ in range(2):
                eng.budget(db)
                tb, rp = eng.budget_table()
                seen.append((tb.tobytes(), rp.tobytes()) + tuple(a.tobytes() for a in eng.dest_budget(40)))
            assert seen[0] == seen[1]
        finally:
            eng.sync()
            db.free()
        same_fanout(eng, fan)


# ---- random cases -----------------------------------------------------------------------------

def test_200_random_small_cases(eng):
    """tests/wsfan.py's random turns with the budgets of the CPU test, every
    fragment / masked form in turn, on one context."""
    rng = random.Random(2025)
    forms = ((0, False), (5, False), (126, False), (0, True), (5, True), (1, False))
    cut = whole = 0
    for case in range(200):
        row, topics, ndest, pub, dest_of, flags = W.random_case(rng)
        fragment, masked = forms[case % len(forms)]
        with replied(eng, row) as t, fanned(eng, t, topics, ndest, pub, dest_of, flags) as fan:
            want = compare(eng, fan, G.random_budgets(rng, fan, fragment, masked), 1, fragment, masked)
            cut += sum(1 for f in want[5] if f)
            whole += sum(1 for d in range(ndest) if fan[3][d] and not want[5][d])
    assert cut > 100 and whole > 100
