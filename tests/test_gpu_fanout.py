"""GPU: hvws_fanout (include/hvws.h) against the contract restated in
tests/wsfan.py, field for field: the delivery table, reply[], first / count per
destination, the counts and *out_deliveries.  The reply table it expands comes
from a real turn -- scan, a message call, hvws_replies or hvws_replies_checked
-- and is itself compared with the oracles of tests/wssend.py, tests/wsrfc.py
and tests/wscheck.py, so the model and the device start from the same rows.

Shapes are the smallest that can still go wrong: edge counts around the
256-thread block, the 64-lane wave and the sort's 2048-pair tile; destination
counts at which the number of 8-bit sort passes changes (the largest key is
2 * ndest: 127 | 128 and 32767 | 32768) and the ones either side of them."""
from __future__ import annotations

import contextlib
import random

import numpy as np
import pytest

import libhv_amd
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
CAP = 16384
# hvws_check's classes that need no hvws_utf8 pass
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
        assert eng.message_table().tolist() == res[1].tolist()
        got, piece = eng.reply_table()
        assert [tuple(int(x) for x in r) for r in got.tolist()] == rep[0]
        assert piece.tolist() == rep[1]
        assert eng.reply_flags(n).tolist() == rep[3]
        yield Replied(res[0], res[1], rep, rep[3], out, cap)
    finally:
        eng.sync()
        rx.free()
        out.free()
        if pv is not None:
            pv.free()


@contextlib.contextmanager
def subscriptions(eng, topics):
    first, member = W.flatten(topics)
    df, dm = eng.to_device(first), eng.to_device(member)
    try:
        yield df, dm, len(topics), len(member)
    finally:
        eng.sync()
        df.free()
        dm.free()


def count_word(eng) -> int:
    """The device word hvws_send_messages takes as its d_n."""
    L = libhv_amd.lib()
    addr = L.hvws_fanout_count_device(eng.ctx)
    assert addr
    v = np.zeros(1, np.uint64)
    assert L.hvws_d2h(eng.ctx, v.ctypes.data, addr, 8) == 0
    eng.sync()
    return int(v[0])


def compare(eng, t: Replied, topics, ndest: int, pub, dest_of, flags: int = 0, sub=None):
    """hvws_fanout on the device against the model; returns the model's result."""
    want = W.fanout(t.rep, t.sender, topics, ndest, pub, dest_of, flags)
    with contextlib.ExitStack() as st:
        df, dm, nt, nm = sub if sub is not None else st.enter_context(subscriptions(eng, topics))
        n = eng.fanout(df, dm, nt, nm, ndest, pub, dest_of, flags)
        assert n == len(want[0]) == eng.last_deliveries
        assert libhv_amd.lib().hvws_fanout_count(eng.ctx) == n and count_word(eng) == n
        table, reply = eng.fanout_table()
        assert [tuple(int(x) for x in r) for r in table.tolist()] == want[0]
        assert reply.tolist() == want[1]
        first, count = eng.dest_fanout(ndest)
        assert first.tolist() == want[2] and count.tolist() == want[3]
    return want


def none_yet(eng) -> bool:
    L = libhv_amd.lib()
    return (not L.hvws_fanout_device(eng.ctx) and not L.hvws_fanout_count_device(eng.ctx)
            and L.hvws_fanout_count(eng.ctx) == -1 and L.hvws_get_fanout(eng.ctx, None, None, 0, 0) != 0
            and L.hvws_get_dest_fanout(eng.ctx, None, None) != 0)


# ---- no deliveries -------------------------------------------------------------------

def test_no_deliveries(eng):
    """E = 0: pongs are not answered, so there is no reply at all; then control
    replies only under pub = all NONE and pub = NULL; then publications whose
    every edge is a dropped self edge."""
    with replied(eng, [B([(10 | FIN | MASK, b"pong", KEY)]), b""]) as t:
        assert t.rep == []
        assert compare(eng, t, [[0, 1]], 2, [0, 0], [0, 1])[0] == []
    row = [B([text(b"unheard"), (9 | FIN | MASK, b"p", K2)]), B([(9 | FIN | MASK, b"q", KEY), text(b"x", 2)])]
    with replied(eng, row) as t:
        for pub in ([NONE, NONE], None):
            want = compare(eng, t, [[0, 1, 2]], 3, pub, [2, 0])
            assert [r[2] & 0xF for r in want[0]] == [10, 10] and want[3] == [1, 0, 1]
        want = compare(eng, t, [[2, 2], [0]], 3, [0, 1], [2, 0])
        assert [r[2] & 0xF for r in want[0]] == [10, 10]


# ---- expansion across block and wave edges ------------------------------------------------

@pytest.mark.parametrize("npub,nmem", [(1, 257), (257, 1), (65, 65), (3, 64), (64, 3)])
def test_expansion_shapes(eng, npub, nmem):
    nconn = 3
    per = [npub // nconn + (1 if c < npub % nconn else 0) for c in range(nconn)]
    row = [texts(k, b"c%d-" % c) if k else b"" for c, k in enumerate(per)]
    rng = random.Random(npub * 1000 + nmem)
    ndest = 300
    members = [rng.randrange(3, ndest) for _ in range(nmem)]
    with replied(eng, row) as t:
        want = compare(eng, t, [members], ndest, [0, 0, 0], [0, 1, 2])
        assert len(want[0]) == npub * nmem


def test_one_huge_list_beside_many_empty_ones(eng):
    rng = random.Random(11)
    huge = [rng.randrange(8, 500) for _ in range(5000)]
    topics = [[], [], [], huge, [], [], [9], []]
    row = [texts(2, b"a"), texts(1, b"b"), texts(3, b"c"), texts(2, b"d"), texts(1, b"e")]
    with replied(eng, row) as t:
        want = compare(eng, t, topics, 500, [0, 3, 1, 6, NONE], [0, 1, 2, 3, 4])
        assert len(want[0]) == 5000 + 2


# ---- the number of sort passes ---------------------------------------------------------

@pytest.mark.parametrize("ndest", [1, 127, 128, 129, 32767, 32768, 32769])
@pytest.mark.parametrize("digit", ["top", "bottom"])
def test_sort_passes(eng, ndest, digit):
    """A few dozen edges whose keys differ only in the sort's top digit, or only
    in its bottom digit (destinations a multiple of 2^(8 p - 1) apart for the
    pass p that sorts them)."""
    passes = ((2 * ndest).bit_length() + 7) // 8
    rng = random.Random(ndest)
    if digit == "top" and passes > 1:
        pool = list(range(0, ndest, 1 << (8 * (passes - 1) - 1)))
    else:
        pool = list(range(min(ndest, 128)))
    senders = sorted(rng.sample(pool, min(3, len(pool))))
    # every sender is listed too: without HVWS_FAN_SELF its own edges take the
    # key 2 * ndest, the only one that reaches the top digit when ndest is a power of two
    members = [rng.choice(pool) for _ in range(12)] + senders
    rng.shuffle(members)
    row = [B([text(b"a%d" % c), (9 | FIN | MASK, b"p", K2), text(b"b%d" % c, 2), text(b"c%d" % c)]) for c in senders]
    with replied(eng, row) as t:
        want = compare(eng, t, [members], ndest, [0] * len(row), senders)
        assert len(want[0]) == sum(3 * (len(members) - members.count(c)) + 1 for c in senders)
    if passes > 1 and digit == "top" and len(pool) > 1:
        low = (1 << (8 * (passes - 1))) - 1
        assert len({(2 * d) & low for d in pool}) == 1 and len({(2 * d) >> (8 * (passes - 1)) for d in pool}) > 1


# ---- stability ------------------------------------------------------------------------------

@pytest.mark.parametrize("nedges", [1000, 9000])
def test_many_edges_to_one_destination_keep_reply_order(eng, nedges):
    """Every edge has the same key: the sort must leave them as they came, over
    several waves (1000) and several workgroups of 2048 pairs (9000)."""
    row = [texts(10, b"x"), texts(10, b"y")]
    with replied(eng, row) as t:
        want = compare(eng, t, [[7] * (nedges // 20)], 9, [0, 0], [0, 1])
        assert len(want[0]) == nedges and want[1] == sorted(want[1]) and want[3][7] == nedges


def test_two_destinations_interleaved(eng):
    row = [texts(9, b"x"), texts(8, b"y"), texts(7, b"z")]
    with replied(eng, row) as t:
        want = compare(eng, t, [[5, 4] * 100], 6, [0, 0, 0], [0, 1, 2])
        half = 24 * 100
        assert want[3] == [0, 0, 0, 0, half, half]
        assert want[1][:half] == sorted(want[1][:half]) and want[1][half:] == sorted(want[1][half:])


def test_a_destination_listed_twice_is_delivered_twice(eng):
    with replied(eng, [B([text(b"one"), text(b"two")]), b""]) as t:
        want = compare(eng, t, [[1, 2, 1]], 3, [0, NONE], [0, 1])
        assert want[1] == [0, 0, 1, 1, 0, 1] and want[3] == [0, 4, 2]


# ---- self edges -----------------------------------------------------------------------------

def test_self_edges(eng):
    """Connection 0 subscribes to its own topic (twice), connection 1 does not
    subscribe to the one it publishes to."""
    row = [B([text(b"from 0")]), B([text(b"from 1", 2)]), b""]
    topics = [[0, 1, 0, 2], [0, 2]]
    with replied(eng, row) as t:
        drop = compare(eng, t, topics, 3, [0, 1, NONE], [0, 1, 2])
        keep = compare(eng, t, topics, 3, [0, 1, NONE], [0, 1, 2], SELF)
        assert drop[3] == [1, 1, 2] and keep[3] == [3, 1, 2]


# ---- the rules inherited from the reply pass ------------------------------------------------

def test_ping_between_fragments_publish_then_close(eng):
    """After hvws_check and hvws_replies_checked with nothing to fail.  Sender 0 PINGs between the fragments of a text, publishes, then CLOSEs:
    its PONG and CLOSE go to itself alone, the CLOSE last -- behind the
    deliveries it receives from the later senders -- and what it sends after the
    CLOSE reaches nobody."""
    s0 = B([(1 | MASK, b"frag", KEY), (9 | FIN | MASK, b"ping", K2), (0 | FIN | MASK, b"ment", KEY),
            (8 | FIN | MASK, b"\x03\xe8bye", K2), text(b"after the close")])
    row = [s0, B([text(b"from 1")]), B([text(b"from 2", 2)])]
    with replied(eng, row, classes=CLASSES) as t:
        assert not any(f & libhv_amd.RF_FAILED for f in t.flags)
        want = compare(eng, t, [[0, 1, 2]], 3, [0, 0, 0], [0, 1, 2])
        mine = want[0][want[2][0]: want[2][0] + want[3][0]]
        got = [(fl, t.out[o:o + ln]) for o, ln, fl, _ in mine]
        assert got == [(10 | FIN, b"ping"), (1 | FIN, b"from 1"), (2 | FIN, b"from 2"), (8 | FIN, b"\x03\xe8bye")]
        other = want[0][want[2][1]: want[2][1] + want[3][1]]
        assert [(fl, t.out[o:o + ln]) for o, ln, fl, _ in other] == [(1 | FIN, b"fragment"), (2 | FIN, b"from 2")]
        assert all(b"after the close" != t.out[o:o + ln] for o, ln, _, _ in want[0])


def test_a_failed_senders_later_messages_reach_nobody(eng):
    """hvws_check fails connection 0 at a CONTINUE with no message open: the text
    before it is delivered, the texts at and after it are not."""
    s0 = B([text(b"before"), (0 | FIN | MASK, b"stray", K2), text(b"after")])
    row = [s0, B([text(b"fine")])]
    with replied(eng, row, classes=CLASSES) as t:
        assert t.flags[0] & libhv_amd.RF_FAILED and not t.flags[1] & libhv_amd.RF_FAILED
        want = compare(eng, t, [[0, 1]], 2, [0, 0], [0, 1], SELF)
        sent = sorted(t.out[o:o + ln] for o, ln, _, _ in want[0])
        assert sent == [b"before", b"before", b"fine", b"fine"]


def test_a_deferred_piece_produces_nothing(eng):
    """Connection 0's first frame completes a message begun in an earlier batch.
    After hvws_messages its bytes are not all there: no reply, no delivery.
    After hvws_messages_joined the message is whole and is delivered."""
    row = [B([(0 | FIN | MASK, b" tail", KEY), text(b"whole")]), B([text(b"other")])]
    st = M.states([(5, 1, 1), M.FRESH])
    with replied(eng, row, form="plain", state_in=st) as t:
        assert t.flags[0] & S.RF_DEFERRED
        want = compare(eng, t, [[0, 1]], 2, [0, 0], [0, 1], SELF)
        assert sorted(t.out[o:o + ln] for o, ln, _, _ in want[0]) == [b"other", b"other", b"whole", b"whole"]
    with replied(eng, row, form="joined", state_in=st, prev=b"first") as t:
        assert not t.flags[0] & S.RF_DEFERRED
        want = compare(eng, t, [[0, 1]], 2, [0, 0], [0, 1], SELF)
        assert sorted(t.out[o:o + ln] for o, ln, _, _ in want[0]) == [b"first tail", b"first tail", b"other", b"other",
                                                                     b"whole", b"whole"]


# ---- errors ---------------------------------------------------------------------------------

def fails(eng, *a, **kw) -> int:
    with pytest.raises(libhv_amd.HvwsError):
        eng.fanout(*a, **kw)
    assert none_yet(eng)
    return eng.last_deliveries


def test_every_einval_of_the_contract(eng):
    row = [B([text(b"a"), text(b"b")]), B([text(b"c"), (9 | FIN | MASK, b"p", K2)])]
    topics = [[0, 1, 2], [2], [1, 7]]          # topic 2 holds a member id outside 3 destinations
    first, member = W.flatten(topics)
    with replied(eng, row) as t, subscriptions(eng, topics) as (df, dm, nt, nm):
        def ok(pub=(0, 1), **kw):
            return eng.fanout(df, dm, nt, nm, 3, list(pub), [0, 1], **kw)

        E = ok()
        assert E == len(W.fanout(t.rep, t.sender, topics, 3, [0, 1], [0, 1])[0]) == 2 + 2 + 1 + 1
        # max_deliveries: E passes, E - 1 fails and still reports E
        assert ok(max_deliveries=E) == E
        assert fails(eng, df, dm, nt, nm, 3, [0, 1], [0, 1], 0, E - 1) == E
        assert ok() == E and not none_yet(eng)
        # arguments
        fails(eng, df, dm, nt, nm, 3, [0, 1], [0, 1], 2)                       # an unknown flag bit
        fails(eng, df, dm, nt, nm, 3, [0, 1], None)                            # dest_of NULL
        fails(eng, df, dm, nt, nm, 3, [0, 1], [0, 3])                          # dest_of[s] >= ndest
        fails(eng, df, dm, nt, nm, 3, [0, 3], [0, 1])                          # pub[s] >= ntopics, not NONE
        fails(eng, df, dm, nt, nm, 0, [0, 1], [0, 0])                          # ndest 0
        fails(eng, df, dm, nt, nm, 1 << 31, [0, 1], [0, 1])                    # ndest above 2^31 - 1
        # a bad member id fails only when a publication reaches it
        assert ok(pub=[0, NONE]) == 2 + 2 + 1
        fails(eng, df, dm, nt, nm, 3, [0, 2], [0, 1])
        assert ok(pub=[NONE, NONE]) == 1
    # bad topic rows: first[1] > first[2], and a last row that leaves the member table
    for bad_first, reach, miss in (([0, 2, 1, 3], [1, NONE], [0, 2]), ([0, 1, 2, 9], [2, NONE], [0, 1])):
        with replied(eng, row) as t:
            df, dm = eng.to_device(np.array(bad_first, np.uint64)), eng.to_device(np.array([0, 1, 2], np.uint32))
            try:
                fails(eng, df, dm, 3, 3, 3, reach, [0, 1])
                assert eng.fanout(df, dm, 3, 3, 3, [miss[0], NONE], [0, 1]) >= 1
                assert eng.fanout(df, dm, 3, 3, 3, [NONE, miss[1]], [0, 1]) >= 1
            finally:
                eng.sync()
                df.free()
                dm.free()


def test_the_reply_call_must_be_the_last_pass(eng):
    """No reply call on the context; a scan since the reply call; a message call
    since it; a reply call since the fanout ends the tables' validity."""
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh, subscriptions(fresh, [[0]]) as (df, dm, nt, nm):
        fails(fresh, df, dm, nt, nm, 1, [0], [0])
    row = [B([text(b"a")])]
    data, segs, _, _, _ = R.Chain(1).inputs(row)
    with replied(eng, row) as t, subscriptions(eng, [[0]]) as (df, dm, nt, nm):
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        try:
            assert eng.fanout(df, dm, nt, nm, 1, [0], [0], SELF) == 1 and not none_yet(eng)
            eng.replies(POLICY)                     # a reply call: the tables are gone ...
            assert none_yet(eng)
            assert eng.fanout(df, dm, nt, nm, 1, [0], [0], SELF) == 1   # ... and a new fanout may follow it
            eng.scan(rx, len(data), segs)           # a scan since the reply call
            fails(eng, df, dm, nt, nm, 1, [0], [0], SELF)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)     # a message call and no reply call
            fails(eng, df, dm, nt, nm, 1, [0], [0], SELF)
            eng.replies(POLICY)
            assert eng.fanout(df, dm, nt, nm, 1, [0], [0], SELF) == 1
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)     # a message call since the fanout
            assert none_yet(eng)
        finally:
            eng.sync()
            rx.free()
    assert L.hvws_fanout_count(None) == -1


# ---- end to end ---------------------------------------------------------------------------

def test_send_from_the_fanout_table(eng):
    """hvws_send_messages from hvws_fanout_device / hvws_fanout_count_device: each
    destination's byte range is the concatenation of the frames the reference
    builds for the model's deliveries.  Lengths 0, 125, 126 and 65536 (the last
    fragments at the default 65535)."""
    rng = random.Random(3)
    bodies = [rng.randbytes(n) for n in (0, 125, 126, 65536)]
    row = [B([text(b, 2) for b in bodies] + [(9 | FIN | MASK, b"ping", K2)]),
           B([text(b"x" * 126), (8 | FIN | MASK, b"\x03\xe8", K2)]), b""]
    cap = 1 << 17
    topics = [[0, 1, 2, 3], [3, 0]]
    ndest = 5
    with replied(eng, row, cap=cap) as t, subscriptions(eng, topics) as sub:
        want = compare(eng, t, topics, ndest, [0, 1, NONE], [0, 1, 2], SELF, sub)
        table, d_n, n = eng.fanout_device()
        assert n == len(want[0])
        per = W.destination_frames(t.out, want[0], want[2], want[3])
        total = sum(len(b) for b in per)
        tx, moff = eng.alloc(total + 64), eng.alloc(8 * (n + 2))
        try:
            nbytes, nfr = eng.send_messages(tx, total, t.dev_out, cap, table, n, d_n, 0, False, moff)
            assert nbytes == total and nfr == n + 4            # four deliveries of 65536 bytes: two frames each
            offs = moff.download(8 * (n + 1), np.uint64).tolist()
            got = bytes(tx.download(total))
            for d in range(ndest):
                a, b = offs[want[2][d]], offs[want[2][d] + want[3][d]]
                assert got[a:b] == per[d], d
            assert per[4] == b"" and per[2] and per[1].endswith(B([(8 | FIN, b"\x03\xe8", None)]))
        finally:
            eng.sync()
            tx.free()
            moff.free()


# ---- random cases, determinism ---------------------------------------------------------------

def test_200_random_small_cases(eng):
    """<= 8 senders, <= 6 topics, <= 40 destinations, every opcode, on one context."""
    rng = random.Random(2024)
    for case in range(200):
        row, topics, ndest, pub, dest_of, flags = W.random_case(rng)
        with replied(eng, row) as t:
            compare(eng, t, topics, ndest, pub, dest_of, flags)


def test_the_same_batch_twice_gives_identical_tables(eng):
    rng = random.Random(77)
    row = [texts(40, b"s%d-" % c) for c in range(4)]
    topics = [[rng.randrange(64) for _ in range(90)] for _ in range(3)]
    seen = []
    for _ in range(2):
        with replied(eng, row) as t, subscriptions(eng, topics) as (df, dm, nt, nm):
            eng.fanout(df, dm, nt, nm, 64, [0, 1, 2, 0], [0, 1, 2, 3])
            table, reply = eng.fanout_table()
            first, count = eng.dest_fanout(64)
            seen.append((table.tobytes(), reply.tobytes(), first.tobytes(), count.tobytes()))
    assert seen[0] == seen[1] and len(seen[0][1]) == 8 * (40 * 90 * 4 - sum(
        40 * topics[p].count(c) for c, p in enumerate([0, 1, 2, 0])))
