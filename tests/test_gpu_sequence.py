"""GPU: hvws_sequence and hvws_envelope_sequenced (include/hvws.h) against the
contract restated in tests/wssequence.py -- the number per reply, the totals and
the counters field for field, d_env byte for byte.  The counters and d_env hold
a sentinel wherever the model says nothing is written, and the whole of both is
compared afterwards, guard bytes included.  The reply table comes from a real
turn (tests/test_gpu_route.py's Session) and the route pass in front is itself
compared with tests/wsroute.py.

Shapes are the smallest at which each part can go wrong: a reply capacity of
three sort workgroups with two topics alternating through it; topic counts on
both sides of every radix pass count; numbers of 1, 2, 10, 11, 19 and 20 digits
and the wrap to 0 on lines whose lengths cover every residue mod 16, in front
of bodies around the 16-byte chunk and the copy's tile."""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import pytest

import libhv_amd
import test_gpu_retain as N
import test_gpu_route as Q
import wsbudget as G
import wsenvelope as E
import wsfan as W
import wsharness as H
import wsretain as R
import wsroute as T
import wssequence as S

pytestmark = pytest.mark.gpu

B, text, PING, CLOSE = Q.B, Q.text, Q.PING, Q.CLOSE
FIN = Q.FIN
SENDER = libhv_amd.ENV_SENDER
M64 = (1 << 64) - 1
FILL = 0xA5
GUARD = 64
SORT_TILE = 2048            # pairs per sort workgroup
body = N.body


def tile() -> int:
    return int(libhv_amd.lib().hvws_envelope_tile())


class Counters:
    """d_seq on the device beside the model of it, guard bytes behind."""

    def __init__(self, eng, values):
        self.eng = eng
        self.model = np.array(values, np.uint64)
        self.buf = eng.alloc(self.model.nbytes + GUARD)
        assert libhv_amd.lib().hvws_memset(eng.ctx, self.buf.ptr, FILL, self.model.nbytes + GUARD) == 0
        if self.model.nbytes:
            self.buf.upload(self.model)

    def same_as_model(self):
        got = self.buf.download(self.model.nbytes + GUARD)
        want = np.concatenate([self.model.view(np.uint8), np.full(GUARD, FILL, np.uint8)])
        assert np.array_equal(got, want), "counters at %s" % (np.flatnonzero(got != want)[:8] // 8).tolist()

    def free(self):
        self.eng.sync()
        self.buf.free()


@contextlib.contextmanager
def counters(eng, values):
    c = Counters(eng, values)
    try:
        yield c
    finally:
        c.free()


def sequence_none(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 2)()
    return (not L.hvws_sequence_device(eng.ctx) and L.hvws_get_sequence(eng.ctx, None, 0, 0) == -2
            and L.hvws_get_sequence_totals(eng.ctx, out) == -2)


def numbered(eng, t: Q.Replied, routed, c: Counters):
    """hvws_sequence on the device against the model, field for field; returns the numbers."""
    L = libhv_amd.lib()
    topics, kinds = routed[1], routed[2]
    want = S.sequential(c.model, topics, kinds)
    assert want == S.closed_form(c.model, topics, kinds)
    eng.sequence(c.buf)
    assert eng.sequence_table().tolist() == want[0]
    assert eng.sequence_totals() == want[2]
    for tp, v in want[1].items():
        c.model[tp] = v
    c.same_as_model()
    n, cap = len(want[0]), int(L.hvws_reply_capacity(eng.ctx))
    # the device table: one entry per reply slot, 0 behind the reply count
    dev = L.hvws_sequence_device(eng.ctx)
    assert dev
    whole = np.zeros(cap, np.uint64)
    if cap:
        assert L.hvws_d2h(eng.ctx, whole.ctypes.data, dev, 8 * cap) == 0
        eng.sync()
    assert whole.tolist() == want[0] + [0] * (cap - n)
    if n:   # a sub-range, a range beyond the count
        a = n // 2
        part = np.zeros(n - a, np.uint64)
        assert L.hvws_get_sequence(eng.ctx, part.ctypes.data, a, n - a) == 0 and part.tolist() == want[0][a:]
    assert L.hvws_get_sequence(eng.ctx, None, 0, n + 1) == -2 and L.hvws_get_sequence(eng.ctx, None, n, 0) == 0
    # the route's and the reply call's tables are untouched, and so is the message output
    r2, t2, k2 = eng.route_table()
    assert (Q.rows_of(r2), t2.tolist(), k2.tolist()) == tuple(routed[:3])
    assert Q.rows_of(eng.reply_table()[0]) == t.rep
    assert bytes(t.dev_out.download(len(t.out))) == bytes(t.out)
    return want[0]


class Env:
    """d_env on the device, seeded with 0xA5, and the model's result for the turn."""

    def __init__(self, eng, env_cap: int):
        self.eng, self.cap = eng, env_cap
        self.buf = eng.alloc(env_cap + GUARD)
        assert libhv_amd.lib().hvws_memset(eng.ctx, self.buf.ptr, FILL, env_cap + GUARD) == 0
        self.want = None

    def expected(self) -> np.ndarray:
        want = np.full(self.cap + GUARD, FILL, np.uint8)
        for a, b in (self.want[2] if self.want else ()):
            want[a:a + len(b)] = np.frombuffer(b, np.uint8)
        return want

    def same_as_model(self):
        got = self.buf.download(self.cap + GUARD)
        want = self.expected()
        assert np.array_equal(got, want), "d_env bytes at %s" % np.flatnonzero(got != want)[:8].tolist()

    def bytes(self) -> bytes:
        return self.expected()[:self.cap].tobytes()


@contextlib.contextmanager
def enveloped(eng, t: Q.Replied, routed, dest_of, seq, flags: int = 0):
    """hvws_envelope_sequenced on the device against the model, field for field and byte for byte; yields the Env."""
    L = libhv_amd.lib()
    rows, topics, kinds = routed[:3]
    want = S.envelope_sequential(rows, topics, kinds, t.sender, dest_of, t.out, seq, flags)
    assert (want[0], want[3]) == S.envelope_closed_form(rows, topics, kinds, t.sender, dest_of, t.out, seq, flags)
    bound = eng.envelope_sequenced_bound()
    assert bound == S.bound(t.cap, int(L.hvws_reply_capacity(eng.ctx))) >= want[3][3]
    e = Env(eng, bound)
    try:
        e.want = want
        eng.envelope_sequenced(e.buf, e.cap, flags)
        assert Q.rows_of(eng.envelope_table()) == want[0]
        assert eng.envelope_totals() == want[3]
        e.same_as_model()
        assert eng.sequence_table().tolist() == list(seq)          # the envelope ends nothing of the numbering
        assert bytes(t.dev_out.download(len(t.out))) == bytes(t.out)
        yield e
    finally:
        eng.sync()
        e.buf.free()


# ---- ranks across sort workgroups --------------------------------------------------------------------

def test_two_topics_alternate_through_three_sort_workgroups(eng):
    """About 5000 one-byte publications on three connections: a topic's run spans
    the sort's workgroups, the scan's blocks and the number kernel's."""
    row = []
    for c in range(3):
        msgs = []
        for i in range(1700):
            if i % 7 == 6:
                msgs.append(text(T.header("SU"[(i // 7) % 2], i % 2)))
            else:
                msgs.append(text(T.header("P", (i + c) % 2) + bytes([65 + i % 26]), 1 + i % 2))
            if c == 0 and i == 800:
                msgs.append(PING)
            if c == 1 and i == 1000:
                msgs.append(text(b"oops"))                    # the publications behind it are STOPPED: no number
        if c == 2:
            msgs.append(CLOSE)
        row.append(B(msgs))
    seeds = [10 ** 10 - 1000, 5]
    with Q.replied(eng, row) as t, counters(eng, seeds) as c:
        assert int(libhv_amd.lib().hvws_reply_capacity(eng.ctx)) > 2 * SORT_TILE
        r = Q.route(eng, t, 2, 3, [0, 1, 2])
        kinds = r[2]
        assert {T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED} == set(kinds)
        assert kinds.count(T.RK_STOPPED) > 500 and kinds.count(T.RK_PUB) > 3 * SORT_TILE // 2
        seq = numbered(eng, t, r, c)
        pubs = [sum(1 for k, tp in zip(kinds, r[1]) if k == T.RK_PUB and tp == x) for x in (0, 1)]
        assert c.model.tolist() == [seeds[0] + pubs[0], seeds[1] + pubs[1]] and min(pubs) > 1000
        assert len({len(str(q)) for q in seq}) >= 5               # "0", 1 .. 4 digits and 10, 11


# ---- radix pass counts -----------------------------------------------------------------------------------

@pytest.mark.parametrize("ntopics", [1, 255, 256, 300, 70000])
def test_topic_counts_on_both_sides_of_every_radix_pass(eng, ntopics):
    """The pairs' keys go up to ntopics itself (the slots that take no number):
    one sort pass up to 255 topics, two up to 65535, three beyond.  Every counter
    but the published topics' keeps its sentinel bit for bit."""
    ids = sorted({0, ntopics // 2, ntopics - 1})
    row = [B([text(T.header("P", tid) + b"a%d" % k) for k, tid in enumerate(ids)] + [text(T.header("S", ids[-1])), PING]),
           B([text(T.header("P", tid) + b"b") for tid in reversed(ids)] + [text(T.header("P", ntopics) + b"no such topic")]),
           B([text(T.header("P", ids[0]))] * 3)]
    with Q.replied(eng, row) as t, counters(eng, [(1 << 40) + k for k in range(ntopics)]) as c:
        r = Q.route(eng, t, ntopics, 3, [0, 1, 2])
        seq = numbered(eng, t, r, c)
        assert eng.sequence_totals() == (2 * len(ids) + 3, len(ids))
        assert seq[0] == (1 << 40) + 1 and T.RK_BAD in r[2]
        touched = np.flatnonzero(c.model != (1 << 40) + np.arange(ntopics, dtype=np.uint64)).tolist()
        assert touched == ids


# ---- two turns ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_the_second_turn_continues_the_first(eng, form):
    with Q.session(eng, 2, form) as s, counters(eng, [9, 99, 7]) as c:
        t = s.turn([B([text(b"P0\na"), text(b"P1\nb"), text(b"P0\nc")]), B([text(b"P1\nd"), text(b"P2\ne"), text(b"S0\n")])])
        r = Q.route(eng, t, 3, 2, [0, 1])
        assert numbered(eng, t, r, c) == [10, 100, 11, 101, 8, 0]
        t = s.turn([B([text(b"P0\nf"), PING]), B([text(b"P2\ng"), text(b"P0\nh"), text(b"U0\n")])])
        r = Q.route(eng, t, 3, 2, [0, 1])
        assert numbered(eng, t, r, c) == [12, 0, 9, 13, 0]
        assert c.model.tolist() == [13, 101, 9]                    # topic 1 was quiet in turn 2


# ---- digits ---------------------------------------------------------------------------------------------------

NTOPICS_D = 1300000                                                # topics of 1 .. 7 digits: 10 MB of counters
BASES = (2, 20, 200, 2000, 20000, 200000, 1200000)
SEEDS = (8, 10 ** 10 - 2, 10 ** 19 - 2, M64 - 1)                 # -> 9, 10 | 10 and 11 digits | 19 and 20 | 20 and "0"
DEST_D = [7, 2147483646]


def digit_row(flags: int):
    """Connection 0 (sender 7) publishes once to each of 28 topics, connection 1
    (sender 2147483646) once more: the first gets the seed + 1, the second the
    seed + 2.  Body lengths are chosen against the line's length h."""
    tl = tile()
    row, hs, lens = [], set(), set()
    k = 0
    for c in range(2):
        msgs = []
        for base in BASES:
            for j, seed in enumerate(SEEDS):
                tid = base + j
                h = len(S.line(tid, DEST_D[c], (seed + 1 + c) & M64, flags))
                n = (0, 1, 15, 16, 17, tl - h, tl - 1, tl, tl + 1, 2 * tl - 1, 2 * tl, 2 * tl + 1, 16 - h % 16, 48 - h)[k % 14]
                k += 3                                            # 3 and 14 are coprime: every length with many lines
                msgs.append(text(T.header("P", tid) + body(n, k), 1 + k % 2))
                hs.add(h)
                lens.add(n)
        row.append(B(msgs))
    return row, hs, lens


@pytest.mark.parametrize("flags", [0, SENDER])
def test_numbers_of_every_digit_count_on_lines_of_every_residue(eng, flags):
    row, hs, lens = digit_row(flags)
    tl = tile()
    # 10-digit topics would need 32 GB of counters: the longest line here is 42 of HVWS_SEQ_HDR_MAX = 45 bytes
    assert {h % 16 for h in hs} == set(range(16)) and max(hs) == (42 if flags else 31)
    assert lens >= {0, 1, 15, 16, 17, tl - 1, tl, tl + 1, 2 * tl - 1, 2 * tl, 2 * tl + 1}
    seeds = np.full(NTOPICS_D, 1 << 40, np.uint64)
    for base in BASES:
        seeds[base:base + 4] = SEEDS
    with Q.replied(eng, row, cap=1 << 17) as t, counters(eng, seeds) as c:
        r = Q.route(eng, t, NTOPICS_D, (1 << 31) - 1, DEST_D)
        assert r[2] == [T.RK_PUB] * 56
        seq = numbered(eng, t, r, c)
        assert {len(str(q)) for q in seq} == {1, 2, 10, 11, 19, 20} and seq.count(0) == 7 and seq.count(M64) == 7
        with enveloped(eng, t, r, DEST_D, seq, flags) as e:
            got = {len(b) - int(rr[1]) for (_, b), rr in zip(e.want[2], r[0])}
            assert got == hs
            first = S.parse(e.want[2][0][1])
            assert first[:3] == (2, 7 if flags else None, 9)


# ---- the chain behind it ---------------------------------------------------------------------------------------

def wire_messages(data: bytes):
    return [(op, bytes(m)) for op, m in H.run_messages("oracle", data, [len(data)])[0]] if data else []


def test_a_cut_destination_sees_the_hole_and_a_joiner_continues_its_snapshot(eng):
    """Turn 1: four publications to topic 0; destination 3's budget ends behind the
    second, so it receives 41, 42 and then nothing, and the over-limit rule drops
    it.  Connection 2 joins topic 0 and 1 in that turn: its snapshot of topic 0
    carries 44, and its first live delivery in turn 2 carries 45."""
    L = libhv_amd.lib()
    ndest, dest_of, nt, slot = 5, [0, 1, 2], 2, 64
    subs = [[0, 1, 3], [1]]
    with Q.session(eng, 3) as s, counters(eng, [40, 999]) as c, N.stored(eng, nt, slot) as d:
        first, member = W.flatten(subs)
        df, dm = eng.to_device(first), eng.to_device(member)
        df2, dm2 = eng.alloc(8 * (nt + 1) + 16), eng.alloc(4 * 32)
        tx = moff = db = None
        try:
            t = s.turn([B([text(b"P0\nfirst"), text(b"P0\nsecond", 2), PING, text(b"P1\nother")]),
                        B([text(b"P0\nthird"), text(b"P0\n" + body(20, 4))]),
                        B([text(b"S0\n"), text(b"S1\n")])])
            r = Q.route(eng, t, nt, ndest, dest_of)
            rows, topics, kinds, events = r[:4]
            seq = numbered(eng, t, r, c)
            assert [q for q, k, tp in zip(seq, kinds, topics) if k == T.RK_PUB and tp == 0] == [41, 42, 43, 44]
            with enveloped(eng, t, r, dest_of, seq, SENDER) as e:
                env = e.bytes()
                want = T.fanout_routed(e.want[0], topics, t.sender, subs, ndest, dest_of, Q.SELF)
                assert eng.fanout_enveloped(df, dm, len(member), Q.SELF) == len(want[0])
                table, reply = eng.fanout_table()
                assert Q.rows_of(table) == want[0] and reply.tolist() == want[1]
                per = W.destination_frames(env, want[0], want[2], want[3])
                two = sum(len(b) for b in W.destination_frames(env, want[0], want[2], [min(n, 2) for n in want[3]])[3:4])
                budgets = [1 << 40, 1 << 40, 1 << 40, two + 1, 0]      # the third delivery is longer than a byte
                db = eng.to_device(np.array(budgets, np.uint64))
                eng.budget(db, 0)
                wb = G.budget(want, budgets, 0, 0, False)
                kept, kreply = eng.budget_table()
                first2, count2, byte_off, bflags = eng.dest_budget(ndest)
                assert (Q.rows_of(kept), kreply.tolist(), first2.tolist(), count2.tolist(), byte_off.tolist(),
                        bflags.tolist()) == tuple(wb[:6]) and eng.budget_totals() == wb[6]
                assert bflags[3] == libhv_amd.BF_OVER and count2[3] == 2 and want[3][3] == 4
                keptper = W.destination_frames(env, Q.rows_of(kept), first2.tolist(), count2.tolist())
                btable, d_n, bn = eng.budget_device()
                total = eng.budget_totals()[1]
                tx, moff = eng.alloc(total + 64), eng.alloc(8 * (bn + 2))
                nbytes, _ = eng.send_messages(tx, total, e.buf, e.cap, btable, bn, d_n, 0, False, moff)
                assert nbytes == total == sum(len(b) for b in keptper)
                sent = bytes(tx.download(total))
                heard = {}
                for dd in range(ndest):
                    mine = sent[int(byte_off[dd]):int(byte_off[dd + 1])]
                    assert mine == keptper[dd], dd
                    heard[dd] = [S.parse(m) for op, m in wire_messages(mine) if op in (1, 2)]
                # destination 0 published 41 and 42 itself and hears them with HVWS_FAN_SELF: no hole
                assert [(p[0], p[2]) for p in heard[0]] == [(0, 41), (0, 42), (0, 43), (0, 44)]
                assert [(p[0], p[1], p[2]) for p in heard[1]] == [(0, 0, 41), (0, 0, 42), (1, 0, 1000), (0, 1, 43), (0, 1, 44)]
                assert [(p[0], p[2], p[3]) for p in heard[3]] == [(0, 41, b"first"), (0, 42, b"second")]    # 43, 44: the hole
                assert len(wire_messages(per[3])) == 4
                # the joins and the over-limit drop make the next turn's table
                new_n = eng.subs_update_routed(df, dm, len(member), [], df2, dm2, 32, libhv_amd.SUBS_OVER)
                nf = df2.download(8 * (nt + 1)).view(np.uint64).tolist()
                nm = dm2.download(4 * new_n).view(np.uint32).tolist()
                new = [nm[nf[k]:nf[k + 1]] for k in range(nt)]
                assert new == [[0, 1, 2], [1, 2]]
                # the snapshot: line and body kept, the joiner reads the number it holds
                rrows = E.retain_rows(e.want[0], rows, kinds)
                snap = R.sequential(d.model, rrows, topics, kinds, events, t.sender, 3, env)
                eng.retain_enveloped(d.store, slot, d.ret)
                got, topic, sreply = eng.retain_table()
                assert Q.rows_of(got) == snap[0] and topic.tolist() == snap[1] == [0, 1] and sreply.tolist() == snap[2]
                assert eng.retain_totals() == snap[5]
                d.same_as_model()
                stable, sd_n, scap = eng.retain_device()
                sper = W.destination_frames(d.model.store_bytes(), snap[0], snap[3], snap[4])
                stotal = sum(len(b) for b in sper)
                tx2, moff2 = eng.alloc(stotal + 64), eng.alloc(8 * (scap + 2))
                try:
                    nbytes, _ = eng.send_messages(tx2, stotal, d.store, nt * slot, stable, scap, sd_n, 0, False, moff2)
                    assert nbytes == stotal and bytes(tx2.download(stotal)) == sper[2]
                    held = [S.parse(m) for _, m in wire_messages(sper[2])]
                    assert held == [(0, 1, 44, body(20, 4)), (1, 0, 1000, b"other")]
                finally:
                    eng.sync()
                    tx2.free()
                    moff2.free()
                e.same_as_model()                                  # nothing behind the envelope pass wrote d_env
            t = s.turn([b"", B([text(b"P0\nlive")]), B([PING])])
            r = Q.route(eng, t, nt, ndest, dest_of)
            seq = numbered(eng, t, r, c)
            with enveloped(eng, t, r, dest_of, seq, SENDER) as e:
                want = T.fanout_routed(e.want[0], r[1], t.sender, new, ndest, dest_of, Q.SELF)
                assert eng.fanout_enveloped(df2, dm2, new_n, Q.SELF) == len(want[0])
                assert Q.rows_of(eng.fanout_table()[0]) == want[0]
                per = W.destination_frames(e.bytes(), want[0], want[2], want[3])
                live = [S.parse(m) for op, m in wire_messages(per[2]) if op in (1, 2)]
                assert live == [(0, 1, held[0][2] + 1, b"live")]   # the joiner's first live delivery: 45
        finally:
            eng.sync()
            for b in (df, dm, df2, dm2, tx, moff, db):
                if b is not None:
                    b.free()


# ---- refusals and validity ---------------------------------------------------------------------------------------

def test_every_einval_case_leaves_the_counters_and_the_buffer_intact(eng):
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh, counters(fresh, [1, 2]) as c:
        assert L.hvws_sequence(fresh.ctx, c.buf.ptr, 0) == -2              # no route call on the context
        assert sequence_none(fresh) and fresh.envelope_sequenced_bound() == 0
        assert L.hvws_envelope_sequenced(fresh.ctx, c.buf.ptr, 1 << 20, 0) == -2
        c.same_as_model()
    row = [B([text(b"P0\nvalue"), text(b"S0\n"), text(b"P1\nw")])]
    with Q.session(eng, 1) as s, counters(eng, [5, 6]) as c:
        t = s.turn(row)
        assert L.hvws_sequence(eng.ctx, c.buf.ptr, 0) == -2                # a reply call and no route
        e = Env(eng, 1 << 17)
        try:
            r = Q.route(eng, t, 2, 1, [0])
            out = t.dev_out.ptr
            for a in ((c.buf.ptr, 1), (c.buf.ptr, 1 << 31), (None, 0), (c.buf.ptr + 4, 0), (c.buf.ptr + 1, 0),
                      (out, 0), (out + t.cap - 8, 0), (out - 8, 0)):
                assert L.hvws_sequence(eng.ctx, *a) == -2, a
                assert sequence_none(eng), a
            # without a numbering the sequenced envelope is refused; the plain one is not
            bound = eng.envelope_sequenced_bound()
            assert bound == S.bound(t.cap, int(L.hvws_reply_capacity(eng.ctx))) <= e.cap
            assert L.hvws_envelope_sequenced(eng.ctx, e.buf.ptr, e.cap, 0) == -2
            eng.sync()
            c.same_as_model()
            e.same_as_model()
            assert not Q.route_none(eng)                                     # a refused call ends nothing of the route's
            seq = numbered(eng, t, r, c)
            assert seq == [6, 0, 7] and c.model.tolist() == [6, 7]
            # a turn is numbered once: the counters and the table stand
            assert L.hvws_sequence(eng.ctx, c.buf.ptr, 0) == -2
            assert L.hvws_sequence(eng.ctx, c.buf.ptr, 1) == -2
            c.same_as_model()
            assert eng.sequence_table().tolist() == seq and eng.sequence_totals() == (2, 2)
            ebad = [(e.buf.ptr, e.cap, 2), (e.buf.ptr, e.cap, 1 << 31), (None, e.cap, 0), (e.buf.ptr + 8, bound, 0),
                    (e.buf.ptr, bound - 1, 0), (e.buf.ptr, eng.envelope_bound(), 0), (e.buf.ptr, 0, 0),
                    (out, bound, 0), (out + t.cap - 16, bound, 0)]
            for a in ebad:
                assert L.hvws_envelope_sequenced(eng.ctx, *a) == -2, a
                assert not L.hvws_envelope_device(eng.ctx), a
            eng.sync()
            e.same_as_model()
            assert not sequence_none(eng)                                    # a refused envelope ends nothing of the numbering
            # a plain hvws_envelope behind the numbering writes its old bytes
            plain = E.sequential(r[0], r[1], r[2], t.sender, [0], t.out, SENDER)
            eng.envelope(e.buf, eng.envelope_bound(), SENDER)
            assert Q.rows_of(eng.envelope_table()) == plain[0] and eng.envelope_totals() == plain[3]
            e.want = plain
            e.same_as_model()
            assert L.hvws_envelope(eng.ctx, e.buf.ptr, e.cap, 2) == -2       # its other flag bits stay refused
            # env_cap == the bound is enough
            e.want = S.envelope_sequential(r[0], r[1], r[2], t.sender, [0], t.out, seq, 0)
            assert L.hvws_memset(eng.ctx, e.buf.ptr, FILL, e.cap) == 0
            eng.envelope_sequenced(e.buf, bound, 0)
            assert Q.rows_of(eng.envelope_table()) == e.want[0]
            e.same_as_model()
            # a new route re-arms the numbering
            eng.route(2, 1, [0])
            assert sequence_none(eng)
            assert L.hvws_envelope_sequenced(eng.ctx, e.buf.ptr, e.cap, 0) == -2
            assert numbered(eng, t, r, c) == [7, 0, 8]
        finally:
            eng.sync()
            e.buf.free()


def test_what_ends_the_numbering(eng):
    row = [B([text(b"P0\nvalue"), text(b"S0\n")])]
    data, segs, _, _, _ = Q.R.Chain(1).inputs(row)
    with Q.replied(eng, row) as t, counters(eng, [0]) as c, Q.subscriptions(eng, [[0]]) as (df, dm, nm), \
            N.stored(eng, 1, 32) as d:
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        e = Env(eng, 1 << 17)
        k = [0]
        try:
            def again():
                eng.route(1, 1, [0])
                assert sequence_none(eng)                   # a route call
                with pytest.raises(libhv_amd.HvwsError):
                    eng.envelope_sequenced(e.buf, e.cap, 0)
                eng.sequence(c.buf)
                k[0] += 1
                assert eng.sequence_table().tolist() == [k[0], 0] and eng.sequence_totals() == (1, 1)
                eng.envelope_sequenced(e.buf, e.cap, 0)
                line = b"M0 #%d\n" % k[0]
                assert eng.envelope_totals() == (1, 0, len(line) + 5, 16)
                assert bytes(e.buf.download(len(line) + 5)) == line + b"value"

            again()
            again()
            eng.replies(Q.POLICY)                           # a reply call
            assert sequence_none(eng)
            again()
            eng.scan(rx, len(data), segs)                   # a scan
            assert sequence_none(eng) and eng.envelope_sequenced_bound() == 0
            with pytest.raises(libhv_amd.HvwsError):
                eng.sequence(c.buf)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)
            eng.replies(Q.POLICY)
            again()
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)   # a message call
            assert sequence_none(eng)
            eng.replies(Q.POLICY)
            again()
            # the other passes end nothing of the numbering's
            assert eng.fanout_enveloped(df, dm, nm, Q.SELF) == 1
            eng.budget(None)
            eng.retain_enveloped(d.store, 32, d.ret)
            eng.retain(d.store, 32, d.ret)
            assert not sequence_none(eng) and eng.sequence_table().tolist() == [k[0], 0]
            assert eng.last_kernel_ms() >= 0
            eng.sync()
            assert c.buf.download(8).view(np.uint64)[0] == k[0] == 5
        finally:
            eng.sync()
            rx.free()
            e.buf.free()


def test_an_empty_turn_and_a_route_without_topics(eng):
    L = libhv_amd.lib()
    pong = (10 | FIN | Q.MASK, b"unasked", Q.K2)                   # answered by nothing
    with Q.replied(eng, [B([pong]), B([pong, pong])]) as t, counters(eng, [3, 4]) as c:
        r = Q.route(eng, t, 2, 2, [0, 1])
        assert numbered(eng, t, r, c) == [] and eng.sequence_totals() == (0, 0)
        with enveloped(eng, t, r, [0, 1], [], SENDER) as e:
            assert e.want[3] == (0, 0, 0, 0)
    with Q.replied(eng, [B([text(b"P0\nnowhere"), PING])]) as t, counters(eng, []) as c:
        r = Q.route(eng, t, 0, 1, [0])
        assert T.RK_PUB not in r[2]
        assert L.hvws_sequence(eng.ctx, None, 0) == 0            # ntopics == 0: d_seq may be NULL
        assert eng.sequence_table().tolist() == [0] * len(r[2]) and eng.sequence_totals() == (0, 0)
        c.same_as_model()
        with enveloped(eng, t, r, [0], [0] * len(r[2]), 0) as e:
            assert e.want[3][:2] == (0, 1)


# ---- form and determinism ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_the_same_turn_twice_on_fresh_contexts_gives_identical_tables_and_bytes(form):
    import random
    rng = random.Random(83)
    tl = tile()

    def message():      # well-formed, so that no connection is stopped
        verb = rng.choice("PPPSU")
        return T.header(verb, rng.randrange(7)) + (rng.randbytes(rng.randint(0, 40)) if verb == "P" else b"")

    row = [B([text(message()) for _ in range(300)] + [text(b"P2\n" + rng.randbytes(tl + c)), PING]) for c in range(4)]
    seeds = [0, 9, 99, 10 ** 10 - 100, 10 ** 19 - 100, M64 - 100, 12345]
    seen = []
    for _ in range(2):
        with libhv_amd.Engine(0) as eng, Q.replied(eng, row, form, cap=1 << 17) as t, counters(eng, seeds) as c:
            r = Q.route(eng, t, 7, 64, [0, 1, 2, 3])
            seq = numbered(eng, t, r, c)
            with enveloped(eng, t, r, [0, 1, 2, 3], seq, SENDER) as e:
                seen.append((eng.sequence_table().tobytes(), eng.sequence_totals(), c.buf.download().tobytes(),
                             eng.envelope_table().tobytes(), eng.envelope_totals(), e.buf.download().tobytes()))
    assert seen[0] == seen[1] and seen[0][1][0] > 600 and seen[0][1][1] == 7
