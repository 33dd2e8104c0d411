"""GPU: hvws_envelope, hvws_fanout_enveloped and hvws_retain_enveloped
(include/hvws.h) against the contract restated in tests/wsenvelope.py -- the
enveloped rows and the totals field for field, d_env byte for byte.  d_env
holds a sentinel before every call and the whole of it is compared afterwards
(64 guard bytes behind env_cap included): every pad byte between replies and
every byte from the spanned size on is shown unchanged.  The reply table comes
from a real turn (tests/test_gpu_route.py's Session) and the route pass in
front is itself compared with tests/wsroute.py.

Shapes are the smallest at which the copy can go wrong: every source phase
mod 16 against every destination phase (envelopes of 3 .. 23 bytes, topic and
sender ids of 1 .. 10 digits); body lengths around the 16-byte chunk and the
copy's tile; one body of three tiles among one-byte bodies; a body ending at
the last byte of an exact-capacity output and a reply starting at its first;
two hundred replies on one connection and one each on two hundred."""
from __future__ import annotations

import contextlib
import ctypes
import random

import numpy as np
import pytest

import libhv_amd
import test_gpu_retain as N
import test_gpu_route as Q
import wsenvelope as E
import wsfan as W
import wsharness as H
import wsretain as R
import wsroute as T

pytestmark = pytest.mark.gpu

B, text, PING, CLOSE = Q.B, Q.text, Q.PING, Q.CLOSE
FIN, MASK, K2 = Q.FIN, Q.MASK, Q.K2
NT = Q.NT
SENDER = libhv_amd.ENV_SENDER
SEED = 0xC3
GUARD = 64
TOPIC_IDS = (0, 42, 123, 4567, 89012, 345678, 9012345, 67890123, 456789012, 4294967294)      # 1 .. 10 digits
DEST_IDS = (9, 10, 999, 1000, 99999, 345678, 9012345, 67890123, 456789012, 2147483646)       # 1 .. 10 digits
NDEST_MAX = (1 << 31) - 1
body = N.body


def tile() -> int:
    return int(libhv_amd.lib().hvws_envelope_tile())


class Env:
    """d_env on the device, seeded with the sentinel, and the model's result for the turn."""

    def __init__(self, eng, env_cap: int):
        self.eng, self.cap = eng, env_cap
        self.buf = eng.alloc(env_cap + GUARD)
        self.seed()
        self.want = None

    def seed(self):
        assert libhv_amd.lib().hvws_memset(self.eng.ctx, self.buf.ptr, SEED, self.cap + GUARD) == 0

    def expected(self) -> np.ndarray:
        want = np.full(self.cap + GUARD, SEED, np.uint8)
        for a, b in (self.want[2] if self.want else ()):
            want[a:a + len(b)] = np.frombuffer(b, np.uint8)
        return want

    def same_as_model(self):
        got = self.buf.download(self.cap + GUARD)
        want = self.expected()
        assert np.array_equal(got, want), "d_env bytes at %s" % np.flatnonzero(got != want)[:8].tolist()

    def bytes(self) -> bytes:
        """The model's d_env[0, env_cap): the sentinel wherever no reply wrote."""
        return self.expected()[:self.cap].tobytes()


def envelope_none(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 4)()
    return (not L.hvws_envelope_device(eng.ctx) and L.hvws_get_envelope(eng.ctx, None, 0, 0) == -2
            and L.hvws_get_envelope_totals(eng.ctx, out) == -2)


@contextlib.contextmanager
def enveloped(eng, t: Q.Replied, routed, dest_of, flags: int = 0, slack: int = 0):
    """hvws_envelope on the device against the model, field for field and byte for byte; yields the Env."""
    L = libhv_amd.lib()
    rows, topics, kinds = routed[:3]
    want = E.sequential(rows, topics, kinds, t.sender, dest_of, t.out, flags)
    assert want == E.closed_form(rows, topics, kinds, t.sender, dest_of, t.out, flags)
    bound = eng.envelope_bound()
    assert bound == E.bound(t.cap, int(L.hvws_reply_capacity(eng.ctx))) >= want[3][3]
    e = Env(eng, bound + slack)
    try:
        e.want = want
        eng.envelope(e.buf, e.cap, flags)
        got = eng.envelope_table()
        assert Q.rows_of(got) == want[0]
        assert eng.envelope_totals() == want[3]
        assert L.hvws_envelope_device(eng.ctx)
        e.same_as_model()
        n = len(want[0])
        if n:   # a sub-range, a range beyond the count
            a = n // 2
            part = np.zeros(n - a, libhv_amd.TX_MSG_DTYPE)
            assert L.hvws_get_envelope(eng.ctx, part.ctypes.data, a, n - a) == 0 and Q.rows_of(part) == want[0][a:]
        assert L.hvws_get_envelope(eng.ctx, None, 0, n + 1) == -2 and L.hvws_get_envelope(eng.ctx, None, n, 0) == 0
        # the route's and the reply call's tables are untouched, and so is the message output
        r2, t2, k2 = eng.route_table()
        assert (Q.rows_of(r2), t2.tolist(), k2.tolist()) == tuple(routed[:3])
        assert Q.rows_of(eng.reply_table()[0]) == t.rep
        assert bytes(t.dev_out.download(len(t.out))) == bytes(t.out)
        yield e
    finally:
        eng.sync()
        e.buf.free()


def turn(eng, row, ntopics, ndest, dest_of, flags=0, form="rfc", **kw):
    """One turn on a fresh session, route and envelope checked; -> (Replied, routed, the model's result)."""
    with Q.replied(eng, row, form, **kw) as t:
        r = Q.route(eng, t, ntopics, ndest, dest_of)
        with enveloped(eng, t, r, dest_of, flags) as e:
            return t, r, e.want


# ---- every source phase against every destination phase ---------------------------------------

@pytest.mark.parametrize("flags", [0, SENDER])
def test_every_source_phase_against_every_destination_phase(eng, flags):
    """Connection c has a destination id of c + 1 digits and publishes, to a topic
    of each digit count, sixteen messages of 33 bytes: every message starts one
    byte further into its 16-byte chunk than the one before."""
    row = []
    for c in range(10):
        msgs = []
        for k, tid in enumerate(TOPIC_IDS):
            hdr = T.header("P", tid)
            msgs += [text(hdr + body(33 - len(hdr), 16 * k + i), 1 + i % 2) for i in range(16)]
        row.append(B(msgs))
    t, r, want = turn(eng, row, NT, NDEST_MAX, list(DEST_IDS), flags, cap=1 << 17)
    rows, topics, kinds = r[:3]
    assert kinds == [T.RK_PUB] * 1600
    seen = {(rr[0] % 16, (w[1] - rr[1]) % 16, w[1] - rr[1]) for rr, w in zip(rows, want[0])}
    hs = {h for _, _, h in seen}
    assert hs == (set(range(5, 24)) if flags else set(range(3, 13)))
    for h in hs:
        assert {s for s, _, hh in seen if hh == h} == set(range(16)), h
    if flags:
        assert {(s, d) for s, d, _ in seen} == {(s, d) for s in range(16) for d in range(16)}


# ---- body lengths around the chunk and the tile ---------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined", "plain"])
def test_body_lengths_around_the_chunk_and_the_tile(eng, form):
    tl = tile()
    row = []
    for c, (tid, flags_h) in enumerate(((7, 5), (123456, 11))):      # h' = len(b"M7 0\n"), len(b"M123456 10\n")
        lens = [0, 1, 15, 16, 17, tl - flags_h - 1, tl - flags_h, tl - flags_h + 1, 16 - flags_h, 32 - flags_h]
        row.append(B([text(T.header("P", tid) + body(n, k + c), 1 + k % 2) for k, n in enumerate(lens)]))
    t, r, want = turn(eng, row, 1 << 20, 11, [0, 10], SENDER, form, cap=1 << 16)
    assert [w[1] - rr[1] for rr, w in zip(r[0], want[0])] == [5] * 10 + [11] * 10
    assert {w[1] for w in want[0]} >= {5, tl - 1, tl, tl + 1, 16, 32}


def test_one_body_of_three_tiles_and_five_bytes_among_one_byte_bodies(eng):
    tl = tile()
    msgs = [text(b"P3\nx")] * 5 + [text(b"P4\n" + body(3 * tl + 5, 1), 2)] + [text(b"P3\ny")] * 5
    t, r, want = turn(eng, [B(msgs), B([text(b"P1\nz")] * 3)], 5, 2, [0, 1], 0, cap=1 << 15)
    assert want[3] == (14, 0, 13 * 4 + 3 + 3 * tl + 5, 13 * 16 + E.up16(3 + 3 * tl + 5))


# ---- the output's two ends ------------------------------------------------------------------------

@pytest.mark.parametrize("last", [1, 15, 16, 17, 40])
def test_a_body_that_ends_at_the_last_byte_and_a_reply_that_starts_at_the_first(eng, last):
    """The output buffer holds 0xEE beyond out_cap: a chunk's second aligned load
    may not leave the capacity, and what it would find there is not the body.
    The PONG's bytes begin at offset 0: the outward rounding stops there."""
    ping = (9 | FIN | MASK, body(125, 7), K2)
    row = [B([ping]), B([text(b"P1\n" + body(23, 9))]), B([text(b"P0\n" + body(last, 4))])]
    with Q.replied(eng, row, fill=0xEE, exact=True) as t:
        o, ln, _, _ = t.rep[-1]
        assert o + ln == len(t.out) == t.cap and t.rep[0][:2] == (0, 125)
        r = Q.route(eng, t, 2, 3, [0, 1, 2])
        with enveloped(eng, t, r, [0, 1, 2], SENDER) as e:
            assert e.want[0][0][:2] == (0, 125) and e.want[0][-1][1] == 5 + last


# ---- many replies -----------------------------------------------------------------------------------

def test_two_hundred_replies_on_one_connection_and_one_each_on_two_hundred(eng):
    one = B([text(T.header("P", i % 7) + body(i % 40, i), 1 + i % 2) if i % 9 else text(T.header("S", i % 7))
             for i in range(200)])
    t, r, want = turn(eng, [one], 7, 3, [2], SENDER)
    assert len(want[0]) == 200 and want[3][0] == 200 - 23
    row = [B([text(T.header("P", c % 5) + body((c * 3) % 50, c), 1 + c % 2)]) for c in range(200)]
    t, r, want = turn(eng, row, 5, 1000, [5 * c for c in range(200)], SENDER, cap=1 << 15)
    assert want[3][0] == 200 and {w[1] - rr[1] for rr, w in zip(r[0], want[0])} == {5, 6, 7}


# ---- verbatim replies, malformed messages ---------------------------------------------------------

@pytest.mark.parametrize("flags", [0, SENDER])
def test_a_ping_of_125_bytes_a_close_with_a_reason_and_a_malformed_message(eng, flags):
    ping = (9 | FIN | MASK, body(125, 3), K2)
    close = (8 | FIN | MASK, b"\x03\xe9going away, good night", K2)
    row = [B([text(b"P1\nbefore"), ping, text(b"P0\n"), close]),
           B([text(b"P0\nheard"), text(b"oops"), text(b"P1\nunheard"), PING, text(b"S1\n")]),
           B([text(b"S1\n"), text(b"U0\n"), text(b"P1\n" + body(130, 5), 2)])]
    t, r, want = turn(eng, row, 2, 40, [39, 0, 7], flags)
    # within a connection the data replies come first, then the control replies
    assert r[2] == [T.RK_PUB, T.RK_PUB, T.RK_OTHER, T.RK_OTHER, T.RK_PUB, T.RK_BAD, T.RK_STOPPED, T.RK_STOPPED,
                    T.RK_OTHER, T.RK_SUB, T.RK_UNSUB, T.RK_PUB]
    h, g = (6, 5) if flags else (3, 3)           # b"M1 39\n" and b"M0 0\n" / b"M1 7\n" against b"M1\n"
    assert [w[1] for w in want[0]] == [h + 6, h, 125, 24, g + 5, 0, 0, 0, 4, 0, 0, g + 130]
    assert want[3][:2] == (4, 3)
    assert E.parse(want[2][0][1]) == (1, 39 if flags else None, b"before")


def test_a_turn_with_no_reply_to_copy(eng):
    t, r, want = turn(eng, [B([text(b"S0\n")]), b"", B([text(b"nope")])], 4, 3, [0, 1, 2], SENDER)
    assert want[0] == [(0, 0, 1 | FIN, want[0][0][3]), (0, 0, 1 | FIN, want[0][1][3])] and want[3] == (0, 0, 0, 0)


# ---- random turns, determinism ------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined", "plain"])
def test_random_small_turns(eng, form):
    rng = random.Random(2026)
    seen = set()
    for k in range(40):
        row, nt, dest_of, ndest = T.random_turn(rng)
        t, r, want = turn(eng, row, nt, ndest, dest_of, k & 1, form)
        seen |= set(r[2])
    assert seen == {T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED}


def test_the_same_turn_twice_gives_identical_bytes(eng):
    rng = random.Random(79)
    tl = tile()
    def message():      # well-formed, so that no connection is stopped
        verb = rng.choice("PPPSU")
        return T.header(verb, rng.randrange(7)) + (rng.randbytes(rng.randint(0, 40)) if verb == "P" else b"")

    row = [B([text(message()) for _ in range(300)] + [text(b"P2\n" + rng.randbytes(2 * tl + c)), PING])
           for c in range(4)]
    seen = []
    for _ in range(2):
        with Q.replied(eng, row, cap=1 << 17) as t:
            eng.route(7, 64, [0, 1, 2, 3])
            cap = eng.envelope_bound()
            e = Env(eng, cap)
            try:
                eng.envelope(e.buf, cap, SENDER)
                seen.append((eng.envelope_table().tobytes(), eng.envelope_totals(), e.buf.download().tobytes()))
            finally:
                eng.sync()
                e.buf.free()
    assert seen[0] == seen[1] and seen[0][1][0] > 600 and seen[0][1][1] == 4 and seen[0][1][2] > 8 * tl


# ---- end to end: fan-out, budget and send from d_env -----------------------------------------------------

def wire_messages(data: bytes):
    """The messages a client's parser sees in a destination's byte range."""
    return [(op, bytes(m)) for op, m in H.run_messages("oracle", data, [len(data)])[0]] if data else []


@pytest.mark.parametrize("fan_flags", [0, Q.SELF])
def test_fanout_budget_and_send_from_the_envelope_buffer(eng, fan_flags):
    """Connections subscribed to two topics each; every data message a destination
    gets names its topic and its sender.  The routed fan-out on the same turn
    still delivers the bare bodies, and the subscription update behind either
    fan-out is the same."""
    L = libhv_amd.lib()
    ndest, dest_of, nt = 5, [0, 1, 2], 3
    subs = [[0, 1, 3], [1, 2, 0], [2, 0, 3]]                     # destinations 0, 1, 2 are in two topics each
    row = [B([text(b"P0\nzero says hi"), text(b"P1\n" + body(126, 1), 2), PING]),
           B([text(b"P1\nfrom one"), text(b"S2\n"), text(b"P2\n")]),
           B([text(b"U0\n"), text(b"P0\n" + body(700, 2)), CLOSE])]
    with Q.replied(eng, row) as t, Q.subscriptions(eng, subs) as sub:
        r = Q.route(eng, t, nt, ndest, dest_of)
        rows, topics, kinds = r[:3]
        df, dm, nm = sub
        df2, dm2, df3, dm3 = (eng.alloc(8 * (nt + 1) + 16), eng.alloc(4 * 32), eng.alloc(8 * (nt + 1) + 16),
                              eng.alloc(4 * 32))
        tx = moff = None
        try:
            with enveloped(eng, t, r, dest_of, SENDER) as e:
                rows2 = e.want[0]
                want = T.fanout_routed(rows2, topics, t.sender, subs, ndest, dest_of, fan_flags)
                n = eng.fanout_enveloped(df, dm, nm, fan_flags)
                assert n == len(want[0]) == eng.last_deliveries == L.hvws_fanout_count(eng.ctx)
                table, reply = eng.fanout_table()
                assert Q.rows_of(table) == want[0] and reply.tolist() == want[1]
                first, count = eng.dest_fanout(ndest)
                assert first.tolist() == want[2] and count.tolist() == want[3]
                assert L.hvws_envelope_device(eng.ctx)             # the fan-out ends nothing of the envelope's
                eng.budget(None)
                kept, kreply = eng.budget_table()
                assert Q.rows_of(kept) == want[0] and kreply.tolist() == want[1]
                _, _, byte_off, bflags = eng.dest_budget(ndest)
                env = e.bytes()
                per = W.destination_frames(env, want[0], want[2], want[3])
                total = eng.budget_totals()[1]
                assert total == sum(len(b) for b in per) == int(byte_off[ndest]) and not any(bflags)
                btable, d_n, bn = eng.budget_device()
                tx, moff = eng.alloc(total + 64), eng.alloc(8 * (bn + 2))
                nbytes, _ = eng.send_messages(tx, total, e.buf, e.cap, btable, bn, d_n, 0, False, moff)
                assert nbytes == total
                sent = bytes(tx.download(total))
                # the sequential server's list per destination: (destination, close last, reply, listing) order
                es = sorted(T.edges(rows, topics, t.sender, subs, dest_of, fan_flags))
                heard = 0
                for d in range(ndest):
                    mine = sent[int(byte_off[d]):int(byte_off[d + 1])]
                    assert mine == per[d], d
                    msgs = wire_messages(mine)
                    exp = [i for dd, _, i, _ in es if dd == d]
                    assert len(msgs) == len(exp), d
                    for (op, m), i in zip(msgs, exp):
                        o, ln, fl, _ = rows[i]
                        assert op == fl & 0xF
                        if kinds[i] == T.RK_PUB:
                            assert E.parse(m) == (topics[i], dest_of[t.sender[i]], bytes(t.out[o:o + ln])), (d, i)
                            heard += 1
                        else:
                            assert m == bytes(t.out[o:o + ln])
                assert heard == (15 if fan_flags else 12)
                new_n = eng.subs_update_routed(df, dm, nm, [], df2, dm2, 32)
                new_a = (new_n, df2.download(8 * (nt + 1)).tobytes(), dm2.download(4 * new_n).tobytes())
                # the routed fan-out on the same turn: the bare bodies, from the message output
                bare = Q.fan(eng, t, r, subs, ndest, dest_of, fan_flags, sub)
                assert [w[1] for w in bare[0]] != [w[1] for w in want[0]] and bare[1] == want[1]
                eng.budget(None)
                btable, d_n, bn = eng.budget_device()
                bper = W.destination_frames(t.out, bare[0], bare[2], bare[3])
                btotal = sum(len(b) for b in bper)
                nbytes, _ = eng.send_messages(tx, btotal, t.dev_out, t.cap, btable, bn, d_n, 0, False, moff)
                assert nbytes == btotal < total and bytes(tx.download(btotal)) == b"".join(bper)
                new_n = eng.subs_update_routed(df, dm, nm, [], df3, dm3, 32)
                assert new_a == (new_n, df3.download(8 * (nt + 1)).tobytes(), dm3.download(4 * new_n).tobytes())
                e.same_as_model()                                  # nothing behind the envelope pass wrote d_env
        finally:
            eng.sync()
            for b in (df2, dm2, df3, dm3, tx, moff):
                if b is not None:
                    b.free()


# ---- hvws_retain_enveloped ------------------------------------------------------------------------------

def test_the_enveloped_retain_keeps_envelope_and_body_and_a_joiner_of_three_topics_reads_three(eng):
    L = libhv_amd.lib()
    slot, nt = 32, 6
    ndest, dest_of = 8, [7, 3, 0]
    row = [B([text(b"P0\nvalue zero"), text(b"P1\n"), text(b"P2\n" + body(29, 2)), text(b"P5\n" + body(27, 5))]),
           B([text(b"S0\n"), text(b"S3\n"), text(b"S4\n"), text(b"S1\n"), text(b"S2\n")]),
           B([text(b"P3\nxxxxx", 2), text(b"P4\nfour")])]
    with N.stored(eng, nt, slot) as d, Q.replied(eng, row) as t:
        # topic 1 holds a value from an earlier turn: the empty publication clears it
        ent = d.ret.download(16 * nt).view(libhv_amd.RETAINED_DTYPE).copy()
        ent[1] = (9, 1 | FIN, 1)
        d.ret.upload(ent)
        d.model.ret[1] = (9, 1 | FIN, 1)
        assert d.model.value(1) is not None
        r = Q.route(eng, t, nt, ndest, dest_of)
        rows, topics, kinds, events = r[:4]
        with pytest.raises(libhv_amd.HvwsError):
            eng.retain_enveloped(d.store, slot, d.ret)             # no envelope yet
        assert N.retain_none(eng)
        with enveloped(eng, t, r, dest_of, SENDER) as e:
            rrows = E.retain_rows(e.want[0], rows, kinds)
            want = R.sequential(d.model, rrows, topics, kinds, events, t.sender, 3, e.bytes())
            st, rt = d.store.ptr, d.ret.ptr
            for a in ((st, slot, rt, 1), (e.buf.ptr, slot, rt, 0), (e.buf.ptr + e.cap - 16, slot, rt, 0),
                      (st, slot, e.buf.ptr + 16, 0), (t.dev_out.ptr, slot, rt, 0), (st, 24, rt, 0)):
                assert L.hvws_retain_enveloped(eng.ctx, *a) == -2, a     # a flags bit; the store or its entries over d_env / d_out
                assert N.retain_none(eng), a
            eng.retain_enveloped(d.store, slot, d.ret)
            got, topic, reply = eng.retain_table()
            assert Q.rows_of(got) == want[0] and topic.tolist() == want[1] and reply.tolist() == want[2]
            first, count = eng.segment_retain(3)
            assert first.tolist() == want[3] and count.tolist() == want[4]
            assert eng.retain_totals() == want[5]
            d.same_as_model()
            e.same_as_model()
            # P0: 5 + 10; P1 empty: cleared; P2: 29 <= slot < 5 + 29, oversize by its envelope; P5: 5 + 27 == slot
            assert want[5] == (4, 1, 1, 15 + 32 + 10 + 9, 3) and want[1] == [0, 3, 4]
            assert d.model.value(1) is None and d.model.value(2) is None
            assert d.model.value(5) == (b"M5 7\n" + body(27, 5), 1 | FIN)
            # the snapshot on the wire: three messages for the joiner, each naming its topic and sender
            table, d_n, cap = eng.retain_device()
            per = W.destination_frames(d.model.store_bytes(), want[0], want[3], want[4])
            total = sum(len(b) for b in per)
            tx, moff = eng.alloc(total + 64), eng.alloc(8 * (cap + 2))
            try:
                nbytes, _ = eng.send_messages(tx, total, d.store, nt * slot, table, cap, d_n, 0, False, moff)
                assert nbytes == total
                sent = bytes(tx.download(total))
                assert sent == per[1] and per[0] == per[2] == b""
                assert [E.parse(m) for _, m in wire_messages(sent)] == [(0, 7, b"value zero"), (3, 0, b"xxxxx"),
                                                                       (4, 0, b"four")]
            finally:
                eng.sync()
                tx.free()
                moff.free()
            # hvws_retain on the same turn keeps the bare bodies
            eng.retain(d.store, slot, d.ret)
            assert eng.retain_totals()[:3] == (5, 1, 0)


# ---- errors and validity ---------------------------------------------------------------------------------

def test_every_einval_case_leaves_the_buffer_intact(eng):
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh:
        e = Env(fresh, 4096)
        try:
            assert fresh.envelope_bound() == 0
            assert L.hvws_envelope(fresh.ctx, e.buf.ptr, 4096, 0) == -2      # no route call on the context
            assert envelope_none(fresh)
            assert L.hvws_fanout_enveloped(fresh.ctx, None, None, 0, 0, 1, None) == -2
            assert L.hvws_retain_enveloped(fresh.ctx, e.buf.ptr, 16, e.buf.ptr + 64, 0) == -2
            e.same_as_model()
        finally:
            fresh.sync()
            e.buf.free()
    row = [B([text(b"P0\nvalue"), text(b"S0\n")])]
    with Q.session(eng, 1) as s, Q.subscriptions(eng, [[0], []]) as (df, dm, nm):
        t = s.turn(row)
        assert eng.envelope_bound() == 0                                    # a reply call and no route
        e = Env(eng, 1 << 17)
        try:
            assert L.hvws_envelope(eng.ctx, e.buf.ptr, e.cap, 0) == -2
            r = Q.route(eng, t, 2, 1, [0])
            bound = eng.envelope_bound()
            assert 0 < bound <= e.cap
            out = t.dev_out.ptr
            bad = [(e.buf.ptr, e.cap, 2), (e.buf.ptr, e.cap, 1 << 31), (e.buf.ptr, e.cap, 3),      # a flags bit
                   (None, e.cap, 0), (e.buf.ptr + 8, bound, 0), (e.buf.ptr + 1, bound, 0),           # NULL, misaligned
                   (e.buf.ptr, bound - 1, 0), (e.buf.ptr, 0, 0),                                     # below the bound
                   (out, bound, 0), (out + t.cap - 16, bound, 0), (out - bound + 16, bound, 0)]     # over the message output
            for a in bad:
                assert L.hvws_envelope(eng.ctx, *a) == -2, a
                assert envelope_none(eng), a
                assert L.hvws_fanout_enveloped(eng.ctx, df.ptr, dm.ptr, nm, 0, 1 << 40, None) == -2
            eng.sync()
            e.same_as_model()
            assert bytes(t.dev_out.download(len(t.out))) == bytes(t.out)
            assert not Q.route_none(eng)                                     # a refused call ends nothing of the route's
            eng.envelope(e.buf, bound, 0)                                    # env_cap == the bound is enough
            assert eng.envelope_totals() == (1, 0, 8, 16) and not envelope_none(eng)
            for fl in (2, 1 << 31):
                assert L.hvws_fanout_enveloped(eng.ctx, df.ptr, dm.ptr, nm, fl, 1 << 40, None) == -2
            assert L.hvws_fanout_enveloped(eng.ctx, None, None, 0, 0, 1 << 40, None) == -2   # ntopics != 0: the table must be there
        finally:
            eng.sync()
            e.buf.free()


def test_what_ends_the_envelope_tables(eng):
    row = [B([text(b"P0\nvalue"), text(b"S0\n")])]
    data, segs, _, _, _ = Q.R.Chain(1).inputs(row)
    with Q.replied(eng, row) as t, Q.subscriptions(eng, [[0]]) as (df, dm, nm), N.stored(eng, 1, 16) as d:
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        e = Env(eng, 1 << 17)
        try:
            def again():
                eng.route(1, 1, [0])
                assert envelope_none(eng)                   # a route call
                with pytest.raises(libhv_amd.HvwsError):
                    eng.fanout_enveloped(df, dm, nm)
                with pytest.raises(libhv_amd.HvwsError):
                    eng.retain_enveloped(d.store, 16, d.ret)
                eng.envelope(e.buf, e.cap, SENDER)
                assert not envelope_none(eng) and eng.envelope_totals() == (1, 0, 10, 16)
                assert eng.fanout_enveloped(df, dm, nm, Q.SELF) == 1

            again()
            again()
            eng.replies(Q.POLICY)                           # a reply call
            assert envelope_none(eng)
            again()
            eng.scan(rx, len(data), segs)                   # a scan
            assert envelope_none(eng) and eng.envelope_bound() == 0
            with pytest.raises(libhv_amd.HvwsError):
                eng.envelope(e.buf, e.cap, 0)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)
            eng.replies(Q.POLICY)
            again()
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)   # a message call
            assert envelope_none(eng)
            eng.replies(Q.POLICY)
            again()
            # the other passes end nothing of the envelope's
            eng.budget(None)
            eng.retain(d.store, 16, d.ret)
            eng.retain_enveloped(d.store, 16, d.ret)
            assert not envelope_none(eng) and eng.retain_totals() == (1, 0, 0, 10, 1)
            assert bytes(d.store.download(10)) == b"M0 0\nvalue"
        finally:
            eng.sync()
            rx.free()
            e.buf.free()
