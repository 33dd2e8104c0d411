"""GPU: hvws_retain (include/hvws.h) against the contract restated in
tests/wsretain.py -- the store byte for byte, the d_ret entries, the snapshot
rows with topic and reply, first / count per segment, the totals and the count
words, field for field.  The store and its entries hold a sentinel before every
call, and the whole of both is compared afterwards (64 guard bytes behind each
included): every byte outside [t * slot, t * slot + len) of a stored topic and
every entry of a topic without a publication is shown unchanged.  The reply
table comes from a real turn (tests/test_gpu_route.py's Session) and the route
pass in front is itself compared with tests/wsroute.py.

Shapes are the smallest that can still go wrong: body lengths around the
16-byte chunk and the copy's tile; header lengths 3 .. 12 and every body start
alignment mod 16; len == slot and slot + 1; topic 0 and ntopics - 1; one topic;
reply counts around the 64-lane wave, the 256-thread block and the scan's
1024-element tile with winners and SUB replies on those edges; a body ending at
the last byte of an exact-capacity output.  A header of 10 .. 12 bytes names a
topic of eight to ten digits, so its store has 10^7 .. 10^9 slots: those stores
are not read back whole -- what the turn touched is compared and set back to the
sentinel, and the digest of everything is the one taken before the turn."""
from __future__ import annotations

import contextlib
import ctypes
import random

import numpy as np
import pytest

import libhv_amd
import test_gpu_route as Q
import wsfan as W
import wsretain as R
import wsroute as T

pytestmark = pytest.mark.gpu

B, text, PING, CLOSE = Q.B, Q.text, Q.PING, Q.CLOSE
FIN = Q.FIN
SEED = 0xA5
WORD = SEED * 0x0101010101010101


def tile() -> int:
    return int(libhv_amd.lib().hvws_retain_tile())


def body(n: int, salt: int = 0) -> bytes:
    return bytes((salt * 37 + k * 11 + (k >> 8)) % 251 for k in range(n))


class Dev:
    """A device store and its entries, seeded with a sentinel (which retains
    nothing: set != 1), beside the model of it."""

    def __init__(self, eng, ntopics: int, slot: int):
        self.eng, self.nt, self.slot = eng, ntopics, slot
        self.store, self.ret = eng.alloc(ntopics * slot + 64), eng.alloc(ntopics * 16 + 64)
        L = libhv_amd.lib()
        assert L.hvws_memset(eng.ctx, self.store.ptr, SEED, ntopics * slot + 64) == 0
        assert L.hvws_memset(eng.ctx, self.ret.ptr, SEED, ntopics * 16 + 64) == 0
        self.model = R.Store(ntopics, slot, SEED, (WORD, WORD & 0xFFFFFFFF, WORD & 0xFFFFFFFF))

    def same_as_model(self):
        """The whole store and every entry, guard bytes included."""
        nt, slot, m = self.nt, self.slot, self.model
        want = np.full(nt * slot + 64, SEED, np.uint8)
        for t, w in m.written.items():
            want[t * slot:t * slot + len(w)] = np.frombuffer(w, np.uint8)
        got = self.store.download(nt * slot + 64)
        assert np.array_equal(got, want), "store bytes at %s" % np.flatnonzero(got != want)[:8].tolist()
        del got, want
        want = np.full(2 * (nt + 4), WORD, np.uint64).view(libhv_amd.RETAINED_DTYPE)   # two words per entry
        for t, e in m.ret.items():
            want[t] = e
        got = self.ret.download(16 * (nt + 4)).view(libhv_amd.RETAINED_DTYPE)
        assert np.array_equal(got, want), "entries at %s" % np.flatnonzero(got != want)[:8].tolist()

    def digests(self):
        return (self.eng.digest(self.store, self.nt * self.slot + 64), self.eng.digest(self.ret, self.nt * 16 + 64))

    def same_as_model_by_digest(self, before):
        """For a store too large to read back: every slot and entry the model says a
        turn touched is compared and then set back to the sentinel, and the digests
        of the whole store and of all entries (guard bytes included) are those taken
        `before` the turn.  The store is the seeded one again afterwards."""
        L, ctx, slot = libhv_amd.lib(), self.eng.ctx, self.slot
        fill = np.full(slot, SEED, np.uint8)
        for t in sorted(set(self.model.written) | set(self.model.ret)):
            got, ent = np.zeros(slot, np.uint8), np.zeros(1, libhv_amd.RETAINED_DTYPE)
            assert L.hvws_d2h(ctx, got.ctypes.data, self.store.ptr + t * slot, slot) == 0
            assert L.hvws_d2h(ctx, ent.ctypes.data, self.ret.ptr + t * 16, 16) == 0
            self.eng.sync()
            assert bytes(got) == self.model.slot_bytes(t), t
            assert tuple(int(x) for x in ent[0]) == self.model.entry_of(t), t
            assert L.hvws_h2d(ctx, self.store.ptr + t * slot, fill.ctypes.data, slot) == 0
            assert L.hvws_h2d(ctx, self.ret.ptr + t * 16, fill.ctypes.data, 16) == 0
            self.eng.sync()
        assert self.digests() == before

    def free(self):
        self.eng.sync()
        self.store.free()
        self.ret.free()


@contextlib.contextmanager
def stored(eng, ntopics, slot):
    d = Dev(eng, ntopics, slot)
    try:
        yield d
    finally:
        d.free()


def retain(eng, t: Q.Replied, routed, d: Dev, nseg: int, whole: bool = True):
    """hvws_retain on the device against the model, field for field; returns the
    model's result.  whole = False: the caller compares the store itself."""
    L = libhv_amd.lib()
    rows, topics, kinds, events = routed[:4]
    want = R.sequential(d.model, rows, topics, kinds, events, t.sender, nseg, t.out)
    eng.retain(d.store, d.slot, d.ret)
    got, topic, reply = eng.retain_table()
    assert Q.rows_of(got) == want[0]
    assert topic.tolist() == want[1] and reply.tolist() == want[2]
    first, count = eng.segment_retain(nseg)
    assert first.tolist() == want[3] and count.tolist() == want[4]
    assert eng.retain_totals() == want[5]
    n = len(want[0])
    assert L.hvws_retain_count(eng.ctx) == n == Q.word(eng, L.hvws_retain_count_device(eng.ctx))
    table, d_n, cap = eng.retain_device()
    assert table and d_n and cap == L.hvws_reply_capacity(eng.ctx) >= n
    if whole:
        d.same_as_model()
    # a sub-range, any output alone, a range beyond the count
    if n:
        a = n // 2
        one = np.zeros(n - a, np.uint32)
        assert L.hvws_get_retain(eng.ctx, None, one.ctypes.data, None, a, n - a) == 0 and one.tolist() == want[1][a:]
    assert L.hvws_get_retain(eng.ctx, None, None, None, 0, n + 1) == -2
    assert L.hvws_get_retain(eng.ctx, None, None, None, n, 0) == 0
    # the route's and the reply call's tables are untouched
    r2, t2, k2 = eng.route_table()
    assert (Q.rows_of(r2), t2.tolist(), k2.tolist()) == tuple(routed[:3])
    assert Q.rows_of(eng.reply_table()[0]) == t.rep
    return want


def retain_none(eng) -> bool:
    L = libhv_amd.lib()
    out = (ctypes.c_uint64 * 5)()
    return (not L.hvws_retain_device(eng.ctx) and not L.hvws_retain_count_device(eng.ctx)
            and L.hvws_retain_count(eng.ctx) == -1 and L.hvws_get_retain(eng.ctx, None, None, None, 0, 0) == -2
            and L.hvws_get_segment_retain(eng.ctx, None, None) == -2 and L.hvws_get_retain_totals(eng.ctx, out) == -2)


def turn(eng, row, ntopics, d: Dev, form="rfc", dest_of=None, whole=True, **kw):
    """One turn on a fresh session: route and retain checked; -> (Replied, routed, retained)."""
    dest_of = list(range(len(row))) if dest_of is None else dest_of
    with Q.replied(eng, row, form, **kw) as t:
        r = Q.route(eng, t, ntopics, max(dest_of) + 1, dest_of)
        return t, r, retain(eng, t, r, d, len(row), whole)


# ---- body lengths around the chunk and the tile --------------------------------------------------

@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_body_lengths_around_the_chunk_and_the_tile(eng, form):
    tl = tile()
    lens = [1, 15, 16, 17, tl - 1, tl, tl + 1, 2 * tl + 3]
    slot = (2 * tl + 3 + 15) // 16 * 16
    nt = len(lens) + 2
    # two connections; topic 0 and ntopics - 1 among them; a joiner of each length
    msgs = [text(b"P%d\n" % k + body(n, k), 1 + k % 2) for k, n in enumerate(lens, 1)]
    joins = [text(b"S%d\n" % k) for k in range(nt)]
    row = [B(msgs[:4] + [text(b"P0\nzero")] + joins[:5]), B(msgs[4:] + [PING] + joins[5:])]
    with stored(eng, nt, slot) as d:
        t, r, got = turn(eng, row, nt, d, form, cap=1 << 16)
        assert got[5][:3] == (len(lens) + 1, 0, 0) and got[5][3] == sum(lens) + 4
        assert got[1] == list(range(nt - 1))          # topic ntopics - 1 holds nothing: no row
        assert [ln for _, ln, _, _ in got[0]] == [4] + lens
        for k, n in enumerate(lens, 1):
            assert d.model.value(k) == (body(n, k), (1 + k % 2) | FIN)


def test_len_equal_to_the_slot_and_one_more(eng):
    slot = 48
    row = [B([text(b"P0\n" + body(slot, 1)), text(b"P1\n" + body(slot + 1, 2)), text(b"P2\n" + body(slot - 1, 3)),
              text(b"S0\n"), text(b"S1\n"), text(b"S2\n")])]
    with stored(eng, 3, slot) as d:
        _, _, got = turn(eng, row, 3, d)
        assert got[5] == (2, 0, 1, 2 * slot - 1, 2) and got[1] == [0, 2]
        assert d.model.entry_of(1) == R.NOTHING and d.model.written.get(1) is None


def test_one_topic(eng):
    row = [B([text(b"S0\n"), text(b"P0\nfirst"), text(b"P0\nthe last one wins")]), B([text(b"P0\nnot I"), text(b"S0\n")])]
    with stored(eng, 1, 32) as d:
        _, _, got = turn(eng, row, 1, d, dest_of=[1, 0])
        # replies are ordered by segment: connection 1's publication is the turn's last
        assert d.model.value(0) == (b"not I", 1 | FIN)
        assert got[:5] == ([(0, 5, 1 | FIN, 0)] * 2, [0, 0], [0, 4], [0, 1], [1, 1]) and got[5] == (1, 0, 0, 5, 2)


# ---- header lengths and body start alignments ---------------------------------------------------

def test_every_header_length_and_every_body_start_alignment():
    """Topic ids of 1 .. 10 digits, so headers of 3 .. 12 bytes, over stores of up
    to 10^9 + 18 slots of 16 bytes.  Up to seven digits (16 MB of slots) the whole
    store is read back; above, what the turn touched is compared slot by slot and
    the rest by digest (16 GB of slots and of entries at ten digits)."""
    starts, hdrs = set(), set()
    for digits in range(1, 11):
        base = 0 if digits == 1 else 10 ** (digits - 1)
        ks = range(10) if digits == 1 else range(18)
        nt = base + len(ks)
        msgs = [text(T.header("P", base + k) + body(1 + (k * 5) % 16, k), 1 + k % 2) for k in ks]
        row = [B(msgs + [text(T.header("S", nt - 1)), text(T.header("S", base))]), B([text(T.header("S", 0))])]
        whole = digits <= 7
        with libhv_amd.Engine(0) as eng, stored(eng, nt, 16) as d:
            before = None if whole else d.digests()
            t, r, got = turn(eng, row, nt, d, whole=whole)
            assert got[1] == [nt - 1, base] + ([0] if digits == 1 else [])
            assert got[5][0] == len(ks) == len(d.model.written)
            if not whole:
                d.same_as_model_by_digest(before)
            hdrs |= {rr[0] - o for rr, (o, _, _, _), k in zip(r[0], t.rep, r[2]) if k == T.RK_PUB}
            starts |= {rr[0] % 16 for rr, k in zip(r[0], r[2]) if k == T.RK_PUB}
    assert hdrs == set(range(3, 13)) and starts == set(range(16))


# ---- reply counts on the wave, block and scan-tile edges ----------------------------------------

SUB_EDGES = (64, 255, 1023)


def message(i: int, n: int) -> bytes:
    """Reply i of n over n + 1 topics.  Publications to topic i, each the turn's
    last to it, so every edge holds a winner or a SUB; every eighth publishes
    over reply i - 2's topic (which loses); bodies of 0 .. 15 bytes (an empty
    one clears).  SUBs name the reply before them -- retained, cleared or, on
    the edges, a SUB itself and so never published -- or topic n."""
    if i % 4 == 1 or i in SUB_EDGES:
        return T.header("S", n if i % 12 == 1 else i - 1)
    return T.header("P", i - 2 if i % 8 == 6 else i) + body((i * 7) % 16, i)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_reply_counts_on_every_edge(eng, n):
    per = [n // 3 + (1 if c < n % 3 else 0) for c in range(3)]
    at, row = 0, []
    for k in per:
        row.append(B([text(message(i, n), 1 + i % 2) for i in range(at, at + k)]) if k else b"")
        at += k
    with stored(eng, n + 1, 16) as d:
        t, r, got = turn(eng, row, n + 1, d, dest_of=[5, 39, 0], cap=1 << 16)
        assert len(t.rep) == n and r[6][3] == 0
        if n >= 65:
            stored_, empty, over, _, rows = got[5]
            assert stored_ > 0 and empty > 0 and over == 0 and 0 < rows < r[6][1]
            assert r[2][n - 1] in (T.RK_PUB, T.RK_SUB) and sum(got[4]) == rows and all(c > 0 for c in got[4])


# ---- the output's end ---------------------------------------------------------------------------------

@pytest.mark.parametrize("last", [1, 15, 16, 17, 40])
def test_a_body_that_ends_at_the_last_byte_of_an_exact_capacity_output(eng, last):
    """The output buffer holds 0xEE beyond out_cap: a chunk's second aligned load
    may not leave the capacity, and what it would find there is not the body."""
    row = [B([text(b"P1\n" + body(23, 9))]), B([text(b"P0\n" + body(last, 4)), ])]
    with stored(eng, 2, 48) as d:
        with Q.replied(eng, row, fill=0xEE, exact=True) as t:
            o, ln, _, _ = t.rep[-1]
            assert o + ln == len(t.out) == t.cap
            r = Q.route(eng, t, 2, 2, [0, 1])
            retain(eng, t, r, d, 2)
        assert d.model.value(0) == (body(last, 4), 1 | FIN)


# ---- sequences ------------------------------------------------------------------------------------------

def test_a_turn_with_no_data_reply(eng):
    with stored(eng, 4, 16) as d:
        _, r, got = turn(eng, [B([PING]), b"", B([PING, CLOSE])], 4, d)
        assert got == ([], [], [], [0, 0, 0], [0, 0, 0], (0, 0, 0, 0, 0)) and not d.model.ret


@pytest.mark.parametrize("form", ["rfc", "joined"])
def test_set_overwritten_cleared_each_seen_by_a_joiner(eng, form):
    """Turns in a row on one store and one session; a joiner per turn."""
    ndest, dest_of = 3, [0, 1, 2]
    with stored(eng, 2, 32) as d, Q.session(eng, 3, form) as s:
        def one(row):
            t = s.turn(row)
            r = Q.route(eng, t, 2, ndest, dest_of)
            return retain(eng, t, r, d, 3)

        got = one([B([text(b"P1\na long first value")]), B([text(b"S1\n")]), b""])
        assert got[0] == [(32, 18, 1 | FIN, 0)] and d.model.value(1)[0] == b"a long first value"
        got = one([B([text(b"P1\nshort", 2)]), b"", B([text(b"S1\n"), text(b"S0\n")])])
        assert got[0] == [(32, 5, 2 | FIN, 0)] and got[3:5] == ([0, 0, 0], [0, 0, 1])
        assert d.model.slot_bytes(1)[:18] == b"shortg first value"        # only [0, len) was written
        got = one([B([text(b"P1\n")]), B([text(b"S1\n")]), B([PING])])
        assert got[0] == [] and got[5] == (0, 1, 0, 0, 0) and d.model.value(1) is None
        got = one([b"", B([text(b"S1\n"), text(b"P0\n" + b"x" * 33), text(b"S0\n")]), b""])   # oversize on a cleared store
        assert got[0] == [] and got[5] == (0, 0, 1, 0, 0)
        got = one([b"", B([text(b"S1\n"), text(b"U1\n")]), B([text(b"P1\nback")])])
        assert got[1:3] == ([1], [0]) and got[5] == (1, 0, 0, 4, 1)


def test_an_oversize_publication_clears_a_set_topic_and_a_stopped_one_retains_nothing(eng):
    with stored(eng, 2, 16) as d, Q.session(eng, 2) as s:
        t = s.turn([B([text(b"P0\nkeep me"), text(b"P1\nand me")]), b""])
        retain(eng, t, Q.route(eng, t, 2, 2, [0, 1]), d, 2)
        row = [B([text(b"P0\n" + b"y" * 17), text(b"S0\n")]), B([text(b"oops"), text(b"P1\nunheard"), text(b"S1\n")])]
        t = s.turn(row)
        r = Q.route(eng, t, 2, 2, [0, 1])
        assert r[2] == [T.RK_PUB, T.RK_SUB, T.RK_BAD, T.RK_STOPPED, T.RK_STOPPED]
        got = retain(eng, t, r, d, 2)
        assert got[0] == [] and got[5] == (0, 0, 1, 0, 0)
        assert d.model.value(0) is None and d.model.value(1) == (b"and me", 1 | FIN)


def test_a_join_by_a_connection_that_also_closes(eng):
    """The row is produced: the device does not decide who is still there.  The
    caller does not write a closed connection's range."""
    with stored(eng, 1, 16) as d:
        t, r, got = turn(eng, [B([text(b"P0\nstate")]), B([text(b"S0\n"), CLOSE])], 1, d)
        assert got[0] == [(0, 5, 1 | FIN, 0)] and got[3:5] == ([0, 0], [0, 1])
        assert t.flags[1] & libhv_amd.RF_CLOSED


def test_seeded_entries_count_only_where_they_are_well_formed(eng):
    """Entries the caller uploads: set == 1 with 0 < len <= slot is retained, anything else is not."""
    slot, nt = 16, 5
    ents = [(5, 2 | FIN, 1), (0, 1 | FIN, 1), (17, 1 | FIN, 1), (5, 1 | FIN, 2), (16, 1 | FIN, 1)]
    row = [B([text(b"S%d\n" % k) for k in range(nt)])]
    with stored(eng, nt, slot) as d:
        d.ret.upload(np.array(ents, libhv_amd.RETAINED_DTYPE))
        d.model.ret = dict(enumerate(ents))
        _, _, got = turn(eng, row, nt, d)
        assert got[0] == [(0, 5, 2 | FIN, 0), (64, 16, 1 | FIN, 0)] and got[1] == [0, 4]


# ---- errors, validity, determinism ----------------------------------------------------------------------

def test_every_einval_case_leaves_the_store_intact(eng):
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh, stored(fresh, 2, 16) as d:
        with pytest.raises(libhv_amd.HvwsError):
            fresh.retain(d.store, 16, d.ret)            # no route call on the context
        assert retain_none(fresh)
        d.same_as_model()
    row = [B([text(b"P0\nvalue"), text(b"S0\n")])]
    with stored(eng, 2, 16) as d, Q.session(eng, 1) as s:
        t = s.turn(row)
        with pytest.raises(libhv_amd.HvwsError):
            eng.retain(d.store, 16, d.ret)              # a reply call and no route
        r = Q.route(eng, t, 2, 1, [0])
        st, rt, out = d.store.ptr, d.ret.ptr, t.dev_out.ptr
        bad = [(st, 16, rt, 1), (st, 16, rt, 1 << 31),              # a flags bit
               (st, 0, rt, 0), (st, 8, rt, 0), (st, 24, rt, 0),      # slot 0 or no multiple of 16
               (st, 1 << 63, rt, 0),                                 # 2 * 2^63: beyond 64 bits
               (None, 16, rt, 0), (st, 16, None, 0), (st + 8, 16, rt, 0),
               (st, 16, st + 16, 0), (st, 16, st - 16, 0),           # the entries inside / reaching into the store
               (out, 16, rt, 0), (out + t.cap - 16, 16, rt, 0),      # the store over the message output
               (st, 16, out + 16, 0), (out - 16, 16, rt, 0)]
        for a in bad:
            assert L.hvws_retain(eng.ctx, *a) == -2, a
            assert retain_none(eng), a
        eng.sync()
        d.same_as_model()
        assert bytes(t.dev_out.download(len(t.out))) == bytes(t.out)
        retain(eng, t, r, d, 1)
        assert not retain_none(eng)


def test_what_ends_the_snapshot_tables(eng):
    row = [B([text(b"P0\nvalue"), text(b"S0\n")])]
    data, segs, _, _, _ = Q.R.Chain(1).inputs(row)
    with stored(eng, 1, 16) as d, Q.replied(eng, row) as t:
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        try:
            r = Q.route(eng, t, 1, 1, [0])
            retain(eng, t, r, d, 1)
            eng.route(1, 1, [0])                        # a route call
            assert retain_none(eng)
            eng.retain(d.store, 16, d.ret)
            assert not retain_none(eng)
            eng.replies(Q.POLICY)                       # a reply call
            assert retain_none(eng)
            eng.route(1, 1, [0])
            eng.retain(d.store, 16, d.ret)
            assert not retain_none(eng)
            eng.scan(rx, len(data), segs)               # a scan
            assert retain_none(eng)
            with pytest.raises(libhv_amd.HvwsError):
                eng.retain(d.store, 16, d.ret)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)
            eng.replies(Q.POLICY)
            eng.route(1, 1, [0])
            eng.retain(d.store, 16, d.ret)
            assert eng.retain_totals() == (1, 0, 0, 5, 1)
            eng.messages_rfc(rx, len(data), True, t.dev_out, t.cap)   # a message call
            assert retain_none(eng)
            d.same_as_model()                           # the same value each time: the store is the model's still
        finally:
            eng.sync()
            rx.free()


def test_random_small_turns_on_one_store(eng):
    rng = random.Random(416)
    nt, slot = 5, 16
    with stored(eng, nt, slot) as d:
        seen = set()
        for _ in range(40):
            row, _, dest_of, ndest = T.random_turn(rng, ntopics=nt)
            with Q.replied(eng, row, rng.choice(("rfc", "joined"))) as t:
                r = Q.route(eng, t, nt, ndest, dest_of)
                got = retain(eng, t, r, d, len(row))
                seen |= {i for i, v in enumerate(got[5]) if v}
        assert seen == {0, 1, 2, 3, 4}


def test_the_same_turn_twice_gives_identical_outputs(eng):
    rng = random.Random(78)
    row = [B([text(T.random_message(rng, 7)) for _ in range(300)]) for _ in range(4)]
    seen = []
    for _ in range(2):
        with stored(eng, 7, 16) as d, Q.replied(eng, row) as t:
            eng.route(7, 64, [0, 1, 2, 3])
            eng.retain(d.store, 16, d.ret)
            seen.append(tuple(a.tobytes() for a in eng.retain_table() + eng.segment_retain(4))
                        + (eng.retain_totals(), d.store.download().tobytes(), d.ret.download().tobytes()))
    assert seen[0] == seen[1] and seen[0][5][0] > 0 and seen[0][5][4] > 0


# ---- end to end: the snapshot on the wire ----------------------------------------------------------------

def test_the_send_from_the_snapshot_table_is_what_build_frames_writes(eng):
    tl = tile()
    lens = [5, 125, 126, tl + 9, 0x10000 + 7]               # one, two and eight length bytes; two fragments
    slot = (lens[-1] + 15) // 16 * 16
    nt = len(lens)
    pubs = [text(b"P%d\n" % k + body(n, k), 1 + k % 2) for k, n in enumerate(lens)]
    row = [B(pubs), B([text(b"S%d\n" % k) for k in (4, 0, 2)]), b"", B([text(b"S3\n"), text(b"S1\n"), text(b"S3\n")])]
    with stored(eng, nt, slot) as d:
        with Q.replied(eng, row, cap=1 << 17) as t:
            r = Q.route(eng, t, nt, 4, [0, 1, 2, 3])
            got = retain(eng, t, r, d, 4)
            assert got[1] == [4, 0, 2, 3, 1, 3] and got[3:5] == ([0, 0, 3, 3], [0, 3, 0, 3])
            table, d_n, cap = eng.retain_device()
            store = d.model.store_bytes()
            per = W.destination_frames(store, got[0], got[3], got[4])
            total = sum(len(b) for b in per)
            tx, moff = eng.alloc(total + 64), eng.alloc(8 * (cap + 2))
            # the same frames as hvws_build_frames' tables: a body above 0xFFFF bytes goes in two fragments
            offs, lns, fls = [], [], []
            for off, ln, fl, _ in got[0]:
                cuts = list(range(0, ln, 0xFFFF))
                for j, c in enumerate(cuts):
                    offs.append(off + c)
                    lns.append(min(0xFFFF, ln - c))
                    fls.append((fl & 0xF if j == 0 else 0) | (FIN if j == len(cuts) - 1 else 0))
            plan = libhv_amd.TxPlan(eng, offs, lns, np.array(fls, np.uint8))
            try:
                nbytes, nframes = eng.send_messages(tx, total, d.store, nt * slot, table, cap, d_n, 0, False, moff)
                assert (nbytes, nframes) == (total, len(offs))
                sent = bytes(tx.download(total))
                at = moff.download(8 * (len(got[0]) + 1), np.uint64).tolist()
                for s in range(4):
                    assert sent[at[got[3][s]]:at[got[3][s] + got[4][s]]] == per[s], s
                assert libhv_amd.lib().hvws_memset(eng.ctx, tx.ptr, 0, total) == 0
                assert eng.build_frames(tx, total + 64, d.store, nt * slot, plan) == total
                assert bytes(tx.download(total)) == sent
            finally:
                eng.sync()
                tx.free()
                moff.free()
                plan.free()
