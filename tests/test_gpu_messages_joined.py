"""GPU: hvws_messages_joined (include/hvws.h) -- whole messages across batches,
the previous output as the pending store -- against the oracle in
tests/wsjoin.py, exactly: output bytes, every piece field, first and count,
state, carry offsets and hvws_msg_bytes, the bytes from the total on untouched.
A chain of batches over two alternating buffers, carried spans around the
gather's tile and chunk edges at every source misalignment, segments without
records, equivalence with hvws_messages when nothing is pending, the errors,
the whole server turn with nothing deferred, and two more scan paths."""
from __future__ import annotations

import functools
import random

import numpy as np
import pytest

import libhv_amd
import streams
import wsharness as H
import wsjoin as J
import wsmsg as M
import wssend as S

pytestmark = pytest.mark.gpu

EINVAL = -2
PATH_RUN = 7
SENTINEL = 0xA5
SLACK = 64
FIN, MASK = M.FIN, M.MASK
IMPL = "ref" if H.have_ref() else "oracle"
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])


@pytest.fixture(params=[0, 1], ids=["wide_tiles", "one_wave_tiles"])
def geometry(request, monkeypatch):
    """Both gather geometries ($HVWS_EXPERIMENT msg, read at every call)."""
    monkeypatch.setenv("HVWS_EXPERIMENT", f"msg={request.param}")
    return request.param


def _fill(eng, buf, nbytes: int) -> None:
    assert libhv_amd.lib().hvws_memset(eng.ctx, buf.ptr, SENTINEL, nbytes) == 0


def _results(eng, out, cap: int, nseg: int):
    """What the last messages_joined left: (out bytes, pieces, (first, count),
    state, carry offsets); nothing at or beyond hvws_msg_bytes was written."""
    total = eng.msg_bytes()
    table = eng.message_table()
    fc = eng.segment_messages(nseg)
    st = eng.msg_state(nseg)
    off = eng.msg_carry(nseg)
    got = out.download(cap + SLACK)
    assert total <= cap
    assert np.all(got[total:] == SENTINEL), "bytes at or beyond the total were written"
    return got[:total].tobytes(), table, fc, st, off


def _joined(eng, data: bytes, segs, how: str, carries, state_in, prev, prev_len: int, prev_off, out, cap: int):
    """Upload, scan (payloads stay masked) or step, hvws_messages_joined."""
    rx = eng.to_device(np.frombuffer(data, dtype=np.uint8))
    _fill(eng, out, cap + SLACK)
    try:
        if how == "scan":
            eng.scan(rx, len(data), segs, carries)
        else:
            eng.step(rx, len(data), segs, carries)
        eng.messages_joined(rx, len(data), how == "scan", out, cap, state_in, prev, prev_len, prev_off)
        return _results(eng, out, cap, len(segs))
    finally:
        eng.sync()
        rx.free()


def _same(got, want, what=""):
    gout, gtab, (gfirst, gcount), gst, goff = got[:5]
    wout, wtab, (wfirst, wcount), wst, woff = want[:5]
    assert len(gout) == len(wout), what                       # hvws_msg_bytes
    assert gout == wout, (what, next(i for i in range(len(wout)) if gout[i] != wout[i]))
    assert len(gtab) == len(wtab), what
    for f in wtab.dtype.names:
        assert np.array_equal(gtab[f], wtab[f]), (what, f)
    assert list(gfirst) == list(wfirst) and list(gcount) == list(wcount), what
    for f in wst.dtype.names:
        assert np.array_equal(gst[f], wst[f]), (what, f)
    assert list(goff) == list(woff), what


# ------------------------------------------------------------------ 1. chain

@functools.lru_cache(maxsize=None)
def _chain_plan():
    """6 connections, 60 frames each, 12 batches of reads of 0-200 bytes (some
    empty) -> (streams, reads[batch][conn], bytes consumed per connection)."""
    rng = random.Random(612)
    ss = [H.build_frames_ref(J.mixed_frames(rng, 60, p_close=0.02, max_len=120)) for _ in range(6)]
    at = [0] * 6
    reads = []
    for _ in range(12):
        row = []
        for c in range(6):
            n = 0 if rng.random() < 0.2 else rng.randint(0, 200)
            row.append(ss[c][at[c]:at[c] + n])
            at[c] += len(row[-1])
        reads.append(row)
    return ss, reads, at


@pytest.mark.parametrize("how", ["scan", "step"])
def test_chain_over_two_buffers(eng, geometry, how):
    ss, reads, used = _chain_plan()
    cap = 6 * 200 + sum(used)          # a batch and everything that can be pending
    outs = [eng.alloc(cap + SLACK), eng.alloc(cap + SLACK)]
    ch = J.Chain(6)
    empty_carrying = 0
    prev_len = 0
    try:
        for k, row in enumerate(reads):
            data, segs = ch.inputs(row)
            empty_carrying += sum(1 for c in range(6) if not row[c] and int(ch.state["pending"][c]))
            want = ch.oracle(row)
            got = _joined(eng, data, segs, how, ch.carry, ch.state, outs[(k + 1) % 2] if k else None, prev_len,
                          ch.off, outs[k % 2], cap)
            _same(got, want, (how, k))
            ch.take(want)
            prev_len = len(want[0])
    finally:
        for b in outs:
            b.free()
    assert ch.totals_ok and ch.max_span >= 3 and empty_carrying >= 3
    for c in range(6):
        assert ch.logs[c] == H.run_messages(IMPL, ss[c][:used[c]], [max(used[c], 1)])[0], c
    assert sum(len(x) for x in ch.logs) > 60


# ------------------------------------------------------------------ 2. edges

@functools.lru_cache(maxsize=None)
def _edge_plan():
    """One batch: carried spans of 0, 1, 15, 16, 17, T-17 .. T+17 and 3T+5
    bytes from every source misalignment, each followed by records of 0, 1 and
    33 bytes; one range ends at prev_len; wsmsg.edge_frames(T) behind a carry."""
    T = int(libhv_amd.lib().hvws_msg_tile())
    rng = random.Random(1717)
    prev = rng.randbytes(3 * T + 5 + 48)
    lens = [0, 1, 15, 16, 17] + list(range(T - 17, T + 18)) + [3 * T + 5]
    k = rng.randbytes(4)
    tail = [H.build_frames_ref([(2 | MASK, b"", k), (0 | (FIN if i % 2 else 0) | (MASK if i % 3 else 0), rng.randbytes(1), k),
                                (0 | (FIN if i % 3 else 0) | (0 if i % 4 == 1 else MASK), rng.randbytes(33), rng.randbytes(4))])
            for i in range(len(lens))]
    parts, states, offs = [], [], []
    for i, P in enumerate(lens):
        parts.append(tail[i])
        states.append((P, 1 + i % 2, 1) if P else (M.FRESH if i % 2 else (0, 2, 1)))
        offs.append(i % 16 if P != 3 * T + 5 else 21)
    # one range ends at prev_len
    i_end = lens.index(T + 3)
    offs[i_end] = len(prev) - lens[i_end]
    # edge_frames behind 7 carried bytes from an odd offset
    parts.append(H.build_frames_ref(M.edge_frames(T)))
    states.append((7, 2, 1))
    offs.append(13)
    data, segs = J.Chain(len(parts)).inputs(parts)
    st = M.states(states)
    want = J.joined_batch(data, segs, None, st, prev, offs)
    return T, prev, data, segs, st, np.array(offs, np.uint64), want, lens


@pytest.mark.parametrize("how", ["scan", "step"])
def test_carried_spans_around_tile_and_chunk_edges(eng, geometry, how):
    T, prev, data, segs, st, offs, want, lens = _edge_plan()
    total = len(want[0])
    assert total < (1 << 20) and len(data) < (1 << 20)
    assert {int(o) % 16 for o, P in zip(offs, lens) if P} == set(range(16))
    assert int(offs[lens.index(T + 3)]) + T + 3 == len(prev)
    # carried-row / record boundaries at every chunk offset, on both sides of a carried row
    starts = {int(p["off"]) % 16 for p in want[1] if int(p["info"]) & M.M_CONT}
    ends = {(int(want[1][int(f)]["off"]) + P) % 16 for f, P in zip(want[2][0], lens) if P}
    assert starts == set(range(16)) and ends == set(range(16))
    # whole tiles inside one carried span, read from a misaligned source
    big = lens.index(3 * T + 5)
    assert int(want[1][int(want[2][0][big])]["len"]) >= 3 * T + 5 and int(offs[big]) % 16
    pbuf = eng.to_device(np.frombuffer(prev, np.uint8), pad=0)
    out = eng.alloc(total + SLACK)
    try:
        got = _joined(eng, data, segs, how, None, st, pbuf, len(prev), offs, out, total)
        _same(got, want, how)
    finally:
        pbuf.free()
        out.free()


# ------------------------------------------------------ 3. recordless segments

def test_segments_without_records(eng, geometry):
    T = int(libhv_amd.lib().hvws_msg_tile())
    rng = random.Random(33)
    prev = rng.randbytes(T + 4099 + 40)
    pbuf = eng.to_device(np.frombuffer(prev, np.uint8), pad=0)
    a = H.build_frames_ref([(1 | MASK, b"open ", KEY), (0 | FIN | MASK, b"shut", KEY), (2 | MASK, b"tail", KEY)])
    b = H.build_frames_ref([(0 | FIN | MASK, b"!", KEY)])
    cases = [
        # records, no records with and without pending bytes, one header byte only (no record yet)
        ([a, b"", b"", b, b"", b[:1], b""],
         [M.FRESH, (20, 1, 1), (0, 9, 0), (5, 2, 1), (T + 3, 0, 1), (9, 2, 1), (0, 1, 1)],
         [0, 3, 99, 17, 30, 1, 0]),
        # only such segments, and no bytes at all
        ([b"", b"", b"", b""], [M.FRESH, (9, 10, 1), (0, 2, 1), (4099, 1, 1)], [0, len(prev) - 9, 5, 2]),
    ]
    out = eng.alloc(2 * T + 8192 + SLACK)
    try:
        for parts, states, offs in cases:
            data, segs = J.Chain(len(parts)).inputs(parts)
            st = M.states(states)
            want = J.joined_batch(data, segs, None, st, prev, offs)
            cap = len(data) + sum(p for p, _, _ in states)
            for how in ("scan", "step"):
                got = _joined(eng, data, segs, how, None, st, pbuf, len(prev), offs, out, cap)
                _same(got, want, (len(parts), how))
            for s, (P, op, opened) in enumerate(states):
                if segs[s][1] > 1:
                    continue
                f, c = int(got[2][0][s]), int(got[2][1][s])
                assert tuple(int(x) for x in got[3][s]) == (P, op, opened)   # the state unchanged
                assert c == (1 if P else 0)
                if P:
                    p = got[1][f]
                    assert (int(p["len"]), int(p["total"]), int(p["rec"])) == (P, P, J.NOREC)
                    assert int(p["info"]) == (op or 8) | M.M_CONT
                    assert got[0][int(p["off"]): int(p["off"]) + P] == prev[offs[s]: offs[s] + P]
                    assert int(got[4][s]) == int(p["off"])
        assert len(data) == 0   # the last case: rx_len == 0 with carried bytes
    finally:
        pbuf.free()
        out.free()


# ------------------------------------------------------------ 4. equivalence

def test_nothing_pending_equals_hvws_messages(eng, geometry):
    rng = random.Random(44)
    parts = [streams.rand_stream(rng, rng.randrange(0, 40), max_len=90) for _ in range(9)]
    parts[4] = b""
    data, segs = J.Chain(9).inputs(parts)
    st = M.states([M.FRESH if s % 3 == 0 else (0, 2, 1) if s % 3 == 1 else (0, 9, 0) for s in range(9)])
    n = len(data)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = eng.alloc(n + SLACK)
    try:
        eng.scan(rx, n, segs)
        res = []
        for joined in (False, True):
            _fill(eng, out, n + SLACK)
            if joined:
                eng.messages_joined(rx, n, True, out, n, st)   # d_prev and prev_off NULL
            else:
                eng.messages(rx, n, True, out, n, st)
            total = eng.msg_bytes()
            res.append((out.download(n + SLACK).tobytes(), total, eng.message_table(), eng.segment_messages(9),
                        eng.msg_state(9)))
        plain, join = res
        assert plain[0] == join[0] and plain[1] == join[1]
        assert plain[2].tolist() == join[2].tolist() and len(plain[2]) > 50
        assert plain[3][0].tolist() == join[3][0].tolist() and plain[3][1].tolist() == join[3][1].tolist()
        assert plain[4].tolist() == join[4].tolist()
        want = J.joined_batch(data, segs, None, st)
        assert eng.msg_carry(9).tolist() == want[4].tolist()
    finally:
        rx.free()
        out.free()


# ------------------------------------------------------------------ 5. errors

def test_errors():
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as e:
        data = H.build_frames_ref([(1 | MASK, b"part one, ", KEY), (0 | MASK, b"part two", KEY)])
        n = len(data)
        prev_bytes = bytes(range(64))
        P = 23
        st = M.states([(P, 1, 1)])
        off = np.array([40], np.uint64)
        want = J.joined_batch(data, [(0, n)], None, st, prev_bytes, off)
        total = len(want[0])
        assert total == P + 18 and total % 16 not in (0, 15)
        rx = e.to_device(np.frombuffer(data, np.uint8))
        prev = e.to_device(np.frombuffer(prev_bytes, np.uint8), pad=0)
        out = e.alloc(256 + SLACK)
        _fill(e, out, 256 + SLACK)

        def call(d_out, cap, state, d_prev, prev_len, prev_off):
            return L.hvws_messages_joined(e.ctx, rx.ptr, n, 1, d_out, cap, state.ctypes.data if state is not None else None,
                                          d_prev, prev_len, prev_off.ctypes.data if prev_off is not None else None)

        def untouched():
            return bool(np.all(out.download(256 + SLACK) == SENTINEL))

        assert call(out.ptr, 256, st, prev.ptr, 64, off) == EINVAL               # no scan yet
        e.scan(rx, n, [(0, n)])
        assert call(out.ptr, 256, st, None, 0, off) == EINVAL                    # pending without d_prev
        assert call(out.ptr, 256, st, prev.ptr, 64, None) == EINVAL              # ... without prev_off
        assert call(out.ptr, 256, st, prev.ptr, 64, np.array([42], np.uint64)) == EINVAL    # 42 + 23 > 64
        assert call(out.ptr, 256, st, prev.ptr, 64, np.array([1 << 63], np.uint64)) == EINVAL
        assert call(out.ptr, 256, st, prev.ptr, 62, off) == EINVAL               # past a shorter prev_len
        assert call(out.ptr, 256, st, prev.ptr + 8, 56, off) == EINVAL           # misaligned d_prev
        assert call(out.ptr, 256, st, out.ptr + 128, 64, off) == EINVAL          # d_out overlaps d_prev
        assert call(out.ptr + 8, 200, st, prev.ptr, 64, off) == EINVAL           # misaligned d_out
        assert call(out.ptr, total - 1, st, prev.ptr, 64, off) == EINVAL         # one byte short: after the wait
        assert L.hvws_msg_count(e.ctx) == -1
        assert untouched()
        assert call(out.ptr, total, st, prev.ptr, 64, np.array([41], np.uint64)) == 0   # the range ends at prev_len
        assert call(out.ptr, total, st, prev.ptr, 64, off) == 0                  # exactly enough
        got = _results(e, out, total, 1)
        _same(got, want)
        assert np.all(out.download(256 + SLACK)[total:] == SENTINEL)
        # a plain pass leaves no carry offsets
        e.messages(rx, n, True, out, 256)
        assert L.hvws_get_msg_carry(e.ctx, off.ctypes.data) == EINVAL
        # d_out overlapping the batch
        both = e.alloc(2 * n + 64)
        both.upload(np.frombuffer(data, np.uint8))
        e.scan(both, n, [(0, n)])
        assert L.hvws_messages_joined(e.ctx, both.ptr, n, 1, both.ptr + 16, n + P, st.ctypes.data, prev.ptr, 64,
                                      off.ctypes.data) == EINVAL
        for b in (rx, prev, out, both):
            b.free()


# ---------------------------------------------------------------- 6. the turn

def _turn_plan():
    """Three connections over four batches: a masked PING of 100 bytes in 3
    batches; a text of 3 fragments with a PING between them in 4; a CLOSE in 2
    with data frames after it."""
    B = H.build_frames_ref
    k2 = bytes([9, 8, 7, 6])
    ping = B([(9 | FIN | MASK, bytes(range(100)), KEY), (1 | FIN | MASK, b"after the ping", k2)])
    text = B([(1 | MASK, b"A" * 40, KEY), (0 | MASK, b"B" * 30, k2), (9 | FIN | MASK, b"PING", KEY),
              (0 | FIN | MASK, b"C" * 50, k2), (2 | FIN | MASK, b"bin", KEY)])
    close = B([(2 | FIN | MASK, b"first", KEY), (8 | FIN | MASK, b"\x03\xe8 going away now", k2),
               (1 | FIN | MASK, b"ignored", KEY), (9 | FIN | MASK, b"late", k2)])
    cuts = [[30, 80, len(ping)],                                  # inside the PING's payload, twice
            [20, 60, 6 + 40 + 6 + 30 + 6 + 2, len(text)],        # in fragment 1, fragment 2, the PING, the rest
            [6 + 5 + 6 + 7, len(close)]]                          # inside the CLOSE
    ss = [ping, text, close]
    reads = []
    for k in range(4):
        row = []
        for s, c in zip(ss, cuts):
            a = c[k - 1] if 0 < k <= len(c) else (0 if k == 0 else len(s))
            b = c[k] if k < len(c) else len(s)
            row.append(s[a:b])
        reads.append(row)
    assert all(b"".join(r[i] for r in reads) == ss[i] for i in range(3))
    return ss, reads


@pytest.mark.parametrize("joined", [True, False], ids=["joined", "plain_defers"])
def test_the_turn_defers_nothing(eng, joined):
    policy = S.R_SERVER | S.R_ECHO
    ss, reads = _turn_plan()
    cap = 1024
    outs = [eng.alloc(cap + SLACK), eng.alloc(cap + SLACK)]
    tx = eng.alloc(4096)
    moff = eng.alloc(8 * 256)
    ch = J.Chain(3)
    plain_state, plain_carry = M.states([M.FRESH] * 3), [None] * 3
    closed = [0, 0, 0]
    sent = [b"", b"", b""]
    deferred = 0
    prev_len = 0
    try:
        for k, row in enumerate(reads):
            data, segs = ch.inputs(row)
            rx = eng.to_device(np.frombuffer(data, np.uint8))
            cur, old = outs[k % 2], outs[(k + 1) % 2]
            eng.scan(rx, len(data), segs, ch.carry if joined else plain_carry)
            if joined:
                want = ch.oracle(row)
                eng.messages_joined(rx, len(data), True, cur, cap, ch.state, old if k else None, prev_len, ch.off)
            else:
                eng.messages(rx, len(data), True, cur, cap, plain_state)
            eng.replies(policy, closed)
            table, d_n, n = eng.replies_device()
            assert n + 1 <= 256   # moff holds the table's capacity
            nbytes, _ = eng.send_messages(tx, 4096, cur, cap, table, n, d_n, 0, False, moff)
            flags = eng.reply_flags(3).tolist()
            deferred += sum(1 for f in flags if f & S.RF_DEFERRED)
            first, count = eng.segment_replies(3)
            offs = moff.download(8 * (int(first[2]) + int(count[2]) + 1), np.uint64).tolist()
            got = bytes(tx.download(nbytes)) if nbytes else b""
            for s in range(3):
                sent[s] += got[offs[int(first[s])]: offs[int(first[s]) + int(count[s])]]
            closed = [1 if f & S.RF_CLOSED else 0 for f in flags]
            if joined:
                _same(_results_no_sentinel(eng, cur, 3), want, k)
                ch.take(want)
                prev_len = len(want[0])
            else:
                o = M.oracle_batch(data, segs, plain_carry, plain_state, with_carry=True)
                plain_state, plain_carry = o[3], o[4]
            rx.free()
    finally:
        eng.sync()
        for b in outs + [tx, moff]:
            b.free()
    if not joined:
        assert deferred >= 3   # the gap: each split message's reply is left to the host
        return
    assert deferred == 0
    for s in range(3):
        log = H.run_messages(IMPL, ss[s], [len(ss[s])])[0]
        assert ch.logs[s] == log
        rep, was_closed = S.replies_of_messages(log, policy)
        assert sent[s] == S.expected([(fl, d, 0) for fl, d in rep], 0, False)[0], s
        assert was_closed == (s == 2)
    assert closed == [0, 0, 1]
    # nothing follows the CLOSE: its reply is the connection's last frame
    assert sent[2].endswith(H.build_frames_ref([(8 | FIN, b"\x03\xe8 going away now", None)]))


def _results_no_sentinel(eng, out, nseg: int):
    total = eng.msg_bytes()
    return (out.download(total).tobytes() if total else b"", eng.message_table(), eng.segment_messages(nseg),
            eng.msg_state(nseg), eng.msg_carry(nseg))


# -------------------------------------------------- 7. scan-path independence

def _equal_frames_batch():
    """64 segments of 6 equal 200-byte frames; every third connection has an
    open message of 10 + s bytes pending."""
    r = random.Random(9)
    frames = [(0x31 if i % 5 else 0x21, r.randbytes(200), r.randbytes(4)) for i in range(64 * 6)]
    data = H.build_frames_ref(frames)
    size = len(data) // len(frames)
    assert size == 208
    segs = [(s * 6 * size, 6 * size) for s in range(64)]
    prev = r.randbytes(4096)
    st = M.states([(10 + s, 2, 1) if s % 3 == 0 else M.FRESH for s in range(64)])
    offs = np.array([61 * s + 3 for s in range(64)], np.uint64)
    return data, segs, prev, st, offs, J.joined_batch(data, segs, None, st, prev, offs)


def test_after_a_run_step(eng):
    L = libhv_amd.lib()
    data, segs, prev, st, offs, want = _equal_frames_batch()
    cap = len(want[0])
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    pbuf = eng.to_device(np.frombuffer(prev, np.uint8), pad=0)
    out = eng.alloc(cap + SLACK)
    _fill(eng, out, cap + SLACK)
    old_bound = L.hvws_set_fast_bound(eng.ctx, 1)
    old_run = L.hvws_set_run(eng.ctx, 1)
    try:
        eng.step(rx, len(data), segs)
        assert L.hvws_last_scan_path(eng.ctx) == PATH_RUN
        eng.messages_joined(rx, len(data), False, out, cap, st, pbuf, len(prev), offs)
        got = _results(eng, out, cap, 64)
    finally:
        L.hvws_set_run(eng.ctx, old_run)
        L.hvws_set_fast_bound(eng.ctx, old_bound)
        eng.sync()
        for b in (rx, pbuf, out):
            b.free()
    _same(got, want)


def test_behind_a_resident_step(eng):
    data, segs, prev, st, offs, want = _equal_frames_batch()
    other = H.build_frames_ref(streams.rand_frames(random.Random(5), 70, max_len=80))
    cap = len(want[0])
    rx = [eng.to_device(np.frombuffer(d, np.uint8)) for d in (data, other)]
    pbuf = eng.to_device(np.frombuffer(prev, np.uint8), pad=0)
    out = eng.alloc(cap + SLACK)
    _fill(eng, out, cap + SLACK)
    try:
        eng.step_resident(rx[0], len(data), segs)
        eng.messages_joined(rx[0], len(data), False, out, cap, st, pbuf, len(prev), offs)
        eng.step_resident(rx[1], len(other), [(0, len(other))])   # the next step queues behind the pass
        got = _results(eng, out, cap, 64)
        assert eng.last_kernel_ms() >= 0
    finally:
        eng.sync()
        for b in rx + [pbuf, out]:
            b.free()
    _same(got, want)
