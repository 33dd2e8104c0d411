"""GPU: hvws_messages_rfc (include/hvws.h) -- RFC 6455's message rule, control
frames apart from the fragmented data message they interrupt -- against the
oracle in tests/wsrfc.py, exactly: output bytes, every piece field, first and
count, hvws_rfc_state with its offsets and hvws_msg_bytes, the bytes from the
total on untouched.  The Q5 stream whole and cut at every byte, a chain of a
few hundred connections over two alternating buffers on three scan paths,
record boundaries and class changes around the gather's tile edges, the
connection shapes the two classes add, a small out_cap, the errors, and
equality with hvws_messages_joined when a batch has no control frames."""
from __future__ import annotations

import functools
import random

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wsjoin as J
import wsmsg as M
import wsrfc as R

pytestmark = pytest.mark.gpu

EINVAL = -2
PATH_RUN = 7
SENTINEL = 0xA5
SLACK = 64
FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
Q5 = [(1 | MASK, b"AB", KEY), (9 | FIN | MASK, b"PING", KEY), (0 | FIN | MASK, b"CD", KEY)]


@pytest.fixture(params=[0, 1], ids=["wide_tiles", "one_wave_tiles"])
def geometry(request, monkeypatch):
    """Both gather geometries ($HVWS_EXPERIMENT msg, read at every call)."""
    monkeypatch.setenv("HVWS_EXPERIMENT", f"msg={request.param}")
    return request.param


def _fill(eng, buf, nbytes: int) -> None:
    assert libhv_amd.lib().hvws_memset(eng.ctx, buf.ptr, SENTINEL, nbytes) == 0


def _results(eng, out, cap: int, nseg: int):
    """What the last messages_rfc left: (out bytes, pieces, (first, count),
    state); nothing at or beyond hvws_msg_bytes was written."""
    total = eng.msg_bytes()
    table = eng.message_table()
    fc = eng.segment_messages(nseg)
    st = eng.rfc_state(nseg)
    got = out.download(cap + SLACK)
    assert total <= cap
    assert np.all(got[total:] == SENTINEL), "bytes at or beyond the total were written"
    return got[:total].tobytes(), table, fc, st


def _rfc(eng, data: bytes, segs, how: str, carries, state_in, prev, prev_len: int, out, cap: int):
    """Upload, scan (payloads stay masked) or step, hvws_messages_rfc."""
    rx = eng.to_device(np.frombuffer(data, dtype=np.uint8))
    _fill(eng, out, cap + SLACK)
    try:
        if how == "scan":
            eng.scan(rx, len(data), segs, carries)
        else:
            eng.step(rx, len(data), segs, carries)
        eng.messages_rfc(rx, len(data), how == "scan", out, cap, state_in, prev, prev_len)
        return _results(eng, out, cap, len(segs))
    finally:
        eng.sync()
        rx.free()


def _same(got, want, what=""):
    gout, gtab, (gfirst, gcount), gst = got[:4]
    wout, wtab, (wfirst, wcount), wst = want[:4]
    assert len(gout) == len(wout), what                       # hvws_msg_bytes
    assert gout == wout, (what, next(i for i in range(len(wout)) if gout[i] != wout[i]))
    assert len(gtab) == len(wtab), what
    for f in wtab.dtype.names:
        assert np.array_equal(gtab[f], wtab[f]), (what, f)
    assert list(gfirst) == list(wfirst) and list(gcount) == list(wcount), what
    assert gst.tolist() == wst.tolist(), what


# ------------------------------------------------------------ 1. the Q5 stream

def test_q5_stream_whole_and_cut_at_every_byte(eng):
    data = H.build_frames_ref(Q5)
    outs = [eng.alloc(64 + SLACK), eng.alloc(64 + SLACK)]
    try:
        for cut in range(len(data) + 1):
            ch = R.Chain(1)
            prev_len = 0
            for k, part in enumerate((data[:cut], data[cut:]) if cut < len(data) else (data,)):
                d, segs, _, carries, st = ch.inputs([part])
                want = ch.oracle([part])
                got = _rfc(eng, d, segs, "scan", carries, st, outs[(k + 1) % 2] if k else None, prev_len,
                           outs[k % 2], 64)
                _same(got, want, (cut, k))
                ch.take(want, [part])
                prev_len = len(want[0])
            assert ch.data_log[0] == [(1, b"ABCD")] and ch.ctl_log[0] == [(9, b"PING")], cut
    finally:
        for b in outs:
            b.free()


# ------------------------------------------------------------------ 2. chain

NCONN, NBATCH = 240, 6


@functools.lru_cache(maxsize=None)
def _chain_plan():
    """240 connections of 24 mixed frames, 6 batches of reads of 0-160 bytes,
    some empty, some connections left out -> (reads[batch][conn], the oracle's
    result per batch, what each call takes); computed once for every path."""
    rng = random.Random(6455)
    ss = [H.build_frames_ref(J.mixed_frames(rng, 24, p_close=0.02, max_len=120)) for _ in range(NCONN)]
    at = [0] * NCONN
    ch = R.Chain(NCONN)
    steps = []
    left_out = empty_carrying = 0
    for _ in range(NBATCH):
        row = []
        for c in range(NCONN):
            pending = int(ch.state["data"]["pending"][c]) + int(ch.state["ctl"]["pending"][c])
            x = rng.random()
            if x < 0.08 and not pending:
                row.append(None)
                left_out += 1
                continue
            n = 0 if x < 0.25 else rng.randint(0, 160)
            row.append(ss[c][at[c]:at[c] + n])
            at[c] += len(row[-1])
            empty_carrying += 1 if not row[-1] and pending else 0
        inp = ch.inputs(row)
        want = ch.oracle(row)
        steps.append((inp, want, len(ch.prev)))
        ch.take(want, row)
    assert left_out >= 20 and empty_carrying >= 20 and ch.totals_ok
    ctl_carried = sum(1 for _, w, _ in steps for s in w[3] if int(s["ctl"]["pending"]))
    both = sum(1 for _, w, _ in steps for s in w[3] if int(s["ctl"]["pending"]) and int(s["data"]["pending"]))
    assert ctl_carried >= 20 and both >= 5
    assert sum(len(x) for x in ch.ctl_log) > 500 and sum(len(x) for x in ch.data_log) > 500
    cap = max(len(w[0]) for _, w, _ in steps)
    assert cap < (1 << 20)
    return steps, cap


@pytest.mark.parametrize("how", ["scan", "step"])
def test_chain_over_two_buffers(eng, geometry, how):
    steps, cap = _chain_plan()
    outs = [eng.alloc(cap + SLACK), eng.alloc(cap + SLACK)]
    try:
        for k, ((data, segs, _, carries, st), want, prev_len) in enumerate(steps):
            got = _rfc(eng, data, segs, how, carries, st, outs[(k + 1) % 2] if k else None, prev_len, outs[k % 2], cap)
            _same(got, want, (how, k))
    finally:
        for b in outs:
            b.free()


# ------------------------------------------------------------------ 3. edges

@functools.lru_cache(maxsize=None)
def _edge_plan():
    """Two connections.  A: wsmsg.edge_frames(T) -- record boundaries at every
    offset around two multiples of the tile -- with a short control frame
    behind every frame, so the data bytes lie as edge_frames lays them and the
    class changes at every one of those boundaries.  B: the same layout in the
    CONTROL class (every frame a control frame, short data frames between them),
    behind a data frame that brings B's control bytes to a multiple of the
    tile.  Both behind carried bytes of both classes."""
    T = int(libhv_amd.lib().hvws_msg_tile())
    rng = random.Random(929)
    prev = rng.randbytes(600)
    edge = M.edge_frames(T)
    a, b = [], []
    for i, (fl, body, key) in enumerate(edge):
        a.append((fl & ~0xF | (fl & 0xF if fl & 0xF < 8 else 2), body, key))
        a.append(((9, 10, 8)[i % 3] | (FIN if i % 4 else 0) | (MASK if i % 2 else 0), rng.randbytes(i % 4), rng.randbytes(4)))
        b.append((fl & ~0xF | (9, 10, 11)[i % 3], body, key))
        b.append(((0, 1, 2)[i % 3] | (FIN if i % 3 else 0) | (MASK if i % 2 else 0), rng.randbytes(i % 3), rng.randbytes(4)))
    st = R.states([((7, 2, 1), (5, 9, 1), 13, 101), ((3, 1, 1), (0, 0, 0), 222, 0)])
    da, db = H.build_frames_ref(a), H.build_frames_ref(b)
    probe = R.rfc_batch(da + db, [(0, len(da)), (len(da), len(db))], None, st, prev)
    first_ctl_b = next(int(p["off"]) for p in probe[1] if int(p["seg"]) == 1 and int(p["info"]) & R.M_CTL)
    pad = (-first_ctl_b) % T
    if pad:
        b.insert(0, (2 | FIN | MASK, rng.randbytes(pad), rng.randbytes(4)))
        db = H.build_frames_ref(b)
    data, segs = da + db, [(0, len(da)), (len(da), len(db))]
    want = R.rfc_batch(data, segs, None, st, prev)
    return T, prev, data, segs, st, want


@pytest.mark.parametrize("how", ["scan", "step"])
def test_record_boundaries_and_class_changes_around_tile_edges(eng, geometry, how):
    T, prev, data, segs, st, want = _edge_plan()
    total = len(want[0])
    assert total < (1 << 20) and len(data) < (1 << 20)
    tab = want[1]
    # B's control bytes begin at a multiple of the tile; both classes have pieces ending at
    # every offset around a multiple of it
    assert next(int(p["off"]) for p in tab if int(p["seg"]) == 1 and int(p["info"]) & R.M_CTL) % T == 0
    # ... every control record ends a piece: pieces end at every offset around a multiple of it;
    # a data piece ends where a FIN frame does, 4 in 5 of edge_frames' one-byte records
    for ctl, atleast in ((0, 12), (R.M_CTL, 17)):
        ends = {(int(p["off"]) + int(p["len"])) % T for p in tab if int(p["info"]) & R.M_CTL == ctl}
        near = {e if e < T // 2 else e - T for e in ends}
        assert len(near & set(range(-8, 9))) >= atleast, (ctl, sorted(near)[:40])
    pbuf = eng.to_device(np.frombuffer(prev, np.uint8), pad=0)
    out = eng.alloc(total + SLACK)
    try:
        got = _rfc(eng, data, segs, how, None, st, pbuf, len(prev), out, total)
        _same(got, want, how)
    finally:
        pbuf.free()
        out.free()


# ------------------------------------------------------- 4. connection shapes

def test_connection_shapes(eng, geometry):
    """Only control frames; only pending bytes (the two pieces without a
    record); one header byte only; nothing at all; a control frame of 300 bytes
    cut across three batches, with a fragmented text around it."""
    B = H.build_frames_ref
    rng = random.Random(31)
    only_ctl = B([(9 | MASK, b"one", KEY), (10 | FIN, b"two", None), (9 | FIN | MASK, b"no end", KEY)])[:-2]
    long_ping = B([(1 | MASK, b"text, ", KEY), (9 | FIN | MASK, bytes(range(256)) + b"x" * 44, KEY),
                   (0 | FIN | MASK, b"continued", KEY)])
    cuts = [6 + 6 + 8 + 90, 6 + 6 + 8 + 230]
    prev0 = rng.randbytes(200)
    reads = [
        [only_ctl, b"", b"\x81", b"", long_ping[:cuts[0]]],
        [b"", b"", b"", b"", long_ping[cuts[0]:cuts[1]]],
        [b"", b"", b"", b"", long_ping[cuts[1]:]],
    ]
    ch = R.Chain(5)
    ch.prev = prev0
    ch.state[1] = ((40, 2, 1), (9, 9, 1), 150, 7)     # pending in both classes, never a read
    outs = [eng.alloc(1024 + SLACK), eng.alloc(1024 + SLACK)]
    pbuf = eng.to_device(np.frombuffer(prev0, np.uint8), pad=0)
    try:
        prev, prev_len = pbuf, len(prev0)
        for k, row in enumerate(reads):
            data, segs, _, carries, st = ch.inputs(row)
            want = ch.oracle(row)
            for how in ("scan", "step"):
                got = _rfc(eng, data, segs, how, carries, st, prev, prev_len, outs[k % 2], 1024)
                _same(got, want, (k, how))
            f, c = int(got[2][0][1]), int(got[2][1][1])
            assert c == 2   # the two pieces without a record, data first
            for j, (n, op, flag) in enumerate(((40, 2, 0), (9, 9, R.M_CTL))):
                p = got[1][f + j]
                assert (int(p["len"]), int(p["total"]), int(p["rec"])) == (n, n, R.NOREC)
                assert int(p["info"]) == op | M.M_CONT | flag
            assert got[3][1]["data"].tolist() == (40, 2, 1) and got[3][1]["ctl"].tolist() == (9, 9, 1)
            assert int(got[2][1][3]) == 0 and int(got[2][1][2]) == 0   # nothing at all; a header byte only
            ch.take(want, row)
            prev, prev_len = outs[k % 2], len(want[0])
    finally:
        for b in outs + [pbuf]:
            b.free()
    assert ch.ctl_log[0] == [(9, b"one"), (10, b"two")] and ch.data_log[0] == []
    assert int(ch.state[0]["ctl"]["pending"]) == 4 and int(ch.state[0]["ctl"]["open"]) == 1   # "no e"
    assert ch.prev[int(ch.state[0]["ctl_off"]):][:4] == b"no e"
    assert ch.ctl_log[4] == [(9, bytes(range(256)) + b"x" * 44)]
    assert ch.data_log[4] == [(1, b"text, continued")]
    assert ch.totals_ok


# ----------------------------------------------------------- 5. after a RUN step

def test_after_a_run_step(eng):
    """64 segments of 6 equal frames, a PING between two fragments in each;
    every third connection has bytes pending in both classes."""
    L = libhv_amd.lib()
    r = random.Random(9)
    ops = (1, 9 | FIN, 0 | FIN, 2 | FIN, 10 | FIN, 1)
    frames = [(ops[i % 6] | MASK, r.randbytes(100), r.randbytes(4)) for i in range(64 * 6)]
    data = H.build_frames_ref(frames)
    size = len(data) // len(frames)
    assert size == 106
    segs = [(s * 6 * size, 6 * size) for s in range(64)]
    prev = r.randbytes(4096)
    st = R.states([((10 + s, 2, 1), (3 + s % 5, 9, 1), 61 * s + 3, 59 * s + 1) if s % 3 == 0 else R.FRESH
                   for s in range(64)])
    want = R.rfc_batch(data, segs, None, st, prev)
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
        eng.messages_rfc(rx, len(data), False, out, cap, st, pbuf, len(prev))
        got = _results(eng, out, cap, 64)
        assert eng.last_kernel_ms() >= 0
    finally:
        L.hvws_set_run(eng.ctx, old_run)
        L.hvws_set_fast_bound(eng.ctx, old_bound)
        eng.sync()
        for b in (rx, pbuf, out):
            b.free()
    _same(got, want)


# ------------------------------------------------- 6. out_cap and the errors

def test_out_cap_and_errors():
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as e:
        data = H.build_frames_ref([(1 | MASK, b"part one, ", KEY), (9 | FIN | MASK, b"ping!", KEY),
                                   (0 | MASK, b"part two", KEY)])
        n = len(data)
        prev_bytes = bytes(range(64))
        Pd, Pc = 23, 4
        st = R.states([((Pd, 1, 1), (Pc, 9, 1), 40, 3)])
        want = R.rfc_batch(data, [(0, n)], None, st, prev_bytes)
        total = len(want[0])
        assert total == Pd + 18 + Pc + 5 and total % 16 not in (0, 15)
        rx = e.to_device(np.frombuffer(data, np.uint8))
        prev = e.to_device(np.frombuffer(prev_bytes, np.uint8), pad=0)
        out = e.alloc(256 + SLACK)
        _fill(e, out, 256 + SLACK)
        tmp = np.zeros(1, libhv_amd.RFC_STATE_DTYPE)

        def call(d_out, cap, state, d_prev, prev_len):
            return L.hvws_messages_rfc(e.ctx, rx.ptr, n, 1, d_out, cap, state.ctypes.data if state is not None else None,
                                       d_prev, prev_len)

        def untouched():
            return bool(np.all(out.download(256 + SLACK) == SENTINEL))

        def with_(**kw):
            s = st.copy()
            for k, v in kw.items():
                if k in ("data", "ctl"):
                    s[k][0] = v
                else:
                    s[k][0] = v
            return s

        assert call(out.ptr, 256, st, prev.ptr, 64) == EINVAL                      # no scan yet
        e.scan(rx, n, [(0, n)])
        assert L.hvws_get_rfc_state(e.ctx, tmp.ctypes.data) == EINVAL              # no rfc call yet
        assert call(out.ptr, 256, st, None, 0) == EINVAL                           # pending without d_prev
        assert call(out.ptr, 256, with_(data_off=42), prev.ptr, 64) == EINVAL      # 42 + 23 > 64
        assert call(out.ptr, 256, with_(ctl_off=61), prev.ptr, 64) == EINVAL       # 61 + 4 > 64: the control class's
        assert call(out.ptr, 256, with_(ctl_off=1 << 63), prev.ptr, 64) == EINVAL
        assert call(out.ptr, 256, st, prev.ptr, 62) == EINVAL                      # past a shorter prev_len
        assert call(out.ptr, 256, with_(data=(5, 1, 0)), prev.ptr, 64) == EINVAL   # pending, not open
        assert call(out.ptr, 256, with_(ctl=(4, 16, 1)), prev.ptr, 64) == EINVAL   # no opcode
        assert call(out.ptr, 256, st, prev.ptr + 8, 56) == EINVAL                  # misaligned d_prev
        assert call(out.ptr, 256, st, out.ptr + 128, 64) == EINVAL                 # d_out overlaps d_prev
        assert call(out.ptr + 8, 200, st, prev.ptr, 64) == EINVAL                  # misaligned d_out
        assert call(out.ptr, total - 1, st, prev.ptr, 64) == EINVAL                # one byte short: after the wait
        assert L.hvws_msg_count(e.ctx) == -1
        assert untouched()
        assert call(out.ptr, total, with_(data_off=41, ctl_off=60), prev.ptr, 64) == 0   # both ranges end at prev_len
        assert call(out.ptr, total, st, prev.ptr, 64) == 0                         # exactly enough: fits after the wait
        got = _results(e, out, total, 1)
        _same(got, want)
        # the other forms' state getters refuse, and the rfc getter after them
        ms = np.zeros(1, libhv_amd.MSG_STATE_DTYPE)
        off = np.zeros(1, np.uint64)
        assert L.hvws_get_msg_state(e.ctx, ms.ctypes.data) == EINVAL
        assert L.hvws_get_msg_carry(e.ctx, off.ctypes.data) == EINVAL
        e.messages_joined(rx, n, True, out, 256)
        assert L.hvws_get_rfc_state(e.ctx, tmp.ctypes.data) == EINVAL
        assert L.hvws_get_msg_state(e.ctx, ms.ctypes.data) == 0
        # d_out overlapping the batch
        both = e.alloc(2 * n + 64)
        both.upload(np.frombuffer(data, np.uint8))
        e.scan(both, n, [(0, n)])
        assert L.hvws_messages_rfc(e.ctx, both.ptr, n, 1, both.ptr + 16, n + Pd + Pc, st.ctypes.data, prev.ptr, 64) == EINVAL
        for b in (rx, prev, out, both):
            b.free()


# ------------------------------------------------------------ 7. equivalence

def test_without_control_frames_it_equals_hvws_messages_joined(eng, geometry):
    rng = random.Random(44)
    parts = []
    for s in range(9):
        frames = []
        for _ in range(rng.randrange(0, 40)):
            nb = rng.choice([0, 1, rng.randrange(91)])
            frames.append((rng.choice([0, 0, 1, 2]) | (FIN if rng.random() < 0.6 else 0) | (0 if rng.random() < 0.1 else MASK),
                           rng.randbytes(nb), rng.randbytes(4)))
        parts.append(H.build_frames_ref(frames))
    parts[4] = b""
    data, segs = J.Chain(9).inputs(parts)
    prev_bytes = rng.randbytes(256)
    js = M.states([M.FRESH if s % 3 == 0 else (7 + s, 2, 1) if s % 3 == 1 else (0, 1, 0) for s in range(9)])
    joff = np.array([11 * s for s in range(9)], np.uint64)
    rs = R.states([(tuple(int(x) for x in js[s]), (0, 0, 0), int(joff[s]), 0) for s in range(9)])
    n = len(data)
    cap = n + 256
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    prev = eng.to_device(np.frombuffer(prev_bytes, np.uint8), pad=0)
    out = eng.alloc(cap + SLACK)
    try:
        eng.scan(rx, n, segs)
        _fill(eng, out, cap + SLACK)
        eng.messages_joined(rx, n, True, out, cap, js, prev, 256, joff)
        jt = (out.download(cap + SLACK).tobytes(), eng.msg_bytes(), eng.message_table(), eng.segment_messages(9),
              eng.msg_state(9), eng.msg_carry(9))
        _fill(eng, out, cap + SLACK)
        eng.messages_rfc(rx, n, True, out, cap, rs, prev, 256)
        rt = (out.download(cap + SLACK).tobytes(), eng.msg_bytes(), eng.message_table(), eng.segment_messages(9),
              eng.rfc_state(9))
        assert rt[0] == jt[0] and rt[1] == jt[1]
        assert len(rt[2]) == len(jt[2]) > 50
        for f in ("off", "len", "total", "rec", "seg"):
            assert np.array_equal(rt[2][f], jt[2][f]), f
        # Q6 apart: nothing latched reports 0 here, 8 there (no frame of this batch has opcode 8)
        want_info = np.where(jt[2]["info"] & 0xF == 8, jt[2]["info"] & ~np.uint32(0xF), jt[2]["info"])
        assert np.array_equal(rt[2]["info"], want_info) and np.any(jt[2]["info"] & 0xF == 8)
        assert rt[3][0].tolist() == jt[3][0].tolist() and rt[3][1].tolist() == jt[3][1].tolist()
        assert rt[4]["data"].tolist() == jt[4].tolist()
        assert rt[4]["data_off"].tolist() == jt[5].tolist()
        assert not rt[4]["ctl"]["pending"].any() and not rt[4]["ctl_off"].any() and not rt[4]["ctl"]["opcode"].any()
    finally:
        rx.free()
        prev.free()
        out.free()
