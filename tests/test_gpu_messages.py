"""GPU: hvws_messages (include/hvws.h) -- the batch's payload bytes with the
headers squeezed out, the piece table, per-segment first / count and the
carried state, against the oracle in tests/wsmsg.py: after a scan (masked
bytes, buffer untouched) and after a step, the reference's quirks, around the
gather's tile and chunk edges, with a tight out_cap, over many segments with
carried state, over one stream cut into tiny batches, over a segment of many
scan blocks, after a RUN step and behind pipelined steps."""
from __future__ import annotations

import random

import numpy as np
import pytest

import libhv_amd
import streams
import wsharness as H
import wsmsg as M

pytestmark = pytest.mark.gpu

EINVAL = -2
PATH_RUN = 7
SENTINEL = 0xA5
SLACK = 64


class DeviceAt:
    """A batch at an address inside a DeviceBuffer."""

    def __init__(self, ptr: int):
        self.ptr = ptr


def _sentinel_out(eng, nbytes: int):
    out = eng.alloc(nbytes + SLACK)
    assert libhv_amd.lib().hvws_memset(eng.ctx, out.ptr, SENTINEL, nbytes + SLACK) == 0
    return out


def _pass(eng, data: bytes, segs, how: str, carry=None, state_in=None):
    """Upload, scan (how = 'scan': payloads stay masked) or step, hvws_messages
    with out_cap = rx_len.  -> (out bytes, pieces, (first, count), state_out,
    buffer afterwards); the bytes of d_out from the total on must be untouched."""
    rx = eng.to_device(np.frombuffer(data, dtype=np.uint8))
    out = _sentinel_out(eng, len(data))
    try:
        if how == "scan":
            eng.scan(rx, len(data), segs, carry)
        else:
            eng.step(rx, len(data), segs, carry)
        eng.messages(rx, len(data), how == "scan", out, len(data), state_in)
        total = eng.msg_bytes()
        table = eng.message_table()
        fc = eng.segment_messages(len(segs))
        st = eng.msg_state(len(segs))
        got = out.download(len(data) + SLACK)
        after = rx.download(len(data))
    finally:
        rx.free()
        out.free()
    assert total <= len(data)
    assert np.all(got[total:] == SENTINEL), "bytes at or beyond the payload total were written"
    return got[:total].tobytes(), table, fc, st, after.tobytes()


def _same(got, want, what=""):
    gout, gtab, (gfirst, gcount), gst = got[:4]
    wout, wtab, (wfirst, wcount), wst = want[:4]
    assert len(gout) == len(wout), what
    assert gout == wout, (what, next(i for i in range(len(wout)) if gout[i] != wout[i]))
    assert len(gtab) == len(wtab), what
    for f in wtab.dtype.names:
        assert np.array_equal(gtab[f], wtab[f]), (what, f)
    assert list(gfirst) == list(wfirst) and list(gcount) == list(wcount), what
    for f in wst.dtype.names:
        assert np.array_equal(gst[f], wst[f]), (what, f)


def _log(out: bytes, table):
    j = M.Joiner()
    j.feed(out, table)
    return j.msgs


@pytest.fixture(params=[0, 1], ids=["wide_tiles", "one_wave_tiles"])
def geometry(request, monkeypatch):
    """Both gather geometries, whatever the batch's mean record size would pick
    ($HVWS_EXPERIMENT msg, read at every call)."""
    monkeypatch.setenv("HVWS_EXPERIMENT", f"msg={request.param}")
    return request.param


def test_one_segment_masked_and_unmasked(eng, geometry):
    frames = streams.rand_frames(random.Random(11), 300, max_len=40)
    data = H.build_frames_ref(frames)
    segs = [(0, len(data))]
    recs = H.scan_segment(data)[0]
    assert 280 <= len(recs) <= 320 and int(recs["pay_len"].max()) <= 40
    assert int((recs["pay_len"] == 0).sum()) > 0
    assert any(not f[0] & M.MASK for f in frames) and any(not f[0] & M.FIN for f in frames)
    assert any(f[0] & 8 for f in frames)
    want = M.oracle_batch(data, segs)
    got1 = _pass(eng, data, segs, "scan")
    _same(got1, want, "masked")
    assert got1[4] == data   # the batch is only read
    got0 = _pass(eng, data, segs, "step")
    _same(got0, want, "unmasked")
    # the complete messages are what the message layer delivers (the stream may end inside one)
    log = H.run_messages("oracle", data, [len(data)])[0]
    ends = [p for p in got1[1] if int(p["info"]) & M.M_END]
    assert len(ends) == len(log) > 100
    assert _log(got1[0], got1[1]) == log


@pytest.mark.parametrize("name, want", [
    ("q5_control_between_fragments", [(9, b"ABPING"), (9, b"CD")]),
    ("q6_lone_continue", [(8, b"orphan")]),
    ("q7_zero_length", [(1, b""), (2, b""), (2, b"x")]),
    ("fragments", [(1, b"Hello!")]),
])
def test_quirks(eng, name, want):
    data = dict(streams.quirk_streams())[name]
    for how in ("scan", "step"):
        out, table, (first, count), st, _ = _pass(eng, data, [(0, len(data))], how)
        assert all(int(p["info"]) & M.M_END for p in table)
        assert [(int(p["info"]) & 0xF, out[int(p["off"]): int(p["off"]) + int(p["len"])]) for p in table] == want
        assert [int(p["len"]) for p in table] == [len(w[1]) for w in want]
        assert (int(first[0]), int(count[0])) == (0, len(want))
        assert (int(st["pending"][0]), int(st["open"][0])) == (0, 0)


def test_tile_and_chunk_edges(eng, geometry):
    """Record boundaries at every output offset around two multiples of the
    gather's largest tile (every geometry's divides it); the batch begins inside the first frame's header (an odd
    number of header bytes: odd source misalignments) or inside its payload (a
    carried-in frame at mask phases 1-3)."""
    tile = int(libhv_amd.lib().hvws_msg_tile())
    data = H.build_frames_ref(M.edge_frames(tile))
    assert len(data) < (1 << 20)
    misalign, phases, carried_phases, hdr_lens = set(), set(), set(), set()
    for cut in (0, 1, 3, 14 + 5, 14 + 6, 14 + 7):
        carry = H.scan_segment(data[:cut])[1] if cut else None
        batch = data[cut:]
        segs = [(0, len(batch))]
        want = M.oracle_batch(batch, segs, [carry] if carry is not None else None)
        recs = H.scan_segment(batch, carry)[0]
        out_off = np.concatenate([[0], np.cumsum(recs["pay_len"].astype(np.int64))])
        bounds = set(int(x) for x in out_off)
        if cut <= 3:
            for b in M.edge_bounds(tile):
                assert all(x in bounds for x in range(b - 17, b + 18)), (cut, b)
        for r, o in zip(recs, out_off):
            if int(r["pay_len"]) >= 16:
                misalign.add((int(r["pay_off"]) - int(o)) % 16)
            if int(r["info"]) & M.MASK and int(r["pay_len"]):
                phases.add((int(r["pay_off"]) - int(o)) % 4)
            if int(r["hdr_off"]) >= 0:
                hdr_lens.add(int(r["pay_off"]) - int(r["hdr_off"]))
        if cut > 14:
            assert int(recs[0]["hdr_off"]) == -1 and int(recs[0]["info"]) & M.MASK
            carried_phases.add((int(recs[0]["info"]) >> 8) & 3)
        for how in ("scan", "step"):
            got = _pass(eng, batch, segs, how, [carry] if carry is not None else None)
            _same(got, want, (cut, how))
            if how == "scan":
                assert got[4] == batch
    assert misalign == set(range(16))
    assert phases == {0, 1, 2, 3} and carried_phases == {1, 2, 3}
    assert hdr_lens == {2, 4, 6, 8, 10, 14}


def test_tight_out_cap(eng):
    L = libhv_amd.lib()
    data = H.build_frames_ref(streams.rand_frames(random.Random(4), 120, max_len=200))
    segs = [(0, len(data))]
    wout = M.oracle_batch(data, segs)[0]
    total = len(wout)
    assert total % 16 not in (0, 15) and total < len(data)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = _sentinel_out(eng, total)
    try:
        eng.scan(rx, len(data), segs)
        assert L.hvws_messages(eng.ctx, rx.ptr, len(data), 1, out.ptr, total - 1, None) == EINVAL
        assert np.all(out.download(total + SLACK) == SENTINEL)
        eng.messages(rx, len(data), True, out, total)
        assert eng.msg_bytes() == total
        got = out.download(total + SLACK)
        assert got[:total].tobytes() == wout
        assert np.all(got[total:] == SENTINEL)
    finally:
        rx.free()
        out.free()


def _two_batches(nseg: int):
    """Per segment one stream cut in two (inside headers and payloads) and
    short at the end; -> (batch 1, segs 1, batch 2, segs 2)."""
    rng = random.Random(64)
    p1, p2 = [], []
    for s in range(nseg):
        if s == 20:   # one frame, cut inside its payload: batch 2 holds a header-less body
            d = H.build_frames_ref([(0x22, bytes(range(60)), b"\x11\x22\x33\x44")])
            a, b = d[:6 + 13], d[6 + 13: 6 + 50]
        else:
            d = streams.rand_stream(rng, 6, max_len=60, edge=(s % 2 == 0))
            d = d[: len(d) - (7 * s) % 23]
            cut = len(d) if s == 10 else rng.randint(1, len(d) - 1)   # s == 10: an empty segment in batch 2
            a, b = d[:cut], d[cut:]
        p1.append(a)
        p2.append(b)

    def lay(parts):
        segs, at = [], 0
        for p in parts:
            segs.append((at, len(p)))
            at += len(p)
        return b"".join(parts), segs

    return lay(p1) + lay(p2)


def test_64_segments_with_carried_state(eng):
    d1, s1, d2, s2 = _two_batches(64)
    assert s2[10][1] == 0
    want1 = M.oracle_batch(d1, s1, with_carry=True)
    got1 = _pass(eng, d1, s1, "scan")
    _same(got1, want1, "batch 1")
    # the parser carries out of batch 1, from the device
    rx = eng.to_device(np.frombuffer(d1, np.uint8))
    eng.scan(rx, len(d1), s1)
    carries, _ = eng.carry(64)
    rx.free()
    # fresh / open with pending / latched but closed, whatever batch 1 left
    mix = [M.FRESH if s % 3 == 0 else (5 + s, 2, 1) if s % 3 == 1 else (0, 9, 0) for s in range(64)]
    for name, state_in in (("mixed", M.states(mix)), ("threaded", want1[3])):
        want2 = M.oracle_batch(d2, s2, want1[4], state_in)
        if name == "mixed":
            r20 = H.scan_segment(d2[s2[20][0]: s2[20][0] + s2[20][1]], want1[4][20])[0]
            assert len(r20) == 1 and int(r20[0]["hdr_off"]) == -1 and not int(r20[0]["info"]) & M.I_HDR
            assert int(want2[2][1][10]) == 0
            assert tuple(int(x) for x in want2[3][10]) == mix[10]   # no records: the state unchanged
            assert sum(1 for p in want2[1] if int(p["info"]) & M.M_CONT) >= 10
        for how in ("scan", "step"):
            _same(_pass(eng, d2, s2, how, carries, state_in), want2, (name, how))


def test_one_stream_in_tiny_batches(eng):
    """~200 frames cut into batches of 1-13 bytes; the parser carry and the
    message state ride along.  The joined pieces are the message log."""
    rng = random.Random(8)
    data = streams.rand_stream(rng, 200, max_len=10, edge=False)
    log = H.run_messages("oracle", data, [len(data)])[0]
    assert len(log) > 100
    j = M.Joiner()
    at, k, carry, st = 0, 0, None, M.states([M.FRESH])
    while at < len(data):
        n = min(rng.randint(1, 13), len(data) - at)
        k += 1
        out, table, _, st_out, _ = _pass(eng, data[at:at + n], [(0, n)], "scan" if k % 2 else "step", carry, st)
        cg, _ = eng.carry(1)
        # CONT exactly where the state said open: the batch's first piece, and only it
        for i, p in enumerate(table):
            assert bool(int(p["info"]) & M.M_CONT) == (i == 0 and int(st["open"][0]) == 1), (at, i)
        j.feed(out, table)
        carry, st = [cg[0]], st_out
        at += n
    assert j.msgs == log
    assert j.totals_ok   # every END piece's total is its message's length


def test_many_scan_blocks(eng, geometry):
    """70 000 records of 1-48 bytes in one segment (69 scan blocks, the last
    one short), then the same frames as 3 segments."""
    rng = random.Random(70)
    frames = []
    for i in range(70000):
        op = (1, 2, 0, 9)[i % 4] if i % 11 else 0xA
        fl = op | (M.FIN if rng.random() < 0.7 else 0) | (0 if i % 13 == 0 else M.MASK)
        frames.append((fl, rng.randbytes(rng.randint(1, 48)), rng.randbytes(4)))
    parts = [H.build_frames_ref(frames[a:b]) for a, b in ((0, 20011), (20011, 49999), (49999, 70000))]
    data = b"".join(parts)
    assert 1 << 20 < len(data) < 8 << 20
    offs = [0, len(parts[0]), len(parts[0]) + len(parts[1])]
    for segs in ([(0, len(data))], [(o, len(p)) for o, p in zip(offs, parts)]):
        want = M.oracle_batch(data, segs)
        assert int(want[2][1].sum()) == len(want[1]) > 40000
        _same(_pass(eng, data, segs, "scan"), want, len(segs))
    _same(_pass(eng, data, segs, "step"), want, "step")


def test_after_a_run_step(eng):
    """64 segments of equal 200-byte frames through the RUN path: its records
    are built for the pass."""
    L = libhv_amd.lib()
    r = random.Random(9)
    per_seg = 6
    frames = [(0x31 if i % 5 else 0x21, r.randbytes(200), r.randbytes(4)) for i in range(64 * per_seg)]
    data = H.build_frames_ref(frames)
    size = len(data) // len(frames)
    assert size == 208
    segs = [(s * per_seg * size, per_seg * size) for s in range(64)]
    want = M.oracle_batch(data, segs)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = _sentinel_out(eng, len(data))
    old_bound = L.hvws_set_fast_bound(eng.ctx, 1)
    old_run = L.hvws_set_run(eng.ctx, 1)
    try:
        eng.step(rx, len(data), segs)
        assert L.hvws_last_scan_path(eng.ctx) == PATH_RUN
        eng.messages(rx, len(data), False, out, len(data))
        total = eng.msg_bytes()
        got = (out.download(total).tobytes(), eng.message_table(), eng.segment_messages(64), eng.msg_state(64))
    finally:
        L.hvws_set_run(eng.ctx, old_run)
        L.hvws_set_fast_bound(eng.ctx, old_bound)
        rx.free()
        out.free()
    _same(got, want)


def test_pass_queued_behind_pipelined_steps(eng):
    """Pipelined steps A, B, C on alternating buffers; the pass over A is held
    back 20 ms on the context stream, so it is still queued when C's scan wants
    the table set A's records live in.  A's messages must be A's."""
    L = libhv_amd.lib()
    batches = [H.build_frames_ref(streams.rand_frames(random.Random(seed), nf, max_len=80))
               for seed, nf in ((31, 90), (32, 50), (33, 130))]
    segs = [[(0, len(d) // 2), (len(d) // 2, len(d) - len(d) // 2)] for d in batches]
    want = M.oracle_batch(batches[0], segs[0])
    assert len(want[1]) != len(M.oracle_batch(batches[2], segs[2])[1])
    rx = [eng.to_device(np.frombuffer(d, np.uint8)) for d in batches]
    out = _sentinel_out(eng, len(batches[0]))
    try:
        eng.step_resident(rx[0], len(batches[0]), segs[0])
        assert L.hvws_debug_stall(eng.ctx, 20000) == 0
        eng.messages(rx[0], len(batches[0]), False, out, len(batches[0]))
        eng.step_resident(rx[1], len(batches[1]), segs[1])
        eng.step_resident(rx[2], len(batches[2]), segs[2])
        total = eng.msg_bytes()
        got = (out.download(total).tobytes(), eng.message_table(), eng.segment_messages(2), eng.msg_state(2))
        assert eng.last_kernel_ms() > 0
    finally:
        eng.sync()
        for b in rx:
            b.free()
        out.free()
    _same(got, want)


def test_errors():
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as e:
        data = H.build_frames_ref(streams.rand_frames(random.Random(2), 20, max_len=50))
        n = len(data)
        rx = e.to_device(np.frombuffer(data, np.uint8))
        other = e.alloc(n + 64)
        both = e.alloc(2 * n + 64)   # a batch and an output that runs into it
        out = _sentinel_out(e, n)

        def untouched():
            return bool(np.all(out.download(n + SLACK) == SENTINEL))

        assert L.hvws_messages(e.ctx, rx.ptr, n, 1, out.ptr, n, None) == EINVAL       # no scan yet
        assert L.hvws_msg_count(e.ctx) == -1 and not L.hvws_messages_device(e.ctx)
        e.scan(rx, n, [(0, n)])
        assert L.hvws_messages(e.ctx, other.ptr, n, 1, out.ptr, n, None) == EINVAL    # another buffer
        assert L.hvws_messages(e.ctx, rx.ptr, n - 1, 1, out.ptr, n, None) == EINVAL   # another length
        assert L.hvws_messages(e.ctx, rx.ptr, n, 1, out.ptr + 8, n, None) == EINVAL   # misaligned d_out
        for st in ((1, 1, 0), (0, 16, 0)):   # open = 0 with pending = 1; opcode 16
            s = M.states([st])
            assert L.hvws_messages(e.ctx, rx.ptr, n, 1, out.ptr, n, s.ctypes.data) == EINVAL, st
        assert untouched()
        # d_out overlapping the batch: beginning inside it, or ending inside it
        both.upload(np.frombuffer(data, np.uint8))
        e.scan(both, n, [(0, n)])
        assert L.hvws_messages(e.ctx, both.ptr, n, 1, both.ptr + (n // 2 & ~15), n, None) == EINVAL
        hi = both.ptr + ((n + 15) & ~15)
        assert L.hvws_messages(e.ctx, both.ptr, n, 1, hi, n, None) == 0               # adjacent is fine
        assert np.array_equal(both.download(n), np.frombuffer(data, np.uint8))
        e.sync()
        assert L.hvws_d2d(e.ctx, hi, both.ptr, n) == 0
        e.sync()
        e.scan(DeviceAt(hi), n, [(0, n)])
        assert L.hvws_messages(e.ctx, hi, n, 1, both.ptr, n + 32, None) == EINVAL     # runs into the batch from below
        assert L.hvws_messages(e.ctx, hi, n, 1, both.ptr, 16, None) == EINVAL         # too small, after the wait
        for b in (rx, other, both, out):
            b.free()


def test_getters(eng):
    L = libhv_amd.lib()
    data = H.build_frames_ref(streams.rand_frames(random.Random(3), 60, max_len=30))
    n = len(data)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = eng.alloc(n + 64)
    try:
        eng.scan(rx, n, [(0, n)])
        eng.messages(rx, n, True, out, n)
        cnt = L.hvws_msg_count(eng.ctx)
        want = M.oracle_batch(data, [(0, n)])[1]
        assert cnt == len(want) > 10
        buf = np.zeros(4, libhv_amd.MSG_DTYPE)
        assert L.hvws_get_messages(eng.ctx, buf.ctypes.data, cnt - 1, 2) == EINVAL
        assert L.hvws_get_messages(eng.ctx, buf.ctypes.data, cnt + 1, 0) == EINVAL
        assert L.hvws_get_messages(eng.ctx, buf.ctypes.data, cnt - 1, 1) == 0
        assert tuple(buf[0]) == tuple(want[-1])
        dev = L.hvws_messages_device(eng.ctx)
        assert dev
        raw = np.zeros(cnt, libhv_amd.MSG_DTYPE)
        assert L.hvws_d2h(eng.ctx, raw.ctypes.data, dev, raw.nbytes) == 0
        eng.sync()
        assert np.array_equal(raw, eng.message_table())
    finally:
        rx.free()
        out.free()
