"""GPU: hvws_send_messages against the reference's WebSocketChannel::send
(http/WebSocketChannel.cpp:5-48) as tests/wssend.py plans it and the
reference's websocket_build_frame builds it, byte for byte: length and
fragment edges, scan block edges, skewed work, zero-length and broadcast
batches, d_msg_off / out_len / out_frames, the device-side count, every
rejection (nothing written), a device round trip through scan and
hvws_messages, and hvws_build_frames undisturbed around a send."""
from __future__ import annotations

import random

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wssend as S
from test_gpu_tx import _frames, _gpu_build

pytestmark = pytest.mark.gpu

FIN = S.FIN
CANARY = 0xA5


def _table(msgs, offs):
    t = np.zeros(len(msgs), dtype=libhv_amd.TX_MSG_DTYPE)
    for i, (fl, data, key) in enumerate(msgs):
        t[i] = (offs[i], len(data), fl, key)
    return t


def _layout(msgs, gap_rng=None):
    """Payloads back to back, or behind random gaps of 0-18 bytes (misaligned)."""
    pay, offs = bytearray(), []
    for _, data, _ in msgs:
        if gap_rng is not None:
            pay += bytes(gap_rng.randrange(19))
        offs.append(len(pay))
        pay += data
    return bytes(pay), offs


def _send(eng, table, pay: bytes, n=None, fragment=0, masked=False, d_n=None, out_cap=None, want_len=0):
    """Send `table` over `pay`; returns (bytes out incl. 64 canary bytes beyond
    out_len, msg_off, out_len, frames).  The output starts all canary."""
    n = len(table) if n is None else n
    cap = want_len + 64 if out_cap is None else out_cap
    payload = eng.to_device(np.frombuffer(pay, dtype=np.uint8)) if pay else eng.alloc(16)
    dt = eng.to_device(table.view(np.uint8)) if len(table) else eng.alloc(32)
    out = eng.alloc(max(cap, want_len) + 64)
    moff = eng.alloc(8 * (n + 1))
    dn = eng.to_device(np.array([d_n], dtype=np.uint64)) if d_n is not None else None
    try:
        L = libhv_amd.lib()
        L.hvws_memset(eng.ctx, out.ptr, CANARY, out.nbytes)
        L.hvws_memset(eng.ctx, moff.ptr, CANARY, moff.nbytes)
        nbytes, nfr = eng.send_messages(out, cap, payload, len(pay), dt, n, dn, fragment, masked, moff)
        got = bytes(out.download(nbytes + 64))
        eff = n if d_n is None else min(n, d_n)
        offs = moff.download(8 * (eff + 1), np.uint64).tolist()
    finally:
        for b in (payload, dt, out, moff, dn):
            if b is not None:
                b.free()
    return got, offs, nbytes, nfr


def _check(eng, msgs, fragment=0, masked=False, gap_rng=None, **kw):
    want, woffs, wfr = S.expected(msgs, fragment, masked)
    pay, offs = _layout(msgs, gap_rng)
    got, goffs, nbytes, nfr = _send(eng, _table(msgs, offs), pay, fragment=fragment, masked=masked,
                                    want_len=len(want), **kw)
    assert (nbytes, nfr) == (len(want), wfr)
    assert goffs == woffs
    assert got[:nbytes] == want
    assert got[nbytes:] == bytes([CANARY]) * 64    # nothing beyond out_len is written


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("F", [1, 2, 7, 125, 126, 127, 65535, 65536])
def test_length_and_fragment_edges(eng, F, masked):
    rng = random.Random(F + masked)
    msgs = []
    for L in [0, 1, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1]:
        for fin in (0, FIN):   # send()'s fin: honoured on single frames, dropped on fragmented ones
            msgs.append((rng.choice([1, 2, 9, 10, 8, 0]) | fin, rng.randbytes(L), rng.getrandbits(32)))
    _check(eng, msgs, F, masked, gap_rng=rng)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_scan_block_edges(eng, n):
    rng = random.Random(n)
    msgs = [(rng.choice([1, 2]) | FIN, rng.randbytes(rng.randrange(41)), rng.getrandbits(32)) for _ in range(n)]
    _check(eng, msgs, 16, masked=bool(n & 1), gap_rng=rng)


@pytest.mark.parametrize("F,big", [(7, 300000), (0, 3 * 65536 + 5), (65536, 3 * 65536 + 5)])
def test_skewed_work(eng, F, big):
    """One long message between 500 one-frame messages on each side: the
    frame-to-message lookups cross many workgroup boundaries."""
    rng = random.Random(big + F)
    small = lambda: (2 | FIN, rng.randbytes(rng.randrange(1, 7)), rng.getrandbits(32))
    msgs = [small() for _ in range(500)] + [(1 | FIN, rng.randbytes(big), 7)] + [small() for _ in range(500)]
    if F == 7:
        assert S.closed_form(big, F, False) == (42858, 385716)
    _check(eng, msgs, F, masked=False)
    _check(eng, msgs, F, masked=True)


def test_zero_length_messages_only(eng):
    msgs = [((1, 2, 9, 8)[i % 4] | (FIN if i % 3 else 0), b"", i) for i in range(3000)]
    _check(eng, msgs, 0, masked=False)
    _check(eng, msgs, 5, masked=True)


def test_broadcast_one_shared_payload(eng):
    rng = random.Random(4)
    body = rng.randbytes(1000)
    msgs = [(2 | FIN, body, rng.getrandbits(32)) for _ in range(2000)]
    table = _table(msgs, [3] * len(msgs))
    pay = b"abc" + body
    for F, masked in ((0, False), (0, True), (300, True)):
        want, woffs, wfr = S.expected(msgs, F, masked)
        got, goffs, nbytes, nfr = _send(eng, table, pay, fragment=F, masked=masked, want_len=len(want))
        assert (nbytes, nfr, goffs) == (len(want), wfr, woffs)
        assert got[:nbytes] == want


def test_uniform_layout_is_found_and_equal(eng, monkeypatch):
    """1 KiB messages at a constant step, one frame each: k_build's index-free
    uniform form; the same bytes as with the index (a step of 0)."""
    monkeypatch.delenv("HVWS_EXPERIMENT", raising=False)
    rng = random.Random(8)
    msgs = [(2 | FIN, rng.randbytes(1024), rng.getrandbits(32)) for _ in range(600)]
    _check(eng, msgs, 0, masked=True)
    assert libhv_amd.lib().hvws_last_build_uniform(eng.ctx) == 1
    assert libhv_amd.lib().hvws_last_build_kernel(eng.ctx).decode().endswith(",lean>")
    _check(eng, msgs, 1000, masked=True)   # two frames each: not uniform
    assert libhv_amd.lib().hvws_last_build_uniform(eng.ctx) == 0
    assert eng.last_kernel_ms() >= 0.0


@pytest.mark.parametrize("d_n,n", [(5, 40), (0, 40), (40, 40), (1000, 40)])
def test_device_count(eng, d_n, n):
    """d_n smaller than n: only the first *d_n messages go out and the byte
    after out_len keeps its canary; larger: clamped to n."""
    rng = random.Random(d_n)
    msgs = [(2 | FIN, rng.randbytes(rng.randrange(300)), rng.getrandbits(32)) for _ in range(n)]
    eff = min(d_n, n)
    want, woffs, wfr = S.expected(msgs[:eff], 100, True)
    pay, offs = _layout(msgs, rng)
    got, goffs, nbytes, nfr = _send(eng, _table(msgs, offs), pay, fragment=100, masked=True, d_n=d_n,
                                    want_len=len(S.expected(msgs, 100, True)[0]))
    assert (nbytes, nfr, goffs) == (len(want), wfr, woffs)
    assert got[:nbytes] == want and got[nbytes:] == bytes([CANARY]) * 64


def test_empty_batch(eng):
    out = eng.alloc(64)
    try:
        assert eng.send_messages(out, 64, None, 0, None, 0) == (0, 0)
    finally:
        out.free()


def _rejected(eng, table, pay, match, out_cap=4096, **kw):
    """The call fails with HVWS_EINVAL and d_out stays all canary."""
    payload = eng.to_device(np.frombuffer(pay, dtype=np.uint8))
    dt = eng.to_device(table.view(np.uint8))
    out = eng.alloc(out_cap + 64)
    try:
        libhv_amd.lib().hvws_memset(eng.ctx, out.ptr, CANARY, out.nbytes)
        with pytest.raises(libhv_amd.HvwsError, match=match) as ei:
            eng.send_messages(out, out_cap, payload, len(pay), dt, len(table), **kw)
        assert "(-2)" in str(ei.value)
        assert bytes(out.download(out.nbytes)) == bytes([CANARY]) * out.nbytes
    finally:
        for b in (payload, dt, out):
            b.free()


def test_rejections_write_nothing(eng):
    pay = bytes(range(256)) * 4
    ok = (2 | FIN, pay[:100], 1)
    _rejected(eng, _table([ok, (2 | FIN, pay[:100], 1), ok], [0, 1000, 0]), pay, "outside")      # range past the end
    _rejected(eng, _table([ok, ok], [0, 1025]), pay, "outside")                                 # offset past the end
    _rejected(eng, _table([ok, (2 | FIN | 0x20, pay[:10], 1)], [0, 0]), pay, "flag bit")         # a flag bit 0x20
    table = _table([ok] * 5, [0] * 5)
    want = len(S.expected([ok] * 5)[0])
    _rejected(eng, table, pay, "capacity", out_cap=want - 1)                                    # one byte short
    assert eng.last_send_len == want                                                            # *out_len still set
    got, _, nbytes, _ = _send(eng, table, pay, out_cap=want, want_len=want)                     # exact capacity fits
    assert nbytes == want and got[:want] == S.expected([ok] * 5)[0]


def test_rejects_too_many_frames(eng):
    """70 000 messages of 65 535 bytes at F = 1: more than 2^32 - 2 frames."""
    pay = bytes(65535)
    table = np.zeros(70000, dtype=libhv_amd.TX_MSG_DTYPE)
    table["len"] = 65535
    table["flags"] = 2 | FIN
    _rejected(eng, table, pay, "frames", fragment=1)


def test_rejects_overlap_and_misalignment(eng):
    buf = eng.alloc(8192)
    dt = eng.to_device(_table([(2 | FIN, bytes(10), 0)], [0]).view(np.uint8))
    try:
        libhv_amd.lib().hvws_memset(eng.ctx, buf.ptr, CANARY, buf.nbytes)
        with pytest.raises(libhv_amd.HvwsError, match="overlaps"):
            eng.send_messages(buf.ptr + 1024, 4096, buf.ptr, 2048, dt, 1)
        with pytest.raises(libhv_amd.HvwsError, match="aligned"):
            eng.send_messages(buf.ptr + 4097, 1024, buf.ptr, 2048, dt, 1)
        assert bytes(buf.download(buf.nbytes)) == bytes([CANARY]) * buf.nbytes
    finally:
        buf.free()
        dt.free()


@pytest.mark.parametrize("nseg", [1, 16])
@pytest.mark.parametrize("F", [3, 126, 0])
def test_round_trip_on_the_device(eng, F, nseg):
    """Random messages sent masked, scanned in segments cut at message
    boundaries, reassembled by hvws_messages(masked = 1): the pieces reproduce
    the opcodes and bytes."""
    rng = random.Random(F * 31 + nseg)
    top = 400 if F else 70000
    msgs = [(rng.choice([1, 2]) | FIN, rng.randbytes(rng.choice([0, 1, rng.randrange(top), rng.randrange(40)])),
             rng.getrandbits(32)) for _ in range(48)]
    if F == 0:
        msgs[5] = (2 | FIN, rng.randbytes(65536 + 9), 77)
    want, woffs, _ = S.expected(msgs, F, True)
    pay, offs = _layout(msgs, rng)
    payload = eng.to_device(np.frombuffer(pay, dtype=np.uint8))
    dt = eng.to_device(_table(msgs, offs).view(np.uint8))
    wire = eng.alloc(len(want) + 64)
    back = eng.alloc(len(want) + 64)
    try:
        nbytes, _ = eng.send_messages(wire, len(want) + 64, payload, len(pay), dt, len(msgs), None, F, True)
        assert nbytes == len(want)
        per = len(msgs) // nseg
        cuts = [woffs[i * per] for i in range(nseg)] + [nbytes]
        segs = [(cuts[i], cuts[i + 1] - cuts[i]) for i in range(nseg)]
        eng.scan(wire, nbytes, segs)
        eng.messages(wire, nbytes, True, back, nbytes)
        pieces = eng.message_table()
        out = bytes(back.download(eng.msg_bytes()))
        assert len(pieces) == len(msgs)
        assert all(int(p["info"]) & libhv_amd.MSG_END for p in pieces)
        got = [(int(p["info"]) & 0xF, out[int(p["off"]):int(p["off"]) + int(p["len"])]) for p in pieces]
        assert got == [(fl & 0xF, d) for fl, d, _ in msgs]
    finally:
        for b in (payload, dt, wire, back):
            b.free()


def test_build_frames_undisturbed_around_a_send(eng):
    """hvws_build_frames shares the send's post-wait half and some tables: a
    plan built before and after a send still gives the reference's bytes."""
    rng = np.random.default_rng(17)
    frames = _frames(rng, 300)
    want = H.build_frames_ref(frames)
    assert _gpu_build(eng, frames, gap_rng=rng)[0] == want
    r = random.Random(3)
    _check(eng, [(2 | FIN, r.randbytes(r.randrange(5000)), r.getrandbits(32)) for _ in range(100)], 700, True, gap_rng=r)
    got, off = _gpu_build(eng, frames, gap_rng=rng, with_off=True)
    assert got == want
    sizes = [len(H.build_frames_ref([f])) for f in frames]
    assert off.tolist() == list(np.cumsum([0] + sizes[:-1]))
