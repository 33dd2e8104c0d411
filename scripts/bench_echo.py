#!/usr/bin/env python3
"""Echo turn measurement: hvws_send_messages against hvws_build_frames on the
same frames, and the whole server turn against the receive side alone.

Two shapes on one card, device resident, 4096 segments of masked FIN binary
frames:
  * "c3": 1M x 64 KiB frames (BASELINE config 3's shape);
  * "c2": 1M x 1 KiB frames (config 2's shape).
Each batch is scanned, reassembled (hvws_messages, masked = 1), answered
(hvws_replies, SERVER | ECHO) and echoed unmasked with fragment = 0, the reply
table and its count read on the device.  At c3 every 65 536-byte message goes
out as two frames (65 535 + 1), exactly as the reference fragments it.  Per
shape, from one process:
  1. the send's device time after its wait (hvws_last_kernel_ms: expansion,
     tile index, spans, k_build);
  2. hvws_build_frames' device time (its own hvws_last_kernel_ms: tile index,
     spans, k_build) for the same frames from tables prepared on the host --
     the yardstick; the two alternate, with the spread of both;
  3. the send's message pass and wait: the device span of the whole call minus
     (1) (the host's round trip for the wait is inside it);
  4. the device span of the whole turn (scan + messages + replies + send)
     against scan + messages alone;
  5. the first and last MiB of the output against frames rebuilt on the CPU
     from the downloaded ends of the payload -- at c3 the only check of offsets
     beyond 4 GiB: the test suite stays in the single-digit MB range.

FRAMES_C3 / FRAMES_C2 shrink the shapes; REPS sets the repetitions.  Prints
JSON lines.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import libhv_amd  # noqa: E402
from libhv_amd import synth  # noqa: E402

NSEG = 4096
MIB = 1 << 20
FRAGMENT = 0xFFFF   # what fragment = 0 means (reference http/WebSocketChannel.cpp:6)
FIN = 0x10


def fetch(eng, buf, off, n):
    out = np.empty(n, np.uint8)
    libhv_amd._check(libhv_amd.lib().hvws_d2h(eng.ctx, out.ctypes.data, buf.ptr + off, n), "hvws_d2h")
    eng.sync()
    return out


def span(eng, fn):
    L = libhv_amd.lib()
    ms = ctypes.c_float(0)
    eng.sync()   # the span's begin markers go on both compute streams: nothing may still run on either
    libhv_amd._check(L.hvws_span_begin(eng.ctx), "span_begin")
    fn()
    libhv_amd._check(L.hvws_span_end(eng.ctx, ctypes.byref(ms)), "span_end")
    return float(ms.value)


def header(flags: int, n: int) -> bytes:
    """An unmasked frame header (reference http/websocket_parser.c:215-246)."""
    b0 = (0x80 if flags & FIN else 0) | (flags & 0xF)
    if n < 126:
        return bytes([b0, n])
    if n <= 0xFFFF:
        return bytes([b0, 126]) + n.to_bytes(2, "big")
    return bytes([b0, 127]) + n.to_bytes(8, "big")


def echo_cpu(payload: np.ndarray, size: int, op: int) -> bytes:
    """The echo of consecutive messages of `size` bytes, fragmented as the
    reference's send does (http/WebSocketChannel.cpp:24-48), built on the CPU."""
    out = bytearray()
    for m in payload.reshape(-1, size):
        if size <= FRAGMENT:
            out += header(op | FIN, size) + m.tobytes()
            continue
        at, first = 0, True
        while size - at > FRAGMENT:
            out += header(op if first else 0, FRAGMENT) + m[at:at + FRAGMENT].tobytes()
            at, first = at + FRAGMENT, False
        out += header(FIN, size - at) + m[at:].tobytes()
    return bytes(out)


def frame_tables(n: int, size: int, op: int):
    """Host tables of the same frames for hvws_build_frames."""
    per = 1 if size <= FRAGMENT else -(-size // FRAGMENT)
    base = np.repeat(np.arange(n, dtype=np.uint64) * np.uint64(size), per)
    j = np.tile(np.arange(per, dtype=np.uint64), n)
    length = np.where(j + 1 < per, FRAGMENT, size - (per - 1) * FRAGMENT).astype(np.uint64)
    flags = (np.where(j == 0, op, 0) | np.where(j + 1 == per, FIN, 0)).astype(np.uint8)
    return base + j * np.uint64(FRAGMENT), length, flags


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    msg = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    op = int(p.flags[0]) & 0xF
    assert op in (1, 2) and bool((p.flags & FIN).all()), "the shapes are FIN data frames"
    pay_bytes = p.n * payload
    per = 1 if payload <= FRAGMENT else -(-payload // FRAGMENT)
    msg_out = len(echo_cpu(np.zeros(payload, np.uint8), payload, op))
    want_len, want_frames = p.n * msg_out, p.n * per
    out = eng.alloc(want_len + 64)   # both builders write it in turn (c3: a second one would not fit the card)
    tx = libhv_amd.TxPlan(eng, *frame_tables(p.n, payload, op))
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)

    def receive():
        eng.scan(rx, p.total, p.segments)
        eng.messages(rx, p.total, True, msg, p.total)

    def send():
        table, d_n, n = eng.replies_device()
        return eng.send_messages(out, want_len + 64, msg, p.total, table, n, d_n, 0, False)

    receive()
    eng.replies(policy)
    assert L.hvws_reply_count(eng.ctx) == p.n, "one echo per frame"
    assert not eng.reply_flags(len(p.segments)).any(), "no segment closed or deferred"
    post, build, whole = [], [], []
    for _ in range(reps + 1):
        whole.append(span(eng, lambda: send()))
        post.append(eng.last_kernel_ms())
        assert eng.build_frames(out, want_len + 64, msg, p.total, tx) == want_len
        build.append(eng.last_kernel_ms())
    # the ends of both outputs against the CPU's frames from the payload's ends
    k = min(p.n, -(-MIB // msg_out) + 1)
    n = min(MIB, want_len)
    head = echo_cpu(fetch(eng, msg, 0, k * payload), payload, op)[:n]
    tail = echo_cpu(fetch(eng, msg, pay_bytes - k * payload, k * payload), payload, op)[-n:]

    def check_ends(what):
        assert fetch(eng, out, 0, n).tobytes() == head, f"{name}: first MiB of the {what} output"
        assert fetch(eng, out, want_len - n, n).tobytes() == tail, f"{name}: last MiB of the {what} output"

    kern, uni = L.hvws_last_build_kernel(eng.ctx).decode(), L.hvws_last_build_uniform(eng.ctx)
    check_ends("build_frames")
    libhv_amd._check(L.hvws_memset(eng.ctx, out.ptr, 0, n), "hvws_memset")   # the send must write both ends anew
    libhv_amd._check(L.hvws_memset(eng.ctx, out.ptr + want_len - n, 0, n), "hvws_memset")
    assert send() == (want_len, want_frames)
    kern_s, uni_s = L.hvws_last_build_kernel(eng.ctx).decode(), L.hvws_last_build_uniform(eng.ctx)
    check_ends("send")
    # the turn against the receive side alone
    t_rx, t_turn = [], []
    for _ in range(reps + 1):
        t_rx.append(span(eng, receive))
        t_turn.append(span(eng, lambda: (receive(), eng.replies(policy), send())))
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    pre = [w - q for w, q in zip(whole, post)]
    row = {
        "bench": "echo", "shape": name, "messages": p.n, "payload": payload, "segments": len(p.segments),
        "frames": want_frames, "out_bytes": want_len, "reps": reps,
        "send_post_wait_ms": round(med(post), 4), "send_post_wait_range": rng(post),
        "build_frames_ms": round(med(build), 4), "build_frames_range": rng(build),
        "ratio_send_to_build": round(med(post) / med(build), 4),
        "send_GBps": round(2 * pay_bytes / med(post) / 1e6, 1),
        "send_call_span_ms": round(med(whole), 4), "send_pre_wait_ms": round(med(pre), 4),
        "span_receive_ms": round(med(t_rx), 4), "span_turn_ms": round(med(t_turn), 4),
        "kernel_send": kern_s, "uniform_send": uni_s, "kernel_build": kern, "uniform_build": uni,
        "checked": "reply and frame counts; first and last MiB of both outputs against frames rebuilt on the CPU"
                   + (" (the only check of offsets beyond 4 GiB)" if want_len > 4 << 30 else ""),
    }
    print(json.dumps(row), flush=True)
    for b in (rx, msg, out):
        b.free()
    tx.free()
    dp.free()


def main():
    reps = int(os.environ.get("REPS", "7"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 20)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    if n3:
        shape(eng, "c3", n3, 65536, reps)
    if n2:
        shape(eng, "c2", n2, 1024, reps)
    eng.close()


if __name__ == "__main__":
    main()
