#!/usr/bin/env python3
"""Fan-out turn measurement: hvws_fanout beside hvws_replies, the send from the
fanout table beside hvws_build_frames on the identical frames, and the whole
fan-out against the echo turn of scripts/bench_echo.py scaled by output bytes.

Two shapes on one card, device resident, 4096 connections (one segment each) of
masked FIN binary frames, in rooms of 16: connection s publishes to room
s // 16 and subscribes to it, HVWS_FAN_SELF set, so every message is delivered
16 times:
  * "c3": 64 KiB frames (BASELINE config 3's frame; FRAMES_C3 of them -- the
    output is 16 times the batch, so the batch is smaller than bench_echo's);
  * "c2": 1 KiB frames (config 2's frame; FRAMES_C2 of them).
Each batch is scanned, reassembled (hvws_messages, masked = 1) and answered
(hvws_replies, SERVER | ECHO).  Per shape, from one process:
  a. hvws_replies' device span and hvws_fanout's: the device span of the whole
     call (the host's round trip for its one wait is inside it) and the device
     time after the wait (hvws_last_kernel_ms: expansion, sort, finish);
  b. the send from the fanout table, device time after its wait, against
     hvws_build_frames (its own hvws_last_kernel_ms) on the identical frames
     from tables made on the host; the two alternate, with the spread of both;
  c. (a) + (b) against the echo turn (hvws_replies + the send from the reply
     table, measured here on the same batch) scaled by the output bytes.
Checks: the delivery table's reply[] against the order computed on the host from
the reply call's per-segment ranges (room by room), first / count, and the
digest of the send's output against the digest of hvws_build_frames' output.

REPS sets the repetitions.  Prints JSON lines.
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
ROOM = 16
FRAGMENT = 0xFFFF
FIN = 0x10


def span(eng, fn):
    L = libhv_amd.lib()
    ms = ctypes.c_float(0)
    eng.sync()
    libhv_amd._check(L.hvws_span_begin(eng.ctx), "span_begin")
    fn()
    libhv_amd._check(L.hvws_span_end(eng.ctx, ctypes.byref(ms)), "span_end")
    return float(ms.value)


def hdr_len(n: int) -> int:
    return 2 + (0 if n < 126 else (2 if n <= 0xFFFF else 8))


def frame_tables(off: np.ndarray, size: int, op: int):
    """Host tables for hvws_build_frames: the frames of messages of `size` bytes at `off`."""
    per = 1 if size <= FRAGMENT else -(-size // FRAGMENT)
    base = np.repeat(off.astype(np.uint64), per)
    j = np.tile(np.arange(per, dtype=np.uint64), len(off))
    length = np.where(j + 1 < per, FRAGMENT, size - (per - 1) * FRAGMENT).astype(np.uint64)
    flags = (np.where(j == 0, op, 0) | np.where(j + 1 == per, FIN, 0)).astype(np.uint8)
    return base + j * np.uint64(FRAGMENT), length, flags


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    nseg = len(p.segments)
    assert nseg % ROOM == 0
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    msg = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    op = int(p.flags[0]) & 0xF
    assert op in (1, 2) and bool((p.flags & FIN).all()), "the shapes are FIN data frames"
    per = 1 if payload <= FRAGMENT else -(-payload // FRAGMENT)
    last = payload - (per - 1) * FRAGMENT
    msg_out = (per - 1) * (hdr_len(FRAGMENT) + FRAGMENT) + hdr_len(last) + last
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.messages(rx, p.total, True, msg, p.total)
    eng.replies(policy)
    assert L.hvws_reply_count(eng.ctx) == p.n, "one echo per frame"
    # the subscription table: rooms of 16 connections
    topic_first = np.arange(nseg // ROOM + 1, dtype=np.uint64) * ROOM
    member = np.arange(nseg, dtype=np.uint32)
    d_first, d_member = eng.to_device(topic_first), eng.to_device(member)
    pub = (np.arange(nseg) // ROOM).astype(np.uint32)
    dest_of = np.arange(nseg, dtype=np.uint32)

    def fanout():
        return eng.fanout(d_first, d_member, nseg // ROOM, nseg, nseg, pub, dest_of, libhv_amd.FAN_SELF)

    ndel = fanout()
    assert ndel == p.n * ROOM
    # the same order on the host: destination d takes its room's replies, which are contiguous
    rfirst, rcount = eng.segment_replies(nseg)
    lo = rfirst[::ROOM].astype(np.int64)
    hi = (rfirst[ROOM - 1::ROOM] + rcount[ROOM - 1::ROOM]).astype(np.int64)
    room_n = hi - lo
    dest_n = np.repeat(room_n, ROOM)
    want_first = np.concatenate(([0], np.cumsum(dest_n)[:-1]))
    want_reply = np.repeat(np.repeat(lo, ROOM) - want_first, dest_n) + np.arange(ndel, dtype=np.int64)
    table, reply = eng.fanout_table()
    first, count = eng.dest_fanout(nseg)
    assert np.array_equal(reply.astype(np.int64), want_reply), "reply[] differs from the order computed on the host"
    assert np.array_equal(first.astype(np.int64), want_first) and np.array_equal(count.astype(np.int64), dest_n)
    rep_table, _ = eng.reply_table()
    assert np.array_equal(table, rep_table[want_reply]), "the delivery table is not the reply rows"
    want_len, want_frames = ndel * msg_out, ndel * per
    out = eng.alloc(want_len + 64)
    tx = libhv_amd.TxPlan(eng, *frame_tables(table["off"], payload, op))
    del table, reply, rep_table, want_reply

    def send_fan():
        t, d_n, n = eng.fanout_device()
        return eng.send_messages(out, want_len + 64, msg, p.total, t, n, d_n, 0, False)

    def send_echo():
        t, d_n, n = eng.replies_device()
        return eng.send_messages(out, want_len + 64, msg, p.total, t, n, d_n, 0, False)

    t_rep, fan_span, fan_post, send_post, build, echo_post = [], [], [], [], [], []
    digests = set()
    for k in range(reps + 1):
        t_rep.append(span(eng, lambda: eng.replies(policy)))
        echo = send_echo()
        echo_post.append(eng.last_kernel_ms())
        assert echo == (p.n * msg_out, p.n * per)
        fan_span.append(span(eng, fanout))
        fan_post.append(eng.last_kernel_ms())
        assert send_fan() == (want_len, want_frames)
        send_post.append(eng.last_kernel_ms())
        kern = L.hvws_last_build_kernel(eng.ctx).decode()
        if k == 0:
            digests.add(eng.digest(out, want_len))
            libhv_amd._check(L.hvws_memset(eng.ctx, out.ptr, 0, min(want_len, 1 << 20)), "hvws_memset")
        assert eng.build_frames(out, want_len + 64, msg, p.total, tx) == want_len
        build.append(eng.last_kernel_ms())
        if k == 0:
            digests.add(eng.digest(out, want_len))
    assert len(digests) == 1, f"{name}: the send from the fanout table and hvws_build_frames wrote different bytes"
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    scale = want_len / (p.n * msg_out)
    fan_turn = med(fan_span) + med(send_post)
    echo_turn = med(t_rep) + med(echo_post)
    row = {
        "bench": "fanout", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "room": ROOM,
        "deliveries": ndel, "frames": want_frames, "out_bytes": want_len, "sort_passes": 2, "reps": reps,
        "replies_span_ms": round(med(t_rep), 4), "replies_span_range": rng(t_rep),
        "fanout_span_ms": round(med(fan_span), 4), "fanout_span_range": rng(fan_span),
        "fanout_post_wait_ms": round(med(fan_post), 4), "fanout_post_wait_range": rng(fan_post),
        "fanout_ns_per_delivery": round(med(fan_post) * 1e6 / ndel, 3),
        "send_post_wait_ms": round(med(send_post), 4), "send_post_wait_range": rng(send_post),
        "build_frames_ms": round(med(build), 4), "build_frames_range": rng(build),
        "ratio_send_to_build": round(med(send_post) / med(build), 4),
        "send_out_GBps": round(want_len / med(send_post) / 1e6, 1),
        "echo_send_post_wait_ms": round(med(echo_post), 4), "echo_send_post_wait_range": rng(echo_post),
        "fanout_plus_send_ms": round(fan_turn, 4), "echo_turn_ms": round(echo_turn, 4),
        "echo_turn_scaled_ms": round(echo_turn * scale, 4), "scale": round(scale, 3),
        "ratio_fanout_to_scaled_echo": round(fan_turn / (echo_turn * scale), 4),
        "kernel_send": kern,
        "checked": "delivery count; reply[], first / count and the delivery rows against the order computed on the "
                   "host; digest of the send's output == digest of hvws_build_frames' output",
    }
    print(json.dumps(row), flush=True)
    for b in (rx, msg, out, d_first, d_member):
        b.free()
    tx.free()
    dp.free()


def main():
    reps = int(os.environ.get("REPS", "5"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 15)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    if n3:
        shape(eng, "c3", n3, 65536, reps)
    if n2:
        shape(eng, "c2", n2, 1024, reps)
    eng.close()


if __name__ == "__main__":
    main()
