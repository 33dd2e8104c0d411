#!/usr/bin/env python3
"""hvws_envelope measurement: the pass's span and device time, its table part
alone (the same call behind a route with ntopics = 0: every message is BAD or
STOPPED, so nothing is copied and the copy kernel finds no tile), the copy as
the difference of the two with its read-plus-written rate, and beside them, in
the same loop and alternating, the two yardsticks: hvws_route's device time
(for the table part: the same three passes over the same replies) and hvws_d2d
of the same number of bytes between the same two buffers (for the copy).  Then
the cost to the turn: hvws_fanout_enveloped and hvws_send_messages from d_env
beside hvws_fanout_routed and hvws_send_messages from the message output, on
the same batch, alternating.

The shapes are scripts/bench_route.py's: one card, device resident, 4096
connections (one segment each) of masked FIN binary frames in rooms of 16,
HVWS_FAN_SELF set, so every message is delivered 16 times;
  * "c3": 64 KiB frames (FRAMES_C3 of them);
  * "c2": 1 KiB frames (FRAMES_C2 of them).
Each batch is scanned, reassembled (hvws_messages, masked = 1) and answered
(hvws_replies, SERVER | ECHO); then the first bytes of every message in the
message call's output are overwritten with "P<room>\\n".  The envelope names
topic and sender (HVWS_ENV_SENDER).  Run one process per shape (FRAMES_C2=0 or
FRAMES_C3=0).
Checks, in the same run: the enveloped rows and the totals against numpy on
the host; the bytes of SAMPLE replies spread over the batch (envelope line,
body, and the pad behind them untouched); the enveloped delivery table against
the routed one; the digest of the send's output from d_env against
hvws_build_frames on the identical frames.

REPS sets the repetitions.  Prints JSON lines.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import libhv_amd  # noqa: E402
from libhv_amd import synth  # noqa: E402
from bench_fanout import FIN, FRAGMENT, NSEG, ROOM, span  # noqa: E402

SAMPLE = 2048
SEED = 0xC3


def digits(v: np.ndarray) -> np.ndarray:
    return np.where(v < 10, 1, np.where(v < 100, 2, np.where(v < 1000, 3, 4)))


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    nseg = len(p.segments)
    assert nseg % ROOM == 0 and nseg <= 10000
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    msg = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    op = int(p.flags[0]) & 0xF
    assert op in (1, 2) and bool((p.flags & FIN).all()), "the shapes are FIN data frames"
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.messages(rx, p.total, True, msg, p.total)
    eng.replies(policy)
    assert L.hvws_reply_count(eng.ctx) == p.n, "one echo per frame"
    nbytes = eng.msg_bytes()
    rep_table, _ = eng.reply_table()
    rfirst, rcount = eng.segment_replies(nseg)
    sender = np.repeat(np.arange(nseg, dtype=np.int64), rcount.astype(np.int64))
    room = sender // ROOM
    # "P<room>\n" over the first bytes of every message, in the message call's output
    host = msg.download(nbytes)
    hlen = digits(room) + 2
    off = rep_table["off"].astype(np.int64)
    assert int(rep_table["len"].min()) >= 8
    for r in range(nseg // ROOM):
        h = np.frombuffer(b"P%d\n" % r, np.uint8)
        at = off[room == r]
        for k in range(len(h)):
            host[at + k] = h[k]
    libhv_amd._check(L.hvws_h2d(eng.ctx, msg.ptr, host.ctypes.data, nbytes), "hvws_h2d")
    eng.sync()
    ntopics = nseg // ROOM
    topic_first = np.arange(ntopics + 1, dtype=np.uint64) * ROOM
    member = np.arange(nseg, dtype=np.uint32)
    d_first, d_member = eng.to_device(topic_first), eng.to_device(member)
    dest_of = np.arange(nseg, dtype=np.uint32)

    eng.route(ntopics, nseg, dest_of)
    env_cap = eng.envelope_bound()
    assert env_cap == p.total + 38 * int(L.hvws_reply_capacity(eng.ctx)) + 16
    env = eng.alloc(env_cap + 64)
    libhv_amd._check(L.hvws_memset(eng.ctx, env.ptr, SEED, env_cap + 64), "hvws_memset")

    # the pass against numpy
    eng.envelope(env, env_cap, libhv_amd.ENV_SENDER)
    rows, topic, kind = eng.route_table()
    assert bool((kind == libhv_amd.RK_PUB).all())
    blen = rows["len"].astype(np.int64)
    src = rows["off"].astype(np.int64)
    eh = 3 + digits(room) + digits(sender)                      # 'M' topic ' ' sender LF
    size = eh + blen
    e = np.concatenate(([0], np.cumsum((size + 15) // 16 * 16)))
    got = eng.envelope_table()
    assert np.array_equal(got["off"].astype(np.int64), e[:-1]) and np.array_equal(got["len"].astype(np.int64), size)
    assert np.array_equal(got["flags"], rows["flags"]) and np.array_equal(got["key"], rows["key"])
    written, spanned = int(size.sum()), int(e[-1])
    assert eng.envelope_totals() == (p.n, 0, written, spanned), eng.envelope_totals()
    for i in np.unique(np.linspace(0, p.n - 1, SAMPLE).astype(np.int64)):
        padded = int(e[i + 1] - e[i])
        mine = np.zeros(padded, np.uint8)
        libhv_amd._check(L.hvws_d2h(eng.ctx, mine.ctypes.data, env.ptr + int(e[i]), padded), "hvws_d2h")
        eng.sync()
        line = b"M%d %d\n" % (room[i], sender[i])
        want = line + host[src[i]:src[i] + blen[i]].tobytes()
        assert mine[:len(want)].tobytes() == want, f"reply {i}"
        assert bool((mine[len(want):] == SEED).all()), f"reply {i}: pad bytes written"
    del host
    # the enveloped delivery table against the routed one
    ndel = eng.fanout_routed(d_first, d_member, nseg, libhv_amd.FAN_SELF)
    assert ndel == p.n * ROOM
    rtable, rreply = eng.fanout_table()
    assert eng.fanout_enveloped(d_first, d_member, nseg, libhv_amd.FAN_SELF) == ndel
    table, reply = eng.fanout_table()
    assert np.array_equal(reply, rreply) and np.array_equal(table, got[reply.astype(np.int64)])
    assert np.array_equal(rtable, rows[reply.astype(np.int64)])

    def wire(lens):
        perd = np.maximum(1, -(-lens // FRAGMENT))
        nfr = int(perd.sum())
        j = np.arange(nfr, dtype=np.int64) - np.repeat(np.cumsum(perd) - perd, perd)
        pr = np.repeat(perd, perd)
        length = np.where(j + 1 < pr, FRAGMENT, np.repeat(lens - (perd - 1) * FRAGMENT, perd))
        flags = (np.where(j == 0, op, 0) | np.where(j + 1 == pr, FIN, 0)).astype(np.uint8)
        total = int((np.where(length < 126, 2, np.where(length <= 0xFFFF, 4, 10)) + length).sum())
        return perd, j, length, flags, total, nfr

    perd, j, length, flags, env_len, env_frames = wire(table["len"].astype(np.int64))
    tx = libhv_amd.TxPlan(eng, np.repeat(table["off"].astype(np.int64), perd) + j * FRAGMENT, length, flags)
    _, _, _, _, bare_len, bare_frames = wire(rtable["len"].astype(np.int64))
    out = eng.alloc(max(env_len, bare_len) + 64)
    del table, reply, rtable, rreply, rows, got, j, length, flags, perd

    def send(payload_buf, payload_len):
        t, d_n, n = eng.fanout_device()
        return eng.send_messages(out, max(env_len, bare_len) + 64, payload_buf, payload_len, t, n, d_n, 0, False)

    def envelope():
        eng.envelope(env, env_cap, libhv_amd.ENV_SENDER)

    route_dev, tab_route_dev, t_env, env_dev, tab_dev, t_d2d = [], [], [], [], [], []
    e_span, e_post, e_send, r_span, r_post, r_send = [], [], [], [], [], []
    digests = set()
    for k in range(reps + 1):
        eng.route(0, nseg, dest_of)                 # every message BAD or STOPPED: the table part, an empty copy
        tab_route_dev.append(eng.last_kernel_ms())
        envelope()
        tab_dev.append(eng.last_kernel_ms())
        assert eng.envelope_totals() == (0, 0, 0, 0)
        eng.route(ntopics, nseg, dest_of)
        route_dev.append(eng.last_kernel_ms())
        t_env.append(span(eng, envelope))
        env_dev.append(eng.last_kernel_ms())
        t_d2d.append(span(eng, lambda: libhv_amd._check(L.hvws_d2d(eng.ctx, out.ptr, msg.ptr, written), "hvws_d2d")))
        # the turn: from d_env ...
        e_span.append(span(eng, lambda: eng.fanout_enveloped(d_first, d_member, nseg, libhv_amd.FAN_SELF)))
        e_post.append(eng.last_kernel_ms())
        assert send(env, env_cap) == (env_len, env_frames)
        e_send.append(eng.last_kernel_ms())
        if k == 0:
            digests.add(eng.digest(out, env_len))
            libhv_amd._check(L.hvws_memset(eng.ctx, out.ptr, 0, min(env_len, 1 << 20)), "hvws_memset")
            assert eng.build_frames(out, env_len + 64, env, env_cap, tx) == env_len
            digests.add(eng.digest(out, env_len))
        # ... and from the message output
        r_span.append(span(eng, lambda: eng.fanout_routed(d_first, d_member, nseg, libhv_amd.FAN_SELF)))
        r_post.append(eng.last_kernel_ms())
        assert send(msg, p.total) == (bare_len, bare_frames)
        r_send.append(eng.last_kernel_ms())
    assert len(digests) == 1, f"{name}: the send from d_env and hvws_build_frames wrote different bytes"
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    copy_ms = [a - b for a, b in zip(env_dev, tab_dev)]
    gbs = lambda ms: round(2 * written / (ms * 1e-3) / 1e9, 1)
    turn_env = [a + b + c for a, b, c in zip(env_dev, e_span, e_send)]
    turn_bare = [a + b for a, b in zip(r_span, r_send)]
    row = {
        "bench": "envelope", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "room": ROOM,
        "bytes_written": written, "bytes_spanned": spanned, "env_cap": env_cap, "deliveries": ndel, "reps": reps,
        "route_device_ms": round(med(route_dev), 4), "route_device_range": rng(route_dev),
        "route_all_bad_device_ms": round(med(tab_route_dev), 4), "route_all_bad_device_range": rng(tab_route_dev),
        "envelope_span_ms": round(med(t_env), 4), "envelope_span_range": rng(t_env),
        "envelope_device_ms": round(med(env_dev), 4), "envelope_device_range": rng(env_dev),
        "envelope_table_only_ms": round(med(tab_dev), 4), "envelope_table_only_range": rng(tab_dev),
        "copy_ms": round(med(copy_ms), 4), "copy_range": rng(copy_ms), "copy_read_plus_written_gbs": gbs(med(copy_ms)),
        "d2d_span_ms": round(med(t_d2d), 4), "d2d_span_range": rng(t_d2d), "d2d_read_plus_written_gbs": gbs(med(t_d2d)),
        "envelope_ns_per_reply_table_only": round(med(tab_dev) * 1e6 / p.n, 3),
        "ratio_table_only_to_route_device": round(med(tab_dev) / med(route_dev), 4),
        "ratio_copy_to_d2d": round(med(copy_ms) / med(t_d2d), 4),
        "enveloped_fanout_span_ms": round(med(e_span), 4), "enveloped_fanout_span_range": rng(e_span),
        "enveloped_post_wait_ms": round(med(e_post), 4),
        "enveloped_send_ms": round(med(e_send), 4), "enveloped_send_range": rng(e_send),
        "routed_fanout_span_ms": round(med(r_span), 4), "routed_fanout_span_range": rng(r_span),
        "routed_post_wait_ms": round(med(r_post), 4),
        "routed_send_ms": round(med(r_send), 4), "routed_send_range": rng(r_send),
        "enveloped_out_bytes": env_len, "routed_out_bytes": bare_len,
        "turn_enveloped_ms": round(med(turn_env), 4), "turn_enveloped_range": rng(turn_env),
        "turn_routed_ms": round(med(turn_bare), 4), "turn_routed_range": rng(turn_bare),
        "ratio_turn": round(med(turn_env) / med(turn_bare), 4),
        "ratio_send": round(med(e_send) / med(r_send), 4),
        "checked": "rows and totals of hvws_envelope against numpy; envelope, body and pad of %d replies byte for byte; "
                   "the enveloped delivery table against the routed one; digest of the send's output from d_env == "
                   "digest of hvws_build_frames' output" % SAMPLE,
    }
    print(json.dumps(row), flush=True)
    for b in (rx, msg, env, out, d_first, d_member):
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
