#!/usr/bin/env python3
"""Routed pub/sub turn measurement: hvws_route alone, hvws_fanout_routed (the
whole call and the device time after its wait) and the send from its table,
against the unrouted path over the same batch in the same loop, alternating:
hvws_fanout with pub[s] and its send (scripts/bench_fanout.py's measurement).

The shapes are bench_fanout's: one card, device resident, 4096 connections (one
segment each) of masked FIN binary frames in rooms of 16, connection s in room
s // 16, HVWS_FAN_SELF set, so every message is delivered 16 times:
  * "c3": 64 KiB frames (FRAMES_C3 of them);
  * "c2": 1 KiB frames (FRAMES_C2 of them).
Each batch is scanned, reassembled (hvws_messages, masked = 1) and answered
(hvws_replies, SERVER | ECHO); then the first bytes of every message in the
message call's output are overwritten with "P<room>\\n", so every message is a
publication to its sender's room and both paths deliver the same replies to the
same destinations (the unrouted one with the header still in front).  Run one
process per shape (FRAMES_C2=0 or FRAMES_C3=0).
Checks, in the same run: every output of the route pass against numpy on the
host (rows, topics, kinds, no events, flags, bad_reply, totals); the routed
delivery table against the unrouted one (same replies, same destinations, rows
trimmed); the digest of the send's output against hvws_build_frames on the
identical frames.

REPS sets the repetitions.  Prints JSON lines.
"""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import libhv_amd  # noqa: E402
from libhv_amd import synth  # noqa: E402
from bench_fanout import FIN, FRAGMENT, NSEG, ROOM, frame_tables, hdr_len, span  # noqa: E402


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
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.messages(rx, p.total, True, msg, p.total)
    eng.replies(policy)
    assert L.hvws_reply_count(eng.ctx) == p.n, "one echo per frame"
    nbytes = eng.msg_bytes()
    rep_table, piece = eng.reply_table()
    rfirst, rcount = eng.segment_replies(nseg)
    sender = np.repeat(np.arange(nseg, dtype=np.int64), rcount.astype(np.int64))
    room = sender // ROOM
    assert np.array_equal(rfirst.astype(np.int64), np.concatenate(([0], np.cumsum(rcount.astype(np.int64))[:-1])))
    # "P<room>\n" over the first bytes of every message, in the message call's output
    host = msg.download(nbytes)
    hlen = np.array([len(b"P%d\n" % r) for r in range(nseg // ROOM)], np.int64)[room]
    off = rep_table["off"].astype(np.int64)
    assert int(rep_table["len"].min()) >= 8
    for r in range(nseg // ROOM):
        h = np.frombuffer(b"P%d\n" % r, np.uint8)
        at = off[room == r]
        for k in range(len(h)):
            host[at + k] = h[k]
    libhv_amd._check(L.hvws_h2d(eng.ctx, msg.ptr, host.ctypes.data, nbytes), "hvws_h2d")
    eng.sync()
    del host
    ntopics = nseg // ROOM
    topic_first = np.arange(ntopics + 1, dtype=np.uint64) * ROOM
    member = np.arange(nseg, dtype=np.uint32)
    d_first, d_member = eng.to_device(topic_first), eng.to_device(member)
    pub = (np.arange(nseg) // ROOM).astype(np.uint32)
    dest_of = np.arange(nseg, dtype=np.uint32)

    def route():
        eng.route(ntopics, nseg, dest_of)

    def fan_routed():
        return eng.fanout_routed(d_first, d_member, nseg, libhv_amd.FAN_SELF)

    def fan_plain():
        return eng.fanout(d_first, d_member, ntopics, nseg, nseg, pub, dest_of, libhv_amd.FAN_SELF)

    # the route pass against numpy
    route()
    rows, topic, kind = eng.route_table()
    assert np.array_equal(kind, np.full(p.n, libhv_amd.RK_PUB, np.uint8)), "kinds"
    assert np.array_equal(topic.astype(np.int64), room), "topics"
    assert np.array_equal(rows["off"].astype(np.int64), off + hlen), "rows.off"
    assert np.array_equal(rows["len"].astype(np.int64), rep_table["len"].astype(np.int64) - hlen), "rows.len"
    assert np.array_equal(rows["flags"], rep_table["flags"]) and np.array_equal(rows["key"], rep_table["key"])
    assert len(eng.route_events()) == 0 and eng.route_totals() == (p.n, 0, 0, 0)
    rflags, bad = eng.route_flags(nseg)
    assert not rflags.any() and bool((bad == libhv_amd.ROUTE_NONE).all())
    # the routed delivery table against the unrouted one
    ndel = fan_plain()
    assert ndel == p.n * ROOM
    ptable, preply = eng.fanout_table()
    pfirst, pcount = eng.dest_fanout(nseg)
    assert fan_routed() == ndel
    table, reply = eng.fanout_table()
    first, count = eng.dest_fanout(nseg)
    assert np.array_equal(reply, preply) and np.array_equal(first, pfirst) and np.array_equal(count, pcount)
    assert np.array_equal(table, rows[reply.astype(np.int64)]), "the routed delivery table is not the routed rows"
    assert np.array_equal(ptable, rep_table[reply.astype(np.int64)])
    # the unrouted send's size: whole messages (64 KiB ones in two fragments)
    per = 1 if payload <= FRAGMENT else -(-payload // FRAGMENT)
    plast = payload - (per - 1) * FRAGMENT
    plain_len = ndel * ((per - 1) * (hdr_len(FRAGMENT) + FRAGMENT) + hdr_len(plast) + plast)
    plain_frames = ndel * per
    out = eng.alloc(plain_len + 64)
    # hvws_build_frames' tables for the routed deliveries: frames of the trimmed
    # bodies (a 64 KiB message less its header fits one fragment)
    lens = table["len"].astype(np.int64)
    perd = np.maximum(1, -(-lens // FRAGMENT))
    want_frames = int(perd.sum())
    j = np.arange(want_frames, dtype=np.int64) - np.repeat(np.cumsum(perd) - perd, perd)
    pr = np.repeat(perd, perd)
    length = np.where(j + 1 < pr, FRAGMENT, np.repeat(lens - (perd - 1) * FRAGMENT, perd))
    flags = (np.where(j == 0, op, 0) | np.where(j + 1 == pr, FIN, 0)).astype(np.uint8)
    want_len = int((np.where(length < 126, 2, np.where(length <= 0xFFFF, 4, 10)) + length).sum())
    tx = libhv_amd.TxPlan(eng, np.repeat(table["off"].astype(np.int64), perd) + j * FRAGMENT, length, flags)
    del table, reply, ptable, preply, rows, j, pr, length, flags

    def send():
        t, d_n, n = eng.fanout_device()
        return eng.send_messages(out, plain_len + 64, msg, p.total, t, n, d_n, 0, False)

    t_rep, t_route, route_dev = [], [], []
    r_span, r_post, r_send, p_span, p_post, p_send, build = [], [], [], [], [], [], []
    digests = set()
    for k in range(reps + 1):
        t_rep.append(span(eng, lambda: eng.replies(policy)))
        p_span.append(span(eng, fan_plain))
        p_post.append(eng.last_kernel_ms())
        assert send() == (plain_len, plain_frames)
        p_send.append(eng.last_kernel_ms())
        t_route.append(span(eng, route))
        route_dev.append(eng.last_kernel_ms())
        r_span.append(span(eng, fan_routed))
        r_post.append(eng.last_kernel_ms())
        assert send() == (want_len, want_frames)
        r_send.append(eng.last_kernel_ms())
        if k == 0:
            digests.add(eng.digest(out, want_len))
            libhv_amd._check(L.hvws_memset(eng.ctx, out.ptr, 0, min(want_len, 1 << 20)), "hvws_memset")
        assert eng.build_frames(out, plain_len + 64, msg, p.total, tx) == want_len
        build.append(eng.last_kernel_ms())
        if k == 0:
            digests.add(eng.digest(out, want_len))
    assert len(digests) == 1, f"{name}: the send from the routed table and hvws_build_frames wrote different bytes"
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    row = {
        "bench": "route", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "room": ROOM,
        "deliveries": ndel, "frames": want_frames, "out_bytes": want_len, "reps": reps,
        "replies_span_ms": round(med(t_rep), 4), "replies_span_range": rng(t_rep),
        "route_span_ms": round(med(t_route), 4), "route_span_range": rng(t_route),
        "route_device_ms": round(med(route_dev), 4), "route_device_range": rng(route_dev),
        "route_ns_per_reply": round(med(route_dev) * 1e6 / p.n, 3),
        "routed_span_ms": round(med(r_span), 4), "routed_span_range": rng(r_span),
        "routed_post_wait_ms": round(med(r_post), 4), "routed_post_wait_range": rng(r_post),
        "routed_send_ms": round(med(r_send), 4), "routed_send_range": rng(r_send),
        "plain_span_ms": round(med(p_span), 4), "plain_span_range": rng(p_span),
        "plain_post_wait_ms": round(med(p_post), 4), "plain_post_wait_range": rng(p_post),
        "plain_send_ms": round(med(p_send), 4), "plain_send_range": rng(p_send),
        "build_frames_ms": round(med(build), 4), "build_frames_range": rng(build),
        "ratio_routed_span": round(med(r_span) / med(p_span), 4),
        "ratio_routed_post_wait": round(med(r_post) / med(p_post), 4),
        "ratio_routed_send": round(med(r_send) / med(p_send), 4),
        "ratio_route_to_replies": round(med(t_route) / med(t_rep), 4),
        "checked": "rows, topics, kinds, events, flags, bad_reply and totals of hvws_route against numpy; the routed "
                   "delivery table against the unrouted one; digest of the send's output == digest of "
                   "hvws_build_frames' output",
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
