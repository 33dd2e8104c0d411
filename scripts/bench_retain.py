#!/usr/bin/env python3
"""hvws_retain measurement: the pass's span and device time, its table part
alone (the same call with a 16-byte slot: every publication is oversize, so
nothing is copied and the copy kernel finds no tile), the copy as the difference
of the two with its read-plus-written rate, and beside them, in the same loop
and alternating, the two yardsticks: hvws_route's span and device time (for the
table part) and hvws_d2d of the same number of bytes out of the same buffer (for
the copy).

The shapes are scripts/bench_route.py's: one card, device resident, 4096
connections (one segment each) of masked FIN binary frames in rooms of 16;
  * "c3": 64 KiB frames (FRAMES_C3 of them), slot 64 KiB;
  * "c2": 1 KiB frames (FRAMES_C2 of them), slot 1 KiB.
Each batch is scanned, reassembled (hvws_messages, masked = 1) and answered
(hvws_replies, SERVER | ECHO); then the first bytes of every message in the
message call's output are overwritten with "P<topic>\\n".  There are 4096
topics, 16 per room: message j of connection c goes to topic
16 * (c // 16) + (c + j) % 16, so every topic is published to by the
connections of its room (by all 16 in c2, by 8 of them in c3, where a
connection sends 8 messages) and the turn stores 4096 bodies of ~1 KiB or
~64 KiB, each the last of its topic's publications in reply order.  Run one
process per shape (FRAMES_C2=0 or FRAMES_C3=0).
Checks, in the same run: the entries, the totals and every stored body against
numpy on the host; no snapshot row (no message subscribes).

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
from bench_fanout import FIN, NSEG, ROOM, span  # noqa: E402


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
    rep_table, _ = eng.reply_table()
    rfirst, rcount = eng.segment_replies(nseg)
    sender = np.repeat(np.arange(nseg, dtype=np.int64), rcount.astype(np.int64))
    j = np.arange(p.n, dtype=np.int64) - np.repeat(rfirst.astype(np.int64), rcount.astype(np.int64))
    ntopics = nseg
    topic = ROOM * (sender // ROOM) + (sender + j) % ROOM
    # "P<topic>\n" over the first bytes of every message, in the message call's output
    host = msg.download(nbytes)
    off = rep_table["off"].astype(np.int64)
    lens = rep_table["len"].astype(np.int64)
    assert int(lens.min()) >= 8
    nd = np.where(topic < 10, 1, np.where(topic < 100, 2, np.where(topic < 1000, 3, 4)))
    assert ntopics <= 10000
    hlen = nd + 2
    host[off] = ord("P")
    for k in range(4):                       # digit k of the ids that have one
        has = nd > k
        host[off[has] + 1 + k] = (topic[has] // 10 ** (nd[has] - 1 - k)) % 10 + ord("0")
    host[off + 1 + nd] = ord("\n")
    libhv_amd._check(L.hvws_h2d(eng.ctx, msg.ptr, host.ctypes.data, nbytes), "hvws_h2d")
    eng.sync()
    dest_of = np.arange(nseg, dtype=np.uint32)
    slot = (payload + 15) // 16 * 16
    store = eng.alloc(ntopics * slot + 64)
    ret = eng.alloc(ntopics * 16 + 64)
    ret16 = eng.alloc(ntopics * 16 + 64)
    for b, n in ((store, ntopics * slot), (ret, ntopics * 16), (ret16, ntopics * 16)):
        libhv_amd._check(L.hvws_memset(eng.ctx, b.ptr, 0, n), "hvws_memset")

    # the pass against numpy: the last publication per topic in reply order
    eng.route(ntopics, nseg, dest_of)
    eng.retain(store, slot, ret)
    win = np.full(ntopics, -1, np.int64)
    win[topic] = np.arange(p.n)             # later replies overwrite earlier ones
    assert bool((win >= 0).all()), "every topic is published to"
    blen = (lens - hlen)[win]
    copied = int(blen.sum())
    assert eng.retain_totals() == (ntopics, 0, 0, copied, 0), eng.retain_totals()
    assert L.hvws_retain_count(eng.ctx) == 0
    ents = ret.download(ntopics * 16).view(libhv_amd.RETAINED_DTYPE)
    assert np.array_equal(ents["len"].astype(np.int64), blen) and bool((ents["set"] == 1).all())
    assert np.array_equal(ents["flags"], rep_table["flags"][win])
    got = store.download(ntopics * slot).reshape(ntopics, slot)
    src = (off + hlen)[win]
    for t in range(ntopics):
        n = int(blen[t])
        assert np.array_equal(got[t, :n], host[src[t]:src[t] + n]), f"topic {t}"
        assert not got[t, n:].any(), f"topic {t}: bytes beyond the body"
    del got, host

    def route():
        eng.route(ntopics, nseg, dest_of)

    t_route, route_dev, t_ret, ret_dev, tab_dev, t_d2d = [], [], [], [], [], []
    for _ in range(reps + 1):
        t_route.append(span(eng, route))
        route_dev.append(eng.last_kernel_ms())
        t_ret.append(span(eng, lambda: eng.retain(store, slot, ret)))
        ret_dev.append(eng.last_kernel_ms())
        eng.retain(store, 16, ret16)          # every publication oversize: the table part and an empty copy
        tab_dev.append(eng.last_kernel_ms())
        assert eng.retain_totals() == (0, 0, ntopics, 0, 0)
        t_d2d.append(span(eng, lambda: libhv_amd._check(L.hvws_d2d(eng.ctx, store.ptr, msg.ptr, copied), "hvws_d2d")))
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    copy_ms = [a - b for a, b in zip(ret_dev, tab_dev)]
    gbs = lambda ms: round(2 * copied / (ms * 1e-3) / 1e9, 1)
    row = {
        "bench": "retain", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "topics": ntopics,
        "slot": slot, "bytes_copied": copied, "reps": reps,
        "route_span_ms": round(med(t_route), 4), "route_span_range": rng(t_route),
        "route_device_ms": round(med(route_dev), 4), "route_device_range": rng(route_dev),
        "retain_span_ms": round(med(t_ret), 4), "retain_span_range": rng(t_ret),
        "retain_device_ms": round(med(ret_dev), 4), "retain_device_range": rng(ret_dev),
        "retain_table_only_ms": round(med(tab_dev), 4), "retain_table_only_range": rng(tab_dev),
        "copy_ms": round(med(copy_ms), 4), "copy_range": rng(copy_ms), "copy_read_plus_written_gbs": gbs(med(copy_ms)),
        "d2d_span_ms": round(med(t_d2d), 4), "d2d_span_range": rng(t_d2d), "d2d_read_plus_written_gbs": gbs(med(t_d2d)),
        "retain_ns_per_reply_table_only": round(med(tab_dev) * 1e6 / p.n, 3),
        "ratio_table_only_to_route_device": round(med(tab_dev) / med(route_dev), 4),
        "ratio_copy_to_d2d": round(med(copy_ms) / med(t_d2d), 4),
        "checked": "entries, totals and every stored body of hvws_retain against numpy; no byte beyond a body written; "
                   "no snapshot row",
    }
    print(json.dumps(row), flush=True)
    for b in (rx, msg, store, ret, ret16):
        b.free()
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
