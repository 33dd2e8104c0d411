#!/usr/bin/env python3
"""Budget pass measurement: hvws_budget beside hvws_fanout's device work, beside
a device-to-device copy of the delivery table (the floor: the table read and
written once), and the send from the budget table beside the send from the
fan-out's table.

scripts/bench_fanout.py's two shapes on one card, device resident, 4096
connections (one segment each) of masked FIN binary frames in rooms of 16,
HVWS_FAN_SELF set, so every message is delivered 16 times:
  * "c3": 64 KiB frames (FRAMES_C3 of them);
  * "c2": 1 KiB frames (FRAMES_C2 of them).
The budgets cut about 1 % of the destinations in half: every 100th destination
may be sent half of its deliveries' wire bytes, every other one exactly its
whole (equality keeps).  Per shape, in one loop of one process:
  a. hvws_fanout's device time after its wait (hvws_last_kernel_ms);
  b. hvws_budget's device time (hvws_last_kernel_ms: the whole pass), and the
     device span of the call -- it does not wait, so the two agree but for the
     enqueue;
  c. hvws_d2d of the delivery table (24 B per delivery read and written once),
     as a device span;
  d. the send from the budget table with out_cap = the totals' kept bytes,
     device time after its wait, against the send from the fan-out's table (what
     unlimited budgets keep); the two alternate.
Checks: first / count / byte_off / flags and the totals against the same rule
computed on the host with numpy, the kept rows and reply[] against the fan-out's
rows gathered on the host, *out_len of the send == the totals' kept bytes, and
the unlimited pass's table == the fan-out's.

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
EVERY = 100   # one destination in EVERY is cut in half
UNLIMITED = (1 << 64) - 1


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


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    nseg = len(p.segments)
    assert nseg % ROOM == 0
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    msg = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    per = 1 if payload <= FRAGMENT else -(-payload // FRAGMENT)
    last = payload - (per - 1) * FRAGMENT
    msg_out = (per - 1) * (hdr_len(FRAGMENT) + FRAGMENT) + hdr_len(last) + last
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.messages(rx, p.total, True, msg, p.total)
    eng.replies(policy)
    topic_first = np.arange(nseg // ROOM + 1, dtype=np.uint64) * ROOM
    member = np.arange(nseg, dtype=np.uint32)
    d_first, d_member = eng.to_device(topic_first), eng.to_device(member)
    pub = (np.arange(nseg) // ROOM).astype(np.uint32)
    dest_of = np.arange(nseg, dtype=np.uint32)

    def fanout():
        return eng.fanout(d_first, d_member, nseg // ROOM, nseg, nseg, pub, dest_of, libhv_amd.FAN_SELF)

    ndel = fanout()
    assert ndel == p.n * ROOM
    table, reply = eng.fanout_table()
    first, count = (a.astype(np.int64) for a in eng.dest_fanout(nseg))
    assert bool((table["len"] == payload).all()), "the shapes are uniform"
    # the rule on the host: every delivery has msg_out wire bytes
    cut = np.arange(nseg) % EVERY == EVERY - 1
    budgets = np.where(cut, (count * msg_out) // 2, count * msg_out).astype(np.uint64)
    want_count = np.where(cut, (count * msg_out // 2) // msg_out, count)
    want_first = np.concatenate(([0], np.cumsum(want_count)[:-1]))
    want_off = np.concatenate(([0], np.cumsum(want_count * msg_out)))
    want_flags = (want_count < count).astype(np.uint8)
    kept = int(want_count.sum())
    src = np.repeat(first - want_first, want_count) + np.arange(kept, dtype=np.int64)   # the fan-out row of each kept row
    d_budget = eng.to_device(budgets)

    def check():
        f2, c2, off, fl = eng.dest_budget(nseg)
        assert np.array_equal(f2.astype(np.int64), want_first) and np.array_equal(c2.astype(np.int64), want_count)
        assert np.array_equal(off.astype(np.int64), want_off) and np.array_equal(fl, want_flags)
        assert eng.budget_totals() == (kept, kept * msg_out, ndel - kept, int(want_flags.sum()))
        t2, r2 = eng.budget_table()
        assert np.array_equal(t2, table[src]) and np.array_equal(r2, reply[src]), "the kept rows are not the fan-out's"

    eng.budget(None, UNLIMITED, 0, False)
    t2, r2 = eng.budget_table()
    assert np.array_equal(t2, table) and np.array_equal(r2, reply), "unlimited budgets must keep the table"
    assert eng.budget_totals() == (ndel, ndel * msg_out, 0, 0)
    del t2, r2
    eng.budget(d_budget, 0, 0, False)
    check()
    want_len = ndel * msg_out
    out = eng.alloc(want_len + 64)
    copy = eng.alloc(ndel * 24 + 64)

    def send_fan():
        t, d_n, n = eng.fanout_device()
        return eng.send_messages(out, want_len, msg, p.total, t, n, d_n, 0, False)

    def send_budget():
        t, d_n, n = eng.budget_device()
        return eng.send_messages(out, kept * msg_out, msg, p.total, t, n, d_n, 0, False)

    fan_post, bud, bud_span, d2d, s_bud, s_fan = [], [], [], [], [], []
    for k in range(reps + 1):
        assert fanout() == ndel
        fan_post.append(eng.last_kernel_ms())
        bud_span.append(span(eng, lambda: eng.budget(d_budget, 0, 0, False)))
        bud.append(eng.last_kernel_ms())
        fan_addr = L.hvws_fanout_device(eng.ctx)
        d2d.append(span(eng, lambda: libhv_amd._check(L.hvws_d2d(eng.ctx, copy.ptr, fan_addr, ndel * 24), "hvws_d2d")))
        assert send_budget() == (kept * msg_out, kept * per)
        s_bud.append(eng.last_kernel_ms())
        assert send_fan() == (want_len, ndel * per)
        s_fan.append(eng.last_kernel_ms())
    check()
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    row = {
        "bench": "budget", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "room": ROOM,
        "deliveries": ndel, "destinations": nseg, "destinations_over": int(want_flags.sum()),
        "kept_deliveries": kept, "kept_bytes": kept * msg_out, "out_bytes_uncut": want_len, "reps": reps,
        "fanout_post_wait_ms": round(med(fan_post), 4), "fanout_post_wait_range": rng(fan_post),
        "budget_ms": round(med(bud), 4), "budget_range": rng(bud),
        "budget_span_ms": round(med(bud_span), 4), "budget_span_range": rng(bud_span),
        "budget_ns_per_delivery": round(med(bud) * 1e6 / ndel, 3),
        "table_d2d_ms": round(med(d2d), 4), "table_d2d_range": rng(d2d),
        "ratio_budget_to_fanout": round(med(bud) / med(fan_post), 4),
        "ratio_budget_to_d2d": round(med(bud) / med(d2d), 3),
        "send_budget_post_wait_ms": round(med(s_bud), 4), "send_budget_range": rng(s_bud),
        "send_fanout_post_wait_ms": round(med(s_fan), 4), "send_fanout_range": rng(s_fan),
        "send_budget_out_GBps": round(kept * msg_out / med(s_bud) / 1e6, 1),
        "send_fanout_out_GBps": round(want_len / med(s_fan) / 1e6, 1),
        "checked": "first / count / byte_off / flags and the totals against the rule computed on the host; the kept "
                   "rows and reply[] against the fan-out's rows; *out_len of the send == the totals' kept bytes; "
                   "unlimited budgets keep the fan-out's table",
    }
    print(json.dumps(row), flush=True)
    for b in (rx, msg, out, copy, d_first, d_member, d_budget):
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
