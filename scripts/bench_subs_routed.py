#!/usr/bin/env python3
"""hvws_subs_update_routed measurement: the call beside the host flow it replaces.

One shape per process (argv[1]: a or b), scripts/bench_subs.py's two tables:
  * "a": 4096 destinations, 4096 rooms of 16 (65 536 listings), 256 events;
  * "b": 1 048 576 destinations, 65 536 topics of 64 (4 194 304 listings), 41 943 events.
The events arrive as routed messages: one connection per event sends "S<room>\\n"
(a pair no row lists) or "U<room>\\n" (a pair a row lists); every 100th of them
also sends a CLOSE (1 % of the connections closed); a few more connections
publish, and 1 % of the destinations -- all reached by a publication -- have a
budget of 0 and go OVER.  16 host events ride along.  Behind scan,
hvws_messages_rfc, hvws_replies, hvws_route, hvws_fanout_routed and hvws_budget,
alternating in one loop:
  a. the host flow: hvws_get_route_events + hvws_get_route_flags +
     hvws_get_reply_flags + hvws_get_dest_budget (flags only), the merged array
     built with numpy, hvws_subs_update over it;
  b. hvws_subs_update_routed: the whole call, and the device time after its
     second wait (hvws_last_kernel_ms: the placement);
  c. one word read back with a wait on the idle stream (hvws_route_event_count):
     what the call's extra count readback costs.
Spans are device spans (hvws_span_begin / _end: the host's work between the two
marks is inside them); wall times beside them.  Check: (a) and (b) leave the
same two arrays and counts, and the merged array of (b) is the one (a) built.

REPS sets the repetitions.  Prints one JSON line.
"""
from __future__ import annotations

import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import libhv_amd  # noqa: E402
from bench_subs import span, table  # noqa: E402

SHAPES = {
    # name: (ndest, ntopics, row, events)
    "a": (4096, 4096, 16, 256),
    "b": (1 << 20, 1 << 16, 64, 41943),
}
CLOSE = bytes([0x88, 0x82, 0, 0, 0, 0, 0x03, 0xE8])   # masked (key 0) FIN CLOSE 1000


def frame(payload: bytes) -> bytes:
    assert len(payload) < 126
    return bytes([0x81, 0x80 | len(payload), 0, 0, 0, 0]) + payload     # masked (key 0) FIN text


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "a"
    ndest, ntopics, row, nev = SHAPES[name]
    reps = int(os.environ.get("REPS", "5"))
    L = libhv_amd.lib()
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    rng = np.random.default_rng(40 + ord(name))
    first, member = table(ndest, ntopics, row, rng)
    nmember = len(member)
    # the publications, and the 1 % of the destinations they put over
    nover = ndest // 100
    npub = nover * 13 // (10 * row) + 2
    pub_t = rng.choice(ntopics, npub, replace=False)
    reached = np.unique(member.reshape(ntopics, row)[pub_t].ravel())
    assert len(reached) >= nover
    over = np.sort(rng.choice(reached, nover, replace=False))
    # one connection per event, the publishers behind them
    nseg = nev + npub
    dest_of = rng.choice(ndest, nseg, replace=False).astype(np.uint32)
    nl = nev // 2
    at = rng.choice(nmember, nl, replace=False)               # LEAVEs of listed pairs
    jt = rng.choice(ntopics, nev - nl, replace=ntopics < nev - nl)
    reads = []
    for s in range(nev):
        if s < nl:
            dest_of[s] = member[at[s]]       # the sender is the listed destination itself
            msg = b"U%d\n" % (at[s] // row)
        else:
            msg = b"S%d\n" % jt[s - nl]
        reads.append(frame(msg) + (CLOSE if s % 100 == 0 else b""))
    for k in range(npub):
        reads.append(frame(b"P%d\nhi" % pub_t[k]))
    data = np.frombuffer(b"".join(reads), np.uint8)
    segs, o = [], 0
    for r in reads:
        segs.append((o, len(r)))
        o += len(r)
    host = np.zeros(16, libhv_amd.SUB_EVENT_DTYPE)
    host["op"], host["topic"], host["dest"] = libhv_amd.SUB_JOIN, rng.choice(ntopics, 16), rng.choice(ndest, 16)
    budgets = np.full(ndest, (1 << 64) - 1, np.uint64)
    budgets[over] = 0

    rx, msg = eng.to_device(data), eng.alloc(len(data) + 64)
    d_first, d_member, d_budget = eng.to_device(first), eng.to_device(member), eng.to_device(budgets)
    cap = nmember + nev + 64
    outs = [(eng.alloc(8 * (ntopics + 1) + 64), eng.alloc(4 * cap + 64)) for _ in range(2)]
    eng.scan(rx, len(data), segs)
    eng.messages_rfc(rx, len(data), True, msg, len(data))
    eng.replies(libhv_amd.R_SERVER | libhv_amd.R_ECHO)
    eng.route(ntopics, ndest, dest_of)
    eng.fanout_routed(d_first, d_member, nmember)
    eng.budget(d_budget, 0)
    assert eng.route_totals()[3] == 0 and eng.budget_totals()[3] == nover
    merged = {}

    def host_flow():
        ev = eng.route_events()
        rt = np.zeros(nseg, np.uint8)
        libhv_amd._check(L.hvws_get_route_flags(eng.ctx, rt.ctypes.data, None), "hvws_get_route_flags")
        rf = eng.reply_flags(nseg)
        bf = np.zeros(ndest, np.uint8)
        libhv_amd._check(L.hvws_get_dest_budget(eng.ctx, None, None, None, bf.ctypes.data), "hvws_get_dest_budget")
        gone = dest_of[((rf & libhv_amd.RF_CLOSED) | (rt & libhv_amd.RT_BAD)) != 0]
        ov = np.flatnonzero(bf & libhv_amd.BF_OVER)
        m = np.zeros(len(ev) + len(gone) + len(ov) + len(host), libhv_amd.SUB_EVENT_DTYPE)
        a, b, c = len(ev), len(ev) + len(gone), len(ev) + len(gone) + len(ov)
        m[:a] = ev
        m["op"][a:c] = libhv_amd.SUB_DROP
        m["dest"][a:b] = gone
        m["dest"][b:c] = ov
        m[c:] = host
        merged["host"] = m
        return eng.subs_update(d_first, d_member, ntopics, nmember, ndest, m, None, outs[0][0], outs[0][1], cap)

    def routed():
        return eng.subs_update_routed(d_first, d_member, nmember, host, outs[1][0], outs[1][1], cap, libhv_amd.SUBS_OVER)

    def word():
        assert L.hvws_route_event_count(eng.ctx) == nev

    def timed(fn):
        t0 = time.perf_counter()
        ms = span(eng, fn)
        return ms, (time.perf_counter() - t0) * 1e3

    n0, c0 = host_flow(), eng.subs_counts()
    n1, c1 = routed(), eng.subs_counts()
    assert n0 == n1 and c0 == c1, (n0, n1, c0, c1)
    parts = eng.subs_merged()
    assert parts == (nev, (nev + 99) // 100, nover, 16), parts
    assert eng.subs_events().tobytes() == merged["host"].tobytes(), "the merged arrays differ"
    fb = 8 * (ntopics + 1)
    assert np.array_equal(outs[0][0].download(fb, np.uint64), outs[1][0].download(fb, np.uint64))
    assert np.array_equal(outs[0][1].download(4 * n0, np.uint32), outs[1][1].download(4 * n1, np.uint32))
    ha, hw, ra, rw, post, rb = [], [], [], [], [], []
    for _ in range(reps + 1):
        s, w = timed(host_flow)
        ha.append(s)
        hw.append(w)
        s, w = timed(routed)
        ra.append(s)
        rw.append(w)
        post.append(eng.last_kernel_ms())
        rb.append(timed(word)[1])
    med = lambda v: float(np.median(v[1:]))
    rg = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    print(json.dumps({
        "bench": "subs_routed", "shape": name, "destinations": ndest, "topics": ntopics, "listings": nmember,
        "segments": nseg, "merged": list(parts), "new_listings": n1, "reps": reps,
        "host_flow_span_ms": round(med(ha), 4), "host_flow_span_range": rg(ha),
        "host_flow_wall_ms": round(med(hw), 4), "host_flow_wall_range": rg(hw),
        "routed_span_ms": round(med(ra), 4), "routed_span_range": rg(ra),
        "routed_wall_ms": round(med(rw), 4), "routed_wall_range": rg(rw),
        "routed_post_wait_ms": round(med(post), 4), "routed_post_wait_range": rg(post),
        "count_readback_wall_ms": round(med(rb), 4), "count_readback_range": rg(rb),
        "ratio_routed_to_host_span": round(med(ra) / med(ha), 3),
        "ratio_routed_to_host_wall": round(med(rw) / med(hw), 3),
        "checked": "both output arrays, the counts and the merged array of the two flows against each other",
    }), flush=True)
    eng.sync()
    for b in (rx, msg, d_first, d_member, d_budget) + outs[0] + outs[1]:
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
