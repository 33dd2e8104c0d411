#!/usr/bin/env python3
"""hvws_subs_update measurement: the pass beside the floor of its traffic and
beside what the caller does without it.

One shape per process (argv[1]: a or b), device resident, behind a real reply
call whose CLOSE frames mark the closed connections:
  * "a": scripts/bench_fanout.py's scale -- 4096 destinations, 4096 rooms of 16
    (65 536 listings, every destination in 16 rooms), 64 closed connections,
    256 events;
  * "b": 1 048 576 destinations, 65 536 topics of 64 (4 194 304 listings),
    4096 closed connections, 41 943 events.
The events are half JOINs of pairs the table does not list, half LEAVEs of pairs
it does.  Per repetition, from one process:
  a. hvws_subs_update: the device span of the whole call (the host's round trip
     for its one wait is inside it) and the device time after the wait
     (hvws_last_kernel_ms: the placement);
  b. hvws_d2d of both arrays of the finished table: the table read and written
     once, the floor of any pass that produces a second table;
  c. hvws_h2d of the finished arrays from pinned memory: what the caller does
     today after rebuilding the table on the host, with the rebuild and the read
     of the reply flags left out -- a lower bound that favours the host.
Check: both output arrays against the table computed here with numpy, and the
four counts.

REPS sets the repetitions.  Prints one JSON line.
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

SHAPES = {
    # name: (ndest, ntopics, row, closed, events)
    "a": (4096, 4096, 16, 64, 256),
    "b": (1 << 20, 1 << 16, 64, 4096, 41943),
}
TEXT = np.array([0x81, 0x82, 0, 0, 0, 0, ord("h"), ord("i")], np.uint8)       # masked (key 0) FIN text "hi"
CLOSE = np.array([0x88, 0x82, 0, 0, 0, 0, 0x03, 0xE8], np.uint8)              # masked FIN CLOSE 1000


def span(eng, fn):
    L = libhv_amd.lib()
    ms = ctypes.c_float(0)
    eng.sync()
    libhv_amd._check(L.hvws_span_begin(eng.ctx), "span_begin")
    fn()
    libhv_amd._check(L.hvws_span_end(eng.ctx, ctypes.byref(ms)), "span_end")
    return float(ms.value)


def table(ndest, ntopics, row, rng):
    """Row t lists `row` distinct destinations: a random start, a stride of ndest / row."""
    start = rng.integers(0, ndest, ntopics, dtype=np.int64)
    member = (start[:, None] + np.arange(row, dtype=np.int64)[None, :] * (ndest // row)) % ndest
    return np.arange(ntopics + 1, dtype=np.uint64) * row, member.astype(np.uint32).ravel()


def expected(first, member, ntopics, closed, events):
    """The new table with numpy: no DROP events, every JOIN pair new, every LEAVE pair listed once."""
    row_of = np.repeat(np.arange(ntopics, dtype=np.int64), np.diff(first.astype(np.int64)))
    pair = (row_of << 32) | member.astype(np.int64)
    ev_pair = (events["topic"].astype(np.int64) << 32) | events["dest"].astype(np.int64)
    leave = ev_pair[events["op"] == libhv_amd.SUB_LEAVE]
    join = np.sort(ev_pair[events["op"] == libhv_amd.SUB_JOIN])
    keep = ~np.isin(member, closed) & ~np.isin(pair, leave)
    kept_n = np.bincount(row_of[keep], minlength=ntopics)
    join_n = np.bincount(join >> 32, minlength=ntopics)
    new_first = np.concatenate(([0], np.cumsum(kept_n + join_n)))
    out = np.zeros(int(new_first[-1]), np.uint32)
    kept_before = np.concatenate(([0], np.cumsum(kept_n)))
    k = np.flatnonzero(keep)
    out[new_first[row_of[k]] + (np.arange(len(k)) - kept_before[row_of[k]])] = member[k]
    jt = join >> 32
    join_before = np.concatenate(([0], np.cumsum(join_n)))
    out[new_first[jt] + kept_n[jt] + (np.arange(len(join)) - join_before[jt])] = (join & 0xFFFFFFFF).astype(np.uint32)
    return new_first.astype(np.uint64), out, (int(keep.sum()), len(join), int((~keep).sum()), len(np.unique(closed)))


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "a"
    ndest, ntopics, row, nclosed, nev = SHAPES[name]
    reps = int(os.environ.get("REPS", "5"))
    L = libhv_amd.lib()
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    rng = np.random.default_rng(20 + ord(name))
    first, member = table(ndest, ntopics, row, rng)
    nmember = len(member)
    # the turn: 2 * nclosed connections of one frame each, every second one CLOSEs
    nseg = 2 * nclosed
    dest_of = rng.choice(ndest, nseg, replace=False).astype(np.uint32)
    data = np.concatenate([CLOSE if s & 1 else TEXT for s in range(nseg)])
    segs = [(8 * s, 8) for s in range(nseg)]
    rx, msg = eng.to_device(data), eng.alloc(len(data) + 64)
    eng.scan(rx, len(data), segs)
    eng.messages_rfc(rx, len(data), True, msg, len(data))
    eng.replies(libhv_amd.R_SERVER | libhv_amd.R_ECHO)
    flags = eng.reply_flags(nseg)
    assert ((flags & libhv_amd.RF_CLOSED) != 0).tolist() == [bool(s & 1) for s in range(nseg)]
    closed = dest_of[1::2]
    # the events: LEAVEs of listed pairs (distinct listings), JOINs of pairs no row lists
    events = np.zeros(nev, libhv_amd.SUB_EVENT_DTYPE)
    nl = nev // 2
    at = rng.choice(nmember, nl, replace=False)
    events["op"][:nl], events["topic"][:nl], events["dest"][:nl] = libhv_amd.SUB_LEAVE, at // row, member[at]
    jt = rng.choice(ntopics, nev - nl, replace=ntopics < nev - nl)
    # one past a listed destination: the stride between a row's members is ndest / row > 1
    jd = (member[jt.astype(np.int64) * row] + 1 + 2 * (np.arange(nev - nl) % max(1, (ndest // row - 1) // 2))) % ndest
    events["op"][nl:], events["topic"][nl:], events["dest"][nl:] = libhv_amd.SUB_JOIN, jt, jd
    jp = (events["topic"][nl:].astype(np.int64) << 32) | events["dest"][nl:]
    assert len(np.unique(jp)) == len(jp), "the JOIN pairs are distinct"
    events = events[rng.permutation(nev)]
    want_first, want_member, want_counts = expected(first, member, ntopics, closed, events)
    newn = len(want_member)
    d_first, d_member = eng.to_device(first), eng.to_device(member)
    o_first, o_member = eng.alloc(8 * (ntopics + 1) + 64), eng.alloc(4 * newn + 64)
    c_first, c_member = eng.alloc(8 * (ntopics + 1) + 64), eng.alloc(4 * newn + 64)
    fb, mb = 8 * (ntopics + 1), 4 * newn
    pin = L.hvws_host_alloc(eng.ctx, fb + mb + 64)
    assert pin
    ctypes.memmove(pin, want_first.ctypes.data, fb)
    ctypes.memmove(pin + fb, want_member.ctypes.data, mb)

    def update():
        return eng.subs_update(d_first, d_member, ntopics, nmember, ndest, events, dest_of, o_first, o_member, newn)

    def d2d():
        libhv_amd._check(L.hvws_d2d(eng.ctx, c_first.ptr, o_first.ptr, fb), "hvws_d2d")
        libhv_amd._check(L.hvws_d2d(eng.ctx, c_member.ptr, o_member.ptr, mb), "hvws_d2d")

    def h2d():
        libhv_amd._check(L.hvws_h2d(eng.ctx, c_first.ptr, pin, fb), "hvws_h2d")
        libhv_amd._check(L.hvws_h2d(eng.ctx, c_member.ptr, pin + fb, mb), "hvws_h2d")

    assert update() == newn
    assert eng.subs_counts() == want_counts, (eng.subs_counts(), want_counts)
    assert np.array_equal(o_first.download(fb, np.uint64), want_first), "topic_first_out differs from the host's table"
    assert np.array_equal(o_member.download(mb, np.uint32), want_member), "member_out differs from the host's table"
    call, post, copy, up = [], [], [], []
    for _ in range(reps + 1):
        call.append(span(eng, update))
        post.append(eng.last_kernel_ms())
        copy.append(span(eng, d2d))
        up.append(span(eng, h2d))
    assert np.array_equal(c_member.download(mb, np.uint32), want_member)
    med = lambda v: float(np.median(v[1:]))
    rg = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    print(json.dumps({
        "bench": "subs", "shape": name, "destinations": ndest, "topics": ntopics, "listings": nmember, "events": nev,
        "closed": nclosed, "segments": nseg, "new_listings": newn, "counts": list(want_counts), "reps": reps,
        "table_bytes": int(first.nbytes + member.nbytes), "new_table_bytes": fb + mb,
        "call_span_ms": round(med(call), 4), "call_span_range": rg(call),
        "post_wait_ms": round(med(post), 4), "post_wait_range": rg(post),
        "d2d_ms": round(med(copy), 4), "d2d_range": rg(copy),
        "h2d_pinned_ms": round(med(up), 4), "h2d_pinned_range": rg(up),
        "ratio_call_to_d2d": round(med(call) / med(copy), 3), "ratio_post_to_d2d": round(med(post) / med(copy), 3),
        "ratio_call_to_h2d": round(med(call) / med(up), 3), "ratio_post_to_h2d": round(med(post) / med(up), 3),
        "call_ns_per_listing": round(med(call) * 1e6 / nmember, 3),
        "checked": "both output arrays and the four counts against the table computed on the host",
    }), flush=True)
    eng.sync()
    L.hvws_host_free(eng.ctx, pin)
    for b in (rx, msg, d_first, d_member, o_first, o_member, c_first, c_member):
        b.free()
    eng.close()


if __name__ == "__main__":
    main()
