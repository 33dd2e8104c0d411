#!/usr/bin/env python3
"""hvws_messages_rfc measurement, against hvws_messages_joined on the same
batch in the same run (never against an earlier figure).

1. No control frames, nothing carried.  The c3 (1M x 64 KiB frames) and c2
   (1M x 1 KiB frames) shapes of scripts/bench_messages.py, 4096 segments,
   still masked after one hvws_scan: hvws_messages_joined and
   hvws_messages_rfc (state_in and d_prev NULL) alternate on the same batch,
   REPS times each, device time of each pass (hvws_last_kernel_ms), with the
   joined form's own min-max spread as the margin.  The rfc pass must give one
   complete piece per frame, the same byte total, no control piece, and its
   first and last MiB of d_out must equal the frames' payloads.
2. The event-loop shape of scripts/bench_joined.py with a masked PING between
   the fragments of every message: 4096 connections, each reading 8 KiB per
   batch from a stream of 64 KiB binary messages sent as two 32 KiB fragments
   with a 16-byte PING between them, connection s starting s % 8 batches late.
   Each form runs its own chain over its own two alternating output buffers
   (the joined form delivers this traffic as libhv does, the PING inside the
   message); per measured batch the two passes alternate.  Then the device span
   of the whole rfc turn (scan + rfc pass + hvws_replies + hvws_send_messages).
   Every complete data message of the rfc form must be 65 536 bytes and every
   control message the PING's 16, nothing deferred, and sampled messages are
   compared with the stream's payloads.

FRAMES_C3 / FRAMES_C2 shrink the first part (0 skips a shape), LOOP_SEGS the
second (0 skips it); REPS sets the repetitions.  Prints JSON lines.
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
from bench_messages import ends_of, payload_ends, span  # noqa: E402

NSEG = 4096
READ = 8192
MSG = 65536
HALF = MSG // 2
PING = 16
M_END, M_CTL = 1 << 4, 1 << 6
RF_DEFERRED = 2

med = lambda v: float(np.median(v))
rng_of = lambda v: [round(min(v), 4), round(max(v), 4)]


def no_control_frames(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    out = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    nseg = len(p.segments)
    want_bytes = p.n * payload
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    joined, rfc = [], []
    for i in range(reps + 1):
        eng.messages_joined(rx, p.total, True, out, p.total)
        joined.append(eng.last_kernel_ms())
        eng.messages_rfc(rx, p.total, True, out, p.total)
        rfc.append(eng.last_kernel_ms())
    assert eng.msg_bytes() == want_bytes and L.hvws_msg_count(eng.ctx) == p.n, f"{name}: totals of the rfc pass"
    st = eng.rfc_state(nseg)
    assert not st["data"]["open"].any() and not st["ctl"]["open"].any() and not st["data_off"].any(), \
        f"{name}: a message left open"
    table = eng.message_table()
    assert not (table["info"] & M_CTL).any() and ((table["info"] & M_END) != 0).all(), f"{name}: pieces"
    del table
    head, tail = ends_of(eng, out, want_bytes)
    eng.step(rx, p.total, eng.prepare(p.segments))   # unmasks the batch in place
    want_head, want_tail = payload_ends(eng, rx, p, payload)
    assert np.array_equal(head, want_head) and np.array_equal(tail, want_tail), f"{name}: ends of d_out"
    L.hvws_set_run(eng.ctx, old_run)
    joined, rfc = joined[1:], rfc[1:]
    row = {
        "bench": "rfc_no_control_frames", "shape": name, "frames": p.n, "payload": payload, "segments": nseg,
        "payload_bytes": want_bytes, "reps": reps,
        "joined_ms": round(med(joined), 4), "joined_range": rng_of(joined),
        "rfc_ms": round(med(rfc), 4), "rfc_range": rng_of(rfc),
        "difference_ms": round(med(rfc) - med(joined), 4), "ratio": round(med(rfc) / med(joined), 4),
        "inside_joined_spread": bool(min(joined) <= med(rfc) <= max(joined)),
        "checked": "piece and byte counts, no control piece; first and last MiB of d_out against the frames' payloads"
                   + (" (the only check of offsets beyond 4 GiB)" if want_bytes > 4 << 30 else ""),
    }
    print(json.dumps(row), flush=True)
    for b in (rx, out):
        b.free()
    dp.free()


def stream_of(nmsg: int):
    """nmsg masked binary messages of 64 KiB, each two 32 KiB fragments with a
    masked 16-byte PING between them -> (stream bytes, payloads, ping payloads)."""
    r = np.random.default_rng(8)
    pay = r.integers(0, 256, (nmsg, MSG), dtype=np.uint8)
    ping = r.integers(0, 256, (nmsg, PING), dtype=np.uint8)
    keys = r.integers(1, 256, (nmsg, 3, 4), dtype=np.uint8)

    def frame(b0, body, key):
        n = body.shape[1]
        if n < 126:
            hdr = np.zeros((nmsg, 6), np.uint8)
            hdr[:, 1] = 0x80 | n
        else:
            hdr = np.zeros((nmsg, 8), np.uint8)
            hdr[:, 1] = 0x80 | 126
            hdr[:, 2:4] = np.frombuffer(n.to_bytes(2, "big"), np.uint8)
        hdr[:, 0] = b0
        hdr[:, -4:] = key
        return [hdr, body ^ np.tile(key, (1, n // 4))]

    parts = (frame(0x02, pay[:, :HALF], keys[:, 0]) + frame(0x89, ping, keys[:, 1])
             + frame(0x80, pay[:, HALF:], keys[:, 2]))
    return np.concatenate(parts, axis=1).reshape(-1), pay, ping


def event_loop(eng, nseg, reps):
    L = libhv_amd.lib()
    warm = 8                               # batches until every connection reads
    nbatch = warm + reps + 1
    per_msg = MSG + 8 + 8 + 6 + PING
    stream, pay, ping = stream_of((nbatch * READ) // per_msg + 2)
    rx_len = nseg * READ
    cap = rx_len + nseg * (MSG + READ)     # a batch and the most that can be pending
    rx = eng.alloc(rx_len + 64)
    jouts = [eng.alloc(cap + 64), eng.alloc(cap + 64)]
    routs = [eng.alloc(cap + 64), eng.alloc(cap + 64)]
    tx = eng.alloc(cap + 64)
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    carries = None
    jstate, joff, jprev = None, np.zeros(nseg, np.uint64), 0
    rstate, rprev = None, 0
    done = np.zeros(nseg, np.int64)        # data messages each connection has completed
    pings = np.zeros(nseg, np.int64)
    t_join, t_rfc, t_rx, t_turn, rows = [], [], [], [], []
    for k in range(nbatch):
        lens = np.array([READ if k >= s % 8 else 0 for s in range(nseg)], np.int64)
        segs, at, parts = [], 0, []
        for s in range(nseg):
            segs.append((at, int(lens[s])))
            at += int(lens[s])
        for j in range(min(8, nseg)):
            if k >= j:
                parts.append(stream[(k - j) * READ:(k - j + 1) * READ])
        group = np.concatenate(parts)
        data = np.concatenate([group] * (nseg // 8)) if nseg >= 8 else group[:at]
        assert data.nbytes == at
        rx.upload(data)
        jcur, jold = jouts[k % 2], jouts[(k + 1) % 2]
        rcur, rold = routs[k % 2], routs[(k + 1) % 2]
        measured = k >= warm + 1
        eng.scan(rx, at, segs, carries)
        # the yardstick on the same batch: the joined form's own chain
        eng.messages_joined(rx, at, True, jcur, cap, jstate, jold if k else None, jprev, joff)
        if measured:
            t_join.append(eng.last_kernel_ms())
        jtotal = eng.msg_bytes()
        jstate, joff, jprev = eng.msg_state(nseg), eng.msg_carry(nseg), jtotal
        eng.messages_rfc(rx, at, True, rcur, cap, rstate, rold if k else None, rprev)
        if measured:
            t_rfc.append(eng.last_kernel_ms())
            rows.append((jtotal, eng.msg_bytes()))
            t_rx.append(span(eng, lambda: (eng.scan(rx, at, segs, carries),
                                           eng.messages_rfc(rx, at, True, rcur, cap, rstate, rold, rprev))))

            def turn():
                eng.scan(rx, at, segs, carries)
                eng.messages_rfc(rx, at, True, rcur, cap, rstate, rold, rprev)
                eng.replies(policy)
                table, d_n, n = eng.replies_device()
                return eng.send_messages(tx, cap + 64, rcur, cap, table, n, d_n, 0, False)

            t_turn.append(span(eng, turn))
            assert not (eng.reply_flags(nseg) & RF_DEFERRED).any(), "a reply was deferred"
        # thread the rfc chain on
        table = eng.message_table()
        first, count = eng.segment_messages(nseg)
        ends = table[(table["info"] & M_END) != 0]
        ctl = (ends["info"] & M_CTL) != 0
        assert (ends["len"][~ctl] == MSG).all() and (ends["len"][ctl] == PING).all(), "message lengths"
        assert (table["total"] == table["len"]).all()
        for s in (0, nseg // 2 + 3, nseg - 1):   # sampled connections: their messages are the stream's
            nd, nc = int(done[s]), int(pings[s])
            for pce in table[int(first[s]): int(first[s]) + int(count[s])]:
                if not int(pce["info"]) & M_END:
                    continue
                n = int(pce["len"])
                got = np.empty(n, np.uint8)
                libhv_amd._check(L.hvws_d2h(eng.ctx, got.ctypes.data, rcur.ptr + int(pce["off"]), n), "hvws_d2h")
                eng.sync()
                if int(pce["info"]) & M_CTL:
                    assert np.array_equal(got, ping[nc]), f"batch {k}, connection {s}: ping bytes"
                    nc += 1
                else:
                    assert np.array_equal(got, pay[nd]), f"batch {k}, connection {s}: message bytes"
                    nd += 1
        np.add.at(done, ends["seg"][~ctl].astype(np.int64), 1)
        np.add.at(pings, ends["seg"][ctl].astype(np.int64), 1)
        carries, _ = eng.carry(nseg)
        rstate, rprev = eng.rfc_state(nseg), eng.msg_bytes()
    assert done.sum() > 0 and pings.sum() > 0
    jb, rb = med([r[0] for r in rows]), med([r[1] for r in rows])
    row = {
        "bench": "rfc_event_loop", "segments": nseg, "read": READ, "message": MSG, "ping": PING,
        "batches_measured": len(rows), "rx_bytes": int(rx_len),
        "joined_ms": round(med(t_join), 4), "joined_range": rng_of(t_join), "joined_out_bytes": int(jb),
        "rfc_ms": round(med(t_rfc), 4), "rfc_range": rng_of(t_rfc), "rfc_out_bytes": int(rb),
        "difference_ms": round(med(t_rfc) - med(t_join), 4), "ratio": round(med(t_rfc) / med(t_join), 4),
        "span_scan_rfc_ms": round(med(t_rx), 4), "span_turn_ms": round(med(t_turn), 4),
        "messages_completed": int(done.sum()), "pings_completed": int(pings.sum()),
        "checked": "every complete data message is 64 KiB, every control message the PING's 16 bytes, total == len; "
                   "sampled messages and pings against the stream; no segment deferred",
    }
    print(json.dumps(row), flush=True)
    for b in [rx, tx] + jouts + routs:
        b.free()


def main():
    reps = int(os.environ.get("REPS", "7"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 20)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    nl = int(os.environ.get("LOOP_SEGS", str(NSEG)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    if n3:
        no_control_frames(eng, "c3", n3, 65536, reps)
    if n2:
        no_control_frames(eng, "c2", n2, 1024, reps)
    if nl:
        event_loop(eng, nl, reps)
    eng.close()


if __name__ == "__main__":
    main()
