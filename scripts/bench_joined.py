#!/usr/bin/env python3
"""hvws_messages_joined measurement, against hvws_messages in the same run.

1. Nothing carried.  The c3 (1M x 64 KiB frames) and c2 (1M x 1 KiB frames)
   shapes of scripts/bench_messages.py, 4096 segments, still masked after one
   hvws_scan: hvws_messages and hvws_messages_joined (state_in, d_prev and
   prev_off NULL) alternate on the same batch, REPS times each, device time of
   each pass (hvws_last_kernel_ms), with hvws_messages' own min-max spread as
   the margin.  The joined pass must give one complete piece per frame, the
   same byte total, and its first and last MiB of d_out must equal the frames'
   payloads as a later step leaves them in the batch -- on the c3 shape
   (68.7 GB) the only check of the joined form's 64-bit offsets beyond 4 GiB:
   the test suite stays below 1 MiB.
2. The event-loop shape.  4096 connections, each reading 8 KiB per batch from
   a stream of masked 64 KiB messages, connection s starting s % 8 batches
   late, so that in the steady state the segments carry 0-56 KiB each.  The
   chain runs over two alternating output buffers, parser carry, message state
   and carry offset threaded per connection.  Per measured batch, alternating:
   hvws_messages on the batch (pieces; the yardstick) and
   hvws_messages_joined (whole messages), with the bytes each reads plus writes
   and the TB/s; then the device span of the whole turn (scan + joined pass +
   hvws_replies + hvws_send_messages) against scan + joined pass alone.  Every
   complete message must be 65 536 bytes, nothing deferred, and sampled
   messages are compared with the stream's payloads.

FRAMES_C3 / FRAMES_C2 shrink the first part (0 skips a shape), LOOP_SEGS the
second (0 skips it); REPS sets the repetitions.  Prints JSON lines.
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
from bench_messages import ends_of, payload_ends, span  # noqa: E402

NSEG = 4096
READ = 8192
MSG = 65536
M_END = 1 << 4
RF_DEFERRED = 2

med = lambda v: float(np.median(v))
rng_of = lambda v: [round(min(v), 4), round(max(v), 4)]


def nothing_carried(eng, name, frames, payload, reps):
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
    plain, joined = [], []
    for i in range(reps + 1):
        eng.messages(rx, p.total, True, out, p.total)
        plain.append(eng.last_kernel_ms())
        eng.messages_joined(rx, p.total, True, out, p.total)
        joined.append(eng.last_kernel_ms())
    assert eng.msg_bytes() == want_bytes and L.hvws_msg_count(eng.ctx) == p.n, f"{name}: totals of the joined pass"
    st = eng.msg_state(nseg)
    assert not st["open"].any() and not eng.msg_carry(nseg).any(), f"{name}: a message left open"
    head, tail = ends_of(eng, out, want_bytes)
    eng.step(rx, p.total, eng.prepare(p.segments))   # unmasks the batch in place
    want_head, want_tail = payload_ends(eng, rx, p, payload)
    assert np.array_equal(head, want_head) and np.array_equal(tail, want_tail), f"{name}: ends of d_out"
    L.hvws_set_run(eng.ctx, old_run)
    plain, joined = plain[1:], joined[1:]
    row = {
        "bench": "joined_nothing_carried", "shape": name, "frames": p.n, "payload": payload, "segments": nseg,
        "payload_bytes": want_bytes, "reps": reps,
        "messages_ms": round(med(plain), 4), "messages_range": rng_of(plain),
        "joined_ms": round(med(joined), 4), "joined_range": rng_of(joined),
        "ratio": round(med(joined) / med(plain), 4),
        "inside_messages_spread": bool(min(plain) <= med(joined) <= max(plain)),
        "checked": "piece and byte counts; first and last MiB of d_out against the frames' payloads"
                   + (" (the only check of offsets beyond 4 GiB)" if want_bytes > 4 << 30 else ""),
    }
    print(json.dumps(row), flush=True)
    for b in (rx, out):
        b.free()
    dp.free()


def stream_of(nmsg: int):
    """nmsg masked binary FIN frames of 64 KiB -> (stream bytes, payloads)."""
    r = np.random.default_rng(8)
    pay = r.integers(0, 256, (nmsg, MSG), dtype=np.uint8)
    keys = r.integers(1, 256, (nmsg, 4), dtype=np.uint8)
    hdr = np.zeros((nmsg, 14), np.uint8)
    hdr[:, 0], hdr[:, 1] = 0x82, 0xFF
    hdr[:, 2:10] = np.frombuffer(MSG.to_bytes(8, "big"), np.uint8)
    hdr[:, 10:14] = keys
    body = pay ^ np.tile(keys, (1, MSG // 4))
    return np.concatenate([hdr, body], axis=1).reshape(-1), pay


def event_loop(eng, nseg, reps):
    L = libhv_amd.lib()
    warm = 8                               # batches until every connection reads
    nbatch = warm + reps + 1
    stream, pay = stream_of((nbatch * READ) // (MSG + 14) + 2)
    rx_len = nseg * READ
    cap = rx_len + nseg * (MSG + READ)     # a batch and the most that can be pending
    rx = eng.alloc(rx_len + 64)
    outs = [eng.alloc(cap + 64), eng.alloc(cap + 64)]
    tx = eng.alloc(cap + 64)
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    carries, state, off = None, None, np.zeros(nseg, np.uint64)
    done = np.zeros(nseg, np.int64)        # messages each connection has completed
    prev_len = 0
    t_plain, t_join, t_rx, t_turn, rows = [], [], [], [], []
    for k in range(nbatch):
        # connection s reads the stream's bytes from (k - s % 8) * READ on, nothing before its start
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
        cur, old = outs[k % 2], outs[(k + 1) % 2]
        measured = k >= warm + 1
        eng.scan(rx, at, segs, carries)
        if measured:       # the yardstick on the same batch: pieces only, the host would join them
            eng.messages(rx, at, True, cur, cap, state)
            t_plain.append(eng.last_kernel_ms())
            new_bytes = eng.msg_bytes()
        eng.messages_joined(rx, at, True, cur, cap, state, old if k else None, prev_len, off)
        if measured:
            t_join.append(eng.last_kernel_ms())
            total = eng.msg_bytes()
            rows.append((new_bytes, total))
            t_rx.append(span(eng, lambda: (eng.scan(rx, at, segs, carries),
                                           eng.messages_joined(rx, at, True, cur, cap, state, old, prev_len, off))))

            def turn():
                eng.scan(rx, at, segs, carries)
                eng.messages_joined(rx, at, True, cur, cap, state, old, prev_len, off)
                eng.replies(policy)
                table, d_n, n = eng.replies_device()
                return eng.send_messages(tx, cap + 64, cur, cap, table, n, d_n, 0, False)

            t_turn.append(span(eng, turn))
            assert not (eng.reply_flags(nseg) & RF_DEFERRED).any(), "a reply was deferred"
        # thread the chain on
        table = eng.message_table()
        first, count = eng.segment_messages(nseg)
        ends = table[(table["info"] & M_END) != 0]
        assert (ends["len"] == MSG).all() and (table["total"] == table["len"]).all(), "a complete message is 64 KiB"
        for s in (0, nseg // 2 + 3, nseg - 1):   # sampled connections: their messages are the stream's
            for pce in table[int(first[s]): int(first[s]) + int(count[s])]:
                if int(pce["info"]) & M_END:
                    got = np.empty(MSG, np.uint8)
                    libhv_amd._check(L.hvws_d2h(eng.ctx, got.ctypes.data, cur.ptr + int(pce["off"]), MSG), "hvws_d2h")
                    eng.sync()
                    assert np.array_equal(got, pay[done[s]]), f"batch {k}, connection {s}: message bytes"
        np.add.at(done, ends["seg"].astype(np.int64), 1)
        carries, _ = eng.carry(nseg)
        state, off = eng.msg_state(nseg), eng.msg_carry(nseg)
        prev_len = eng.msg_bytes()
    assert done.sum() > 0
    new_b, tot_b = med([r[0] for r in rows]), med([r[1] for r in rows])
    row = {
        "bench": "joined_event_loop", "segments": nseg, "read": READ, "message": MSG, "batches_measured": len(rows),
        "payload_bytes": int(new_b), "carried_bytes": int(tot_b - new_b),
        "joined_ms": round(med(t_join), 4), "joined_range": rng_of(t_join),
        "joined_read_plus_written": int(2 * tot_b), "joined_TBps": round(2 * tot_b / med(t_join) / 1e9, 3),
        "messages_ms": round(med(t_plain), 4), "messages_range": rng_of(t_plain),
        "messages_read_plus_written": int(2 * new_b), "messages_TBps": round(2 * new_b / med(t_plain) / 1e9, 3),
        "span_scan_joined_ms": round(med(t_rx), 4), "span_turn_ms": round(med(t_turn), 4),
        "messages_completed": int(done.sum()),
        "checked": "every complete message is 64 KiB and total == len; sampled messages against the stream; "
                   "no segment deferred",
    }
    print(json.dumps(row), flush=True)
    for b in [rx, tx] + outs:
        b.free()


def main():
    reps = int(os.environ.get("REPS", "7"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 20)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    nl = int(os.environ.get("LOOP_SEGS", str(NSEG)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    if n3:
        nothing_carried(eng, "c3", n3, 65536, reps)
    if n2:
        nothing_carried(eng, "c2", n2, 1024, reps)
    if nl:
        event_loop(eng, nl, reps)
    eng.close()


if __name__ == "__main__":
    main()
