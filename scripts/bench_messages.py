#!/usr/bin/env python3
"""hvws_messages measurement: message reassembly on the device against the
unmask of the same batch.

Two shapes on one card, device resident, 4096 segments of masked FIN frames:
  * "c3": 1M x 64 KiB frames (BASELINE config 3's shape);
  * "c2": 1M x 1 KiB frames (config 2's shape).
For each, from the same run:
  * the pass's device time (hvws_last_kernel_ms: table pass, tile index and
    gather) on the still-masked batch after hvws_scan (masked = 1: the XOR
    happens in registers, the batch is never unmasked in place) and on the
    unmasked batch after hvws_step (masked = 0), with the GB/s it moves
    (payload read + payload written);
  * k_unmask's device time on that batch (hvws_last_times) -- the yardstick: it
    moves the same bytes, in place;
  * the end-to-end device span (hvws_span_begin / hvws_span_end) of scan + pass
    against step + pass: one read and one write of the payload against two.
Every frame must come out as one complete piece and the payload total must be
frames x payload (asserted).  The first and the last MiB of d_out are
downloaded after both passes and compared with the payloads of the first and
last frames as the step leaves them in the batch.  On the c3 shape (68.7 GB)
that comparison of the last MiB is the only check of the pass's 64-bit offsets
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


def fetch(eng, buf, off, n):
    out = np.empty(n, np.uint8)
    libhv_amd._check(libhv_amd.lib().hvws_d2h(eng.ctx, out.ctypes.data, buf.ptr + off, n), "hvws_d2h")
    eng.sync()
    return out


def ends_of(eng, out, total):
    n = min(MIB, total)
    return fetch(eng, out, 0, n), fetch(eng, out, total - n, n)


def payload_ends(eng, rx, p, payload):
    """The first and last MiB of payload as they lie, unmasked, in the batch."""
    k = min(p.n, (MIB + payload - 1) // payload)
    size = int(p.frame_off[1] - p.frame_off[0]) if p.n > 1 else p.total
    hdr = size - payload
    n = min(MIB, p.n * payload)

    def strip(first):
        raw = fetch(eng, rx, int(p.frame_off[first]), k * size).reshape(k, size)
        return raw[:, hdr:].reshape(-1)

    return strip(0)[:n], strip(p.n - k)[-n:]


def span(eng, fn):
    L = libhv_amd.lib()
    ms = ctypes.c_float(0)
    eng.sync()   # the span's begin markers go on both compute streams: nothing may still run on either
    libhv_amd._check(L.hvws_span_begin(eng.ctx), "span_begin")
    fn()
    libhv_amd._check(L.hvws_span_end(eng.ctx, ctypes.byref(ms)), "span_end")
    return float(ms.value)


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    out = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    nseg = len(p.segments)
    segs = eng.prepare(p.segments)
    want_bytes = p.n * payload
    old_run = L.hvws_set_run(eng.ctx, 0)   # the yardstick is k_unmask itself, not the RUN path's

    def check_counts(what):
        assert eng.msg_bytes() == want_bytes, f"{what}: payload total"
        assert L.hvws_msg_count(eng.ctx) == p.n, f"{what}: one piece per frame"
        st = eng.msg_state(nseg)
        assert not st["open"].any() and not st["pending"].any(), f"{what}: a message left open"

    # still masked, after a scan
    eng.scan(rx, p.total, p.segments)
    m_masked = []
    for _ in range(reps + 1):
        eng.messages(rx, p.total, True, out, p.total)
        m_masked.append(eng.last_kernel_ms())
    check_counts(name + " masked")
    head1, tail1 = ends_of(eng, out, want_bytes)
    assert eng.synth(rx, p.total, p.seed, dp, 1) == 0, "the masked pass changed the batch"
    # unmasked, after a step; an odd number of steps leaves the batch unmasked
    unmask = []
    for _ in range(2 * (reps // 2) + 3):
        eng.step(rx, p.total, segs)
        unmask.append(eng.last_times()[1])
    m_plain = []
    for _ in range(reps + 1):
        eng.messages(rx, p.total, False, out, p.total)
        m_plain.append(eng.last_kernel_ms())
    check_counts(name + " unmasked")
    head0, tail0 = ends_of(eng, out, want_bytes)
    want_head, want_tail = payload_ends(eng, rx, p, payload)
    for what, got, want in (("masked head", head1, want_head), ("masked tail", tail1, want_tail),
                            ("unmasked head", head0, want_head), ("unmasked tail", tail0, want_tail)):
        assert np.array_equal(got, want), f"{name}: {what} of d_out differs from the frames' payloads"
    # end to end: scan + pass on masked bytes against step + pass; a step in
    # between puts the mask back (XOR twice), untimed
    eng.step(rx, p.total, segs)
    e_scan, e_step = [], []
    for _ in range(reps + 1):
        e_scan.append(span(eng, lambda: (eng.scan(rx, p.total, p.segments),
                                         eng.messages(rx, p.total, True, out, p.total))))
        e_step.append(span(eng, lambda: (eng.step(rx, p.total, segs),
                                         eng.messages(rx, p.total, False, out, p.total))))
        eng.step(rx, p.total, segs)
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    mm, mp, um = med(m_masked), med(m_plain), med(unmask)
    row = {
        "bench": "messages", "shape": name, "frames": p.n, "payload": payload, "segments": nseg, "bytes": p.total,
        "payload_bytes": want_bytes,
        "msg_ms_masked": round(mm, 4), "msg_GBps_masked": round(2 * want_bytes / mm / 1e6, 1),
        "msg_ms_unmasked": round(mp, 4), "msg_GBps_unmasked": round(2 * want_bytes / mp / 1e6, 1),
        "unmask_ms": round(um, 4), "unmask_kernel": L.hvws_unmask_kernel_name_for(p.total).decode(),
        "ratio_masked": round(mm / um, 3), "ratio_unmasked": round(mp / um, 3),
        "span_scan_pass_ms": round(med(e_scan), 4), "span_step_pass_ms": round(med(e_step), 4),
        "checked": "piece and byte counts; first and last MiB of d_out against the frames' payloads"
                   + (" (the only check of offsets beyond 4 GiB)" if want_bytes > 4 << 30 else ""),
    }
    print(json.dumps(row), flush=True)
    for b in (rx, out):
        b.free()
    dp.free()


def main():
    reps = int(os.environ.get("REPS", "9"))
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
