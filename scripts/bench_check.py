#!/usr/bin/env python3
"""hvws_check measurement, against hvws_messages_rfc on the same batch in the
same run (never against an earlier figure).

The c3 (1M x 64 KiB frames) and c2 (1M x 1 KiB frames) shapes of
scripts/bench_messages.py, 4096 segments, still masked after one hvws_scan and
one hvws_utf8: hvws_messages_rfc (state_in and d_prev NULL) and hvws_check
(every class, max_message above the frames' size, state_in NULL) alternate on
the same batch, REPS times each, device time of each pass
(hvws_last_kernel_ms).  The ratio is check / rfc.

Checked on every shape: with the size class alone and max_message one byte
below the frames' payload, every connection fails at its first record with
code 1009 and nothing else in why; with every class and max_message above the
payload, a connection fails exactly when hvws_utf8 rejected it, at that
record, with code 1007.

FRAMES_C3 / FRAMES_C2 shrink a shape (0 skips it); REPS sets the repetitions.
Prints JSON lines (profiles/check_raw/ keeps them).
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

NSEG = 4096
NONE = libhv_amd.CHECK_NONE

med = lambda v: float(np.median(v))
rng_of = lambda v: [round(min(v), 4), round(max(v), 4)]


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    out = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    nseg = len(p.segments)
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.utf8(rx, p.total, True)
    _, bad = eng.utf8_result(nseg)
    first, count = eng.segment_frames(nseg)
    rfc, chk = [], []
    for i in range(reps + 1):
        eng.messages_rfc(rx, p.total, True, out, p.total)
        rfc.append(eng.last_kernel_ms())
        eng.check(libhv_amd.C_ALL, payload + 1)
        chk.append(eng.last_kernel_ms())
    st, fail, why, code = eng.check_result(nseg)
    rejected = bad != np.uint64(NONE)
    assert np.array_equal(fail, bad), f"{name}: fail_rec is hvws_utf8's bad[]"
    assert np.array_equal(why, np.where(rejected, libhv_amd.C_TEXT_UTF8, 0)), f"{name}: why"
    assert np.array_equal(code, np.where(rejected, 1007, 0)), f"{name}: code"
    assert np.array_equal((st & libhv_amd.CK_FAILED) != 0, rejected), f"{name}: state_out"
    eng.check(libhv_amd.C_SIZE, payload - 1)
    size_ms = eng.last_kernel_ms()
    st, fail, why, code = eng.check_result(nseg)
    has = count > 0
    assert np.array_equal(fail[has], first[has]) and (why[has] == libhv_amd.C_SIZE).all() and (code[has] == 1009).all(), \
        f"{name}: every connection fails at its first record"
    assert (fail[~has] == np.uint64(NONE)).all(), f"{name}: a connection without records failed"
    L.hvws_set_run(eng.ctx, old_run)
    rfc, chk = rfc[1:], chk[1:]
    row = {
        "bench": "check", "shape": name, "frames": p.n, "payload": payload, "segments": nseg, "batch_bytes": p.total,
        "reps": reps,
        "rfc_ms": round(med(rfc), 4), "rfc_range": rng_of(rfc),
        "check_ms": round(med(chk), 4), "check_range": rng_of(chk),
        "check_size_only_all_failing_ms": round(size_ms, 4),
        "ratio": round(med(chk) / med(rfc), 4),
        "connections_rejected_by_utf8": int(rejected.sum()),
        "checked": "every class: fail_rec, why, code and state_out against hvws_utf8's bad[]; the size class alone, "
                   "one byte below the payload: every connection at its first record, 1009",
    }
    print(json.dumps(row), flush=True)
    for b in (rx, out):
        b.free()
    dp.free()


def main():
    reps = int(os.environ.get("REPS", "7"))
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
