#!/usr/bin/env python3
"""hvws_utf8 measurement: the UTF-8 pass against the unmask of the same batch.

Two shapes on one card, device resident, both of masked FIN text frames whose
payloads are printable ASCII (hvws_synth's text payloads):
  * "c3": 1M x 64 KiB frames (BASELINE config 3's shape);
  * "c2": 1M x 1 KiB frames (config 2's shape).
For each, from the same run: the pass's device time (hvws_last_kernel_ms: its
tile index and all three kernels) on the still-masked batch after hvws_scan
(the XOR happens in registers) and on the unmasked batch after hvws_step, the
GB/s it reads, and k_unmask's device time on that batch (hvws_last_times).
The yardstick is the unmask: the pass reads what it reads and writes almost
nothing.  Every verdict must be HVWS_U8_NONE (asserted).

A third row, "c2_multibyte", runs the pass over unmasked 1 KiB frames of
3-byte characters (no ASCII run to skip: every byte goes through the
character-boundary predicate) and is set against c2's unmask time.

FRAMES_C3 / FRAMES_C2 shrink the shapes; REPS sets the repetitions.  Prints
JSON lines.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import libhv_amd  # noqa: E402
from libhv_amd import synth  # noqa: E402

U8_NONE = (1 << 64) - 1
NSEG = 4096


def timed_pass(eng, rx, total, masked, reps):
    ms = []
    for _ in range(reps + 1):
        eng.utf8(rx, total, masked)
        ms.append(eng.last_kernel_ms())
    return float(np.median(ms[1:]))


def check_verdicts(eng, nseg, what):
    st, bad = eng.utf8_result(nseg)
    assert np.all(bad == np.uint64(U8_NONE)), f"{what}: a verdict on valid text (first at segment {int(np.argmax(bad != np.uint64(U8_NONE)))})"
    assert np.all(st == 0), f"{what}: a message left open at a frame boundary"


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1, opcode=synth.OP_TEXT, text=True).split(NSEG)
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    nseg = len(p.segments)
    segs = eng.prepare(p.segments)
    old_run = L.hvws_set_run(eng.ctx, 0)   # the yardstick is k_unmask itself, not the RUN path's
    eng.scan(rx, p.total, p.segments)
    u8_masked = timed_pass(eng, rx, p.total, True, reps)
    check_verdicts(eng, nseg, name + " masked")
    assert eng.synth(rx, p.total, p.seed, dp, 1) == 0, "the pass changed the batch"
    unmask = []
    for _ in range(2 * (reps // 2) + 3):   # odd: the batch ends up unmasked
        eng.step(rx, p.total, segs)
        unmask.append(eng.last_times()[1])
    unmask_ms = float(np.median(unmask[1:]))
    u8_plain = timed_pass(eng, rx, p.total, False, reps)
    check_verdicts(eng, nseg, name + " unmasked")
    L.hvws_set_run(eng.ctx, old_run)
    row = {
        "bench": "utf8", "shape": name, "frames": p.n, "payload": payload, "segments": nseg, "bytes": p.total,
        "utf8_ms_masked": round(u8_masked, 4), "utf8_GBps_masked": round(p.total / u8_masked / 1e6, 1),
        "utf8_ms_unmasked": round(u8_plain, 4), "utf8_GBps_unmasked": round(p.total / u8_plain / 1e6, 1),
        "unmask_ms": round(unmask_ms, 4), "unmask_kernel": L.hvws_unmask_kernel_name_for(p.total).decode(),
        "ratio_masked": round(u8_masked / unmask_ms, 3), "ratio_unmasked": round(u8_plain / unmask_ms, 3),
        "verdicts": "all HVWS_U8_NONE",
    }
    print(json.dumps(row), flush=True)
    rx.free()
    dp.free()
    return unmask_ms


def multibyte(eng, frames, payload, reps, unmask_ms):
    text = ("\u20ac" * (payload // 3) + "a" * (payload % 3)).encode()
    assert len(text) == payload and 126 <= payload <= 0xFFFF
    frame = np.frombuffer(bytes([0x81, 126]) + payload.to_bytes(2, "big") + text, dtype=np.uint8)
    per = frames // NSEG
    frames = per * NSEG
    host = np.tile(frame, frames)
    rx = eng.to_device(host)
    total = host.nbytes
    del host
    segs = [(s * per * len(frame), per * len(frame)) for s in range(NSEG)]
    eng.scan(rx, total, segs)
    ms = timed_pass(eng, rx, total, False, reps)
    check_verdicts(eng, NSEG, "c2_multibyte")
    print(json.dumps({
        "bench": "utf8", "shape": "c2_multibyte", "frames": frames, "payload": payload, "segments": NSEG, "bytes": total,
        "utf8_ms_unmasked": round(ms, 4), "utf8_GBps_unmasked": round(total / ms / 1e6, 1),
        "c2_unmask_ms": round(unmask_ms, 4), "ratio_vs_c2_unmask": round(ms / unmask_ms * (frames * (payload + 8)) / total, 3),
        "verdicts": "all HVWS_U8_NONE",
    }), flush=True)
    rx.free()


def main():
    reps = int(os.environ.get("REPS", "9"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 20)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    shape(eng, "c3", n3, 65536, reps)
    um2 = shape(eng, "c2", n2, 1024, reps)
    multibyte(eng, n2, 1024, reps, um2)
    eng.close()


if __name__ == "__main__":
    main()
