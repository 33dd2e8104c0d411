"""GPU: bench.py --dump-outputs writes what a step handed its caller -- the
frame table, the per-segment frames, the carry and the unmasked rx bytes --
whole when small, as a fixed sample when large, the same from call to call."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

import libhv_amd
from libhv_amd import synth
import wsharness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("counts", "frames", "segment_frames", "carry", "rx_offsets", "rx_sample")


@pytest.fixture(scope="module")
def stepped(eng):
    """A small mixed batch of 16 connections after one hvws_step_resident, and
    the oracle's unmasked bytes and frame count for it."""
    plan = synth.mixed_plan(3 << 20, seed=11, hi=1 << 17).split(16)
    host = H.synth_cpu(plan)
    exp = host.copy()
    nrec = 0
    for off, n in plan.segments:
        recs, _, _, out = H.scan_segment(host[off:off + n].tobytes())
        exp[off:off + n] = np.frombuffer(out, np.uint8)
        nrec += len(recs)
    dp = libhv_amd.DevicePlan(eng, plan)
    rx = eng.alloc(plan.total + 64)
    eng.synth(rx, plan.total, plan.seed, dp, 0)
    segs = eng.prepare(plan.segments)
    eng.step_resident(rx, plan.total, segs)
    yield plan, rx, segs, exp, nrec
    dp.free()
    rx.free()


def _load(d):
    return {n: np.load(os.path.join(str(d), n + ".npy")) for n in NAMES}


def test_dump_whole_when_small(eng, stepped, tmp_path):
    plan, rx, segs, exp, nrec = stepped
    info = bench.dump_outputs(eng, rx, plan, segs.n, str(tmp_path), 0, 1)
    a = _load(tmp_path)
    assert sorted(info["arrays"]) == sorted(NAMES)
    assert a["rx_sample"].dtype == np.float32 and all(a[n].dtype == np.float64 for n in NAMES[:-1])
    assert a["counts"].tolist() == [nrec, plan.total, 16]
    assert a["rx_offsets"].tolist() == [0.0] and a["rx_sample"].shape == (1, plan.total)
    assert np.array_equal(a["rx_sample"][0].astype(np.uint8), exp)
    fr = eng.frames()
    assert a["frames"].shape == (nrec, 7) and np.array_equal(a["frames"][:, 0], np.arange(nrec))
    for j, f in enumerate(libhv_amd.FRAME_DTYPE.names):
        assert np.array_equal(a["frames"][:, 1 + j], fr[f].astype(np.float64)), f
    first, cnt = eng.segment_frames(16)
    assert np.array_equal(a["segment_frames"], np.column_stack([np.arange(16), first, cnt]).astype(np.float64))
    assert int(a["segment_frames"][:, 2].sum()) == nrec
    carry, started = eng.carry(16)
    assert a["carry"].shape == (16, 8)
    assert [tuple(r) for r in a["carry"][:, 1:7].astype(np.uint64).tolist()] == [c.fields() for c in carry]
    assert a["carry"][:, 7].tolist() == [float(s) for s in started]


def test_dump_sample_when_large(eng, stepped, tmp_path, monkeypatch):
    """Tables and bytes above the limits are cut to a sample that keeps the
    first and the last row / piece and is the same in every call."""
    plan, rx, segs, exp, nrec = stepped
    monkeypatch.setattr(bench, "DUMP_ROWS", 8)
    monkeypatch.setattr(bench, "DUMP_PIECES", 32)
    bench.dump_outputs(eng, rx, plan, segs.n, str(tmp_path / "a"), 0, 1)
    bench.dump_outputs(eng, rx, plan, segs.n, str(tmp_path / "b"), 0, 1)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    for n in NAMES:
        assert np.array_equal(a[n], b[n]), n
    P = bench.DUMP_PIECE
    offs = a["rx_offsets"].astype(np.int64)
    assert 2 <= len(offs) <= 32 and offs[0] == 0 and offs[-1] == plan.total - P and np.all(np.diff(offs) > 0)
    assert a["rx_sample"].shape == (len(offs), P)
    for i, o in enumerate(offs):
        assert np.array_equal(a["rx_sample"][i].astype(np.uint8), exp[o:o + P]), o
    rows = a["frames"][:, 0].astype(np.int64)
    assert 2 <= len(rows) <= 8 and rows[0] == 0 and rows[-1] == nrec - 1
    assert np.array_equal(a["frames"][:, 2], eng.frames()["pay_off"][rows].astype(np.float64))
    srows = a["segment_frames"][:, 0].astype(np.int64)
    assert 2 <= len(srows) <= 8 and srows[0] == 0 and srows[-1] == 15
    assert np.array_equal(a["carry"][:, 0], a["segment_frames"][:, 0])
