"""GPU: the passes that read the frame table -- hvws_utf8, hvws_messages,
hvws_messages_joined, hvws_messages_rfc and, behind it, hvws_replies /
hvws_send_messages -- behind every scan path (include/hvws.h HVWS_PATH_*).

They produce nothing of their own from the batch: they read f_off / f_len /
f_keyrot / f_info, total, counts[] and bases[] as the scan left them, and each
of the eight paths fills those in its own way (the count on the device, an
exact table, estimated bases, a compacted scratch table, a re-scan into the
same set, a guessed and a re-emitted one-stream table, the sieve's emit sites,
records built on demand after RUN), the pipelined forms in two alternating
sets.  f_keyrot in particular no getter returns: after an hvws_scan the
masked = 1 forms of the passes are its readers.

Every case forces a path (the settings of test_gpu_parity.SCAN_MODES), asserts
it was taken, and runs passcases.check_passes behind that one scan: bytes,
every table column, first / count, every state word, bad[] and the sentinel
bytes beyond the total, exactly, against the CPU oracles; then the next batch
from the engine's own carried state of every kind."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import passcases as P
from test_gpu_parity import SCAN_MODES, _last_sieve, sieve_low, spec_min   # noqa: F401 -- fixtures
from test_gpu_validate_paths import Reads, forced, forces_run, scan_step

pytestmark = pytest.mark.gpu

EINVAL = -2
COUNT_EMIT, COUNT_READ, SINGLE, SPEC, SPEC_FAILED, SLACK, SLACK_FAILED, RUN = range(8)   # HVWS_PATH_*
EXACT = ("exact", 1, 0)


def _mode_hows(modes):
    """(mode, how) for every mode; the RUN path is a step's only."""
    out = [(m, h) for m in modes for h in ("scan", "step") if not (forces_run(m) and h == "scan")]
    return out, [f"{m[0]}-{h}" for m, h in out]


def _wanted_path(mode, uniform: bool) -> int:
    """The path a batch of several segments takes under `mode`: mixed sizes
    reject SPEC's estimates, uniform ones pass them."""
    if forces_run(mode):
        return RUN
    if "speculate" in mode[0]:
        return SPEC if uniform else SPEC_FAILED
    if "slack" in mode[0]:
        return SLACK
    return COUNT_READ if mode[0] == "count_read" else COUNT_EMIT


def _scan(eng, mode, how, rx, n, segs, carries) -> int:
    """hvws_scan (payloads stay masked), or the mode's step; -> the path taken."""
    if how == "scan":
        eng.scan(rx, n, segs, carries)
    else:
        scan_step(eng, mode, rx, n, segs, carries)
    return libhv_amd.lib().hvws_last_scan_path(eng.ctx)


def _learn(eng, rx, data, segs, carries) -> None:
    """SLACK sizes its regions from the last exact scan: let that scan be this
    batch's, whatever ran on the context before, then put the bytes back."""
    with forced(eng, EXACT):
        eng.step(rx, len(data), segs, carries)
    rx.upload(np.frombuffer(data, np.uint8))


def _learn_from(eng, other) -> None:
    """SPEC emits into the table as the last scans left it and is rejected when
    that cannot hold the batch: size it by an exact scan of another batch of
    the same shape, which leaves none of this batch's records behind."""
    data, segs = other
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    try:
        with forced(eng, EXACT):
            eng.step(rx, len(data), segs)
    finally:
        eng.sync()
        rx.free()


def _batch(eng, mode, how, data, segs, carries=None, states=None, prev=None, learn=False, after_scan=None):
    """One batch under `mode` (the caller holds forced(eng, mode)) and
    check_passes behind it -> (path, states, prev).  learn: True = an exact
    scan of this batch first (SLACK), a batch = an exact scan of that one (SPEC)."""
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    try:
        if learn is True:
            _learn(eng, rx, data, segs, carries)
        elif learn:
            _learn_from(eng, learn)
        path = _scan(eng, mode, how, rx, len(data), segs, carries)
        if after_scan:
            after_scan()
        states, prev = P.check_passes(eng, rx, data, segs, carries, how, states, prev)
    finally:
        eng.sync()
        rx.free()
    return path, states, prev


def _two_batches(eng, mode, how, case: P.Case, learn=False):
    """Batch 1, then batch 2 from the engine's own carry of every kind -> (path 1, path 2)."""
    p1, st, prev = _batch(eng, mode, how, *case.batches[0], None, P.fresh(len(case.conns), case.raw), learn=learn)
    try:
        p2, _, prev = _batch(eng, mode, how, *case.batches[1], st.parser, st, prev, learn=learn)
    finally:
        prev.free()
    return p1, p2


# --------------------------------- 1. many mixed connections, every mode, two batches
_ALL, _ALL_IDS = _mode_hows(SCAN_MODES)


@pytest.mark.parametrize("mode,how", _ALL, ids=_ALL_IDS)
def test_mixed_connections_two_batches(eng, spec_min, mode, how):
    """40 mixed connections cut once (tests/test_passes_cases.py: what the
    cuts, frames and verdicts are): COUNT_EMIT, COUNT_READ_EMIT, SPEC_FAILED,
    SLACK and RUN (records built by run_materialize, every segment repaired)."""
    case = P.case1()
    with forced(eng, mode):
        paths = _two_batches(eng, mode, how, case, learn="slack" in mode[0])
    want = _wanted_path(mode, uniform=False)
    assert paths == (want, want), (mode[0], how, paths)


# --------------------------------- 2. uniform connections: SPEC accepted and RUN
_UNI, _UNI_IDS = _mode_hows([m for m in SCAN_MODES if "speculate" in m[0] or forces_run(m)])


@pytest.mark.parametrize("mode,how", _UNI, ids=_UNI_IDS)
def test_uniform_connections_whole_and_cut(eng, mode, how):
    """32 connections of 48 frames of one size: whole (SPEC's estimates hold:
    records at estimated bases), then cut inside a frame, the second batch
    begun by the carried-in record the one-walk pass writes."""
    case = P.case2()
    want = _wanted_path(mode, uniform=True)
    with forced(eng, mode):
        other = P.case2(2).whole   # the same shape, other bytes, sizes, cuts and keys
        path, _, prev = _batch(eng, mode, how, *case.whole, learn=other)
        prev.free()
        assert path == want, (mode[0], how, path)
        paths = _two_batches(eng, mode, how, case, learn=other)
    ok = (RUN,) if want == RUN else (SPEC, SPEC_FAILED)
    assert paths[0] in ok and paths[1] in ok, (mode[0], how, "paths of the cut batches", paths)
    if want == SPEC:   # the carried-in record behind an accepted check, not behind its re-scan
        assert paths[1] == SPEC, (mode[0], how, "paths of the cut batches", paths)


# --------------------------------- 3. SLACK_FAILED
@pytest.mark.parametrize("how", ["scan", "step"])
def test_slack_region_outgrown(eng, how):
    """Regions sized by a thin batch (2 records a segment), then 200 tiny
    frames in one segment: the check fails, the re-scan fills the same set."""
    (thin, tsegs), (dense, dsegs) = P.case3()
    mode = ("slack", 1, 2)
    rx = eng.to_device(np.frombuffer(thin, np.uint8))
    try:
        with forced(eng, EXACT):
            eng.scan(rx, len(thin), tsegs)
    finally:
        rx.free()
    with forced(eng, mode):
        path, _, prev = _batch(eng, mode, how, dense, dsegs)
        prev.free()
    assert path == SLACK_FAILED, path


# --------------------------------- 4. one segment
@pytest.mark.parametrize("how", ["scan", "step"])
def test_single_table_guess_checked(how):
    """One stream whose record bound exceeds the table sized from the first
    guess (passcases.Overflow.FIRST_TABLE records; tests/test_passes_cases.py):
    scan_single's `bound > frame_cap`, so the device checks the count against
    the table and accepts it.  A context of its own: the guess and the table
    are what a fresh one has."""
    data = P.case4_checked()
    assert len(data) // 2 + 3 > P.Overflow.FIRST_TABLE
    mode = SCAN_MODES[0]
    with libhv_amd.Engine(0) as fresh:
        path, _, prev = _batch(fresh, mode, how, data, [(0, len(data))])
        prev.free()
    assert path == SINGLE, path


@pytest.mark.parametrize("how", ["scan", "step"])
def test_single_table_overflowed_and_re_emitted(how):
    """1.4 M records against the first guess of 2^20 and the table sized from
    it (1.25 * 2^20 records): the pass overflows, the segment is re-emitted
    into an exact table and launch_offsets fills counts / bases.  Every record is a whole message, so the expectation is numpy's from
    the frame list (pinned to the oracles in tests/test_passes_cases.py);
    hvws_utf8 and hvws_messages only.  A context of its own, as
    test_gpu_parity.test_single_segment_table_overflow."""
    ov = P.overflow()
    assert ov.n > ov.FIRST_TABLE
    n = len(ov.wire)
    out, table, (first, count), state, words, u8, bad = ov.expect()
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as fresh:
        rx = fresh.to_device(ov.wire)
        d_out = fresh.alloc(n + P.SLACK)
        try:
            assert L.hvws_memset(fresh.ctx, d_out.ptr, P.SENTINEL, n + P.SLACK) == 0
            assert _scan(fresh, SCAN_MODES[0], how, rx, n, [(0, n)], None) == SINGLE
            fresh.utf8(rx, n, how == "scan")
            assert L.hvws_utf8_count(fresh.ctx) == ov.n
            assert np.array_equal(fresh.utf8_words(), words)
            got_u8, got_bad = fresh.utf8_result(1)
            assert got_u8.tolist() == u8.tolist() and got_bad.tolist() == bad.tolist()
            fresh.messages(rx, n, how == "scan", d_out, n)
            assert fresh.msg_bytes() == len(out)
            P._same_bytes(d_out.download(n + P.SLACK), out, how)
            P._same_table(fresh.message_table(), table, how)
            got_first, got_count = fresh.segment_messages(1)
            assert (got_first.tolist(), got_count.tolist()) == (first.tolist(), count.tolist())
            P._same_states(fresh.msg_state(1), state, how)
            assert np.array_equal(rx.download(n), ov.wire if how == "scan" else ov.plain)
        finally:
            fresh.sync()
            rx.free()
            d_out.free()


@pytest.mark.parametrize("how", ["scan", "step"])
@pytest.mark.parametrize("stream", ["clean", "quirks", "cut"])
def test_sieved_stream(eng, sieve_low, stream, how):
    """A 256 KiB stream found by the frame sieve: its chain covers every frame
    (clean); stops at an unmasked and an RSV frame, where the exact walk takes
    over (quirks); ends 3 bytes into the last header, the second batch run from
    the carry (cut)."""
    clean, quirks, cut = P.case4_sieved()
    data = {"clean": clean, "quirks": quirks, "cut": clean[:cut]}[stream]
    nframes = len(P.headers(clean))
    mode = SCAN_MODES[0]

    def sieve_state():
        active, _, npath, pend = _last_sieve(eng)
        assert active == 1, (stream, active)
        if stream == "clean":
            assert npath == nframes and pend == len(data), (npath, nframes, pend, len(data))
        elif stream == "quirks":
            assert pend < len(data), (npath, pend, len(data))   # the exact walk resumed before the end

    path, st, prev = _batch(eng, mode, how, data, [(0, len(data))], after_scan=sieve_state)
    try:
        assert path == SINGLE, path
        if stream == "cut":
            rest = clean[cut:]
            path, _, prev = _batch(eng, mode, how, rest, [(0, len(rest))], st.parser, st, prev)
            assert path == SINGLE, path
    finally:
        prev.free()


# --------------------------------- 5. passes between pipelined steps
_PIPED, _PIPED_IDS = _mode_hows([m for m in SCAN_MODES if m[0].startswith("pipelined")])


@pytest.mark.parametrize("mode,how", _PIPED, ids=_PIPED_IDS)
def test_passes_queued_between_pipelined_steps(eng, mode, how):
    """Pipelined steps A, B, C of three different batches; the four passes over
    A are queued behind a 2 ms stall of the context stream, so they still wait
    when C's scan wants the table set A's records live in (the event recorded
    inside each pass orders it).  Nothing of A is read before C is stepped;
    then every pass's output is A's.  how == "scan": A is scanned (its payloads
    stay masked, the masked forms run) and B is the step that enters pipelined
    mode, behind the queued passes.  Twice: the first round sizes every buffer,
    so the second allocates nothing (a hipFree would synchronise the device and
    close the window)."""
    L = libhv_amd.lib()
    uniform = "speculate" in mode[0] or forces_run(mode)
    batches = [(P.case2(k).whole if uniform else P.case1(k).batches[0]) for k in (1, 2, 3)]
    raw = () if uniform else P.RAW1
    plain = [P.expect(d, segs, None, P.fresh(len(segs), raw)).plain for d, segs in batches]
    (a, asegs), (b, bsegs), (c, csegs) = batches
    assert len({len(d) for d, _ in batches}) == 3
    want = _wanted_path(mode, uniform)
    with forced(eng, mode):
        for rnd in range(2):
            rxs = [eng.to_device(np.frombuffer(d, np.uint8)) for d, _ in batches]
            run = None
            try:
                if "slack" in mode[0]:
                    _learn(eng, rxs[0], a, asegs, None)
                elif "speculate" in mode[0]:
                    _learn_from(eng, batches[1])
                run = P.Run(eng, rxs[0], a, asegs, None, how, P.fresh(len(asegs), raw), None)
                eng.sync()
                path = _scan(eng, mode, how, rxs[0], len(a), asegs, None)
                libhv_amd._check(L.hvws_debug_stall(eng.ctx, 2000), "hvws_debug_stall")
                run.q_utf8()
                run.q_messages()
                run.q_joined()
                run.q_rfc()
                eng.step_resident(rxs[1], len(b), bsegs)
                eng.step_resident(rxs[2], len(c), csegs)   # writes A's table set
                assert path == want, (mode[0], how, rnd, path)
                run.c_utf8()
                run.c_messages(tables=False)
                run.c_joined(tables=False)
                run.c_rfc()
                got = [rx.download(len(d)) for rx, (d, _) in zip(rxs, batches)]
                assert np.array_equal(got[0], np.frombuffer(a, np.uint8) if how == "scan" else plain[0]), (mode[0], how)
                assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2]), (mode[0], how)
            finally:
                eng.sync()
                if run:
                    run.free()
                for rx in rxs:
                    rx.free()


# --------------------------------- 6. after the small path
def _getters(eng, nseg):
    L = libhv_amd.lib()
    st, bad = eng.utf8_result(nseg)
    first, count = eng.segment_messages(nseg)
    rep, piece = eng.reply_table()
    rfirst, rcount = eng.segment_replies(nseg)
    return [int(L.hvws_utf8_count(eng.ctx)), eng.utf8_words().tolist(), st.tolist(), bad.tolist(),
            int(L.hvws_msg_count(eng.ctx)), eng.msg_bytes(), eng.message_table().tolist(), first.tolist(), count.tolist(),
            eng.rfc_state(nseg).tolist(), rep.tolist(), piece.tolist(), rfirst.tolist(), rcount.tolist(),
            eng.reply_flags(nseg).tolist()]


@pytest.mark.parametrize("via", ["rx_batch_small", "rx_reads"])
def test_passes_refuse_after_the_small_path(eng, via):
    """hvws_rx_batch on its small-batch path and hvws_rx_reads leave no device
    frame table: every pass is HVWS_EINVAL, writes nothing, and the previous
    results' getters return what they returned before."""
    L = libhv_amd.lib()
    data, segs = P.case1().batches[0]
    n, nseg = len(data), len(segs)
    buf = np.frombuffer(data, np.uint8)
    rx = eng.to_device(buf)
    d_out = eng.alloc(n + P.SLACK)
    try:
        eng.scan(rx, n, segs)
        _, prev = P.check_passes(eng, rx, data, segs, None, "scan", P.fresh(nseg, P.RAW1))
        prev.free()
        before = _getters(eng, nseg)
        assert before[0] == len(P.expect(data, segs, None, P.fresh(nseg, P.RAW1)).words) > 300
        assert before[4] > 100 and len(before[10]) > 50
        if via == "rx_batch_small":
            host = buf.copy()
            old = L.hvws_set_small_batch_limit(eng.ctx, 0)   # the default: a batch this small takes k_small
            try:
                eng.rx_batch(host, segs, None, True)
            finally:
                L.hvws_set_small_batch_limit(eng.ctx, old)
            assert np.array_equal(host, P.expect(data, segs, None, P.fresh(nseg, P.RAW1)).plain)
        else:
            reads = Reads(eng, n, list(range(nseg)))
            try:
                reads.run([data[o:o + ln] for o, ln in segs])
            finally:
                reads.free()
        assert L.hvws_frame_count(eng.ctx) == before[0]   # the same batch's records, on the host only
        assert L.hvws_memset(eng.ctx, d_out.ptr, P.SENTINEL, n + P.SLACK) == 0
        for masked in (1, 0):
            assert L.hvws_utf8(eng.ctx, rx.ptr, n, masked, None) == EINVAL
            assert L.hvws_messages(eng.ctx, rx.ptr, n, masked, d_out.ptr, n, None) == EINVAL
            assert L.hvws_messages_joined(eng.ctx, rx.ptr, n, masked, d_out.ptr, n, None, None, 0, None) == EINVAL
            assert L.hvws_messages_rfc(eng.ctx, rx.ptr, n, masked, d_out.ptr, n, None, None, 0) == EINVAL
        assert np.all(d_out.download(n + P.SLACK) == P.SENTINEL)
        assert _getters(eng, nseg) == before
        assert np.array_equal(rx.download(n), buf)
    finally:
        eng.sync()
        rx.free()
        d_out.free()
