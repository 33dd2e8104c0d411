"""GPU: hvws_utf8 (include/hvws.h) -- per-record UTF-8 transition words and the
per-connection fold, against the oracle in tests/wsutf8.py: after a scan
(masked bytes, buffer untouched) and after a step, around the word kernel's
tile edges, over many segments with carried state, over one stream cut into
tiny batches, after a RUN step and behind pipelined steps."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wsutf8 as U

pytestmark = pytest.mark.gpu

EINVAL = -2
PATH_RUN = 7


def _pass(eng, data: bytes, segs, how: str, carry=None, state_in=None):
    """Upload, scan (how = 'scan': payloads stay masked) or step, hvws_utf8.
    -> (words, state_out, bad, buffer afterwards, device buffer)."""
    host = np.frombuffer(data, dtype=np.uint8)
    rx = eng.to_device(host)
    if how == "scan":
        eng.scan(rx, len(data), segs, carry)
    else:
        eng.step(rx, len(data), segs, carry)
    eng.utf8(rx, len(data), how == "scan", state_in)
    words = eng.utf8_words()
    st, bad = eng.utf8_result(len(segs))
    after = rx.download(len(data))
    return words, st, bad, after, rx


def _seed_for(pred, start: int):
    """The first seed from `start` the oracle-only predicate accepts."""
    for seed in range(start, start + 200):
        if pred(seed):
            return seed
    raise AssertionError("no seed found")


def test_words_one_segment_masked_and_unmasked(eng):
    seed = _seed_for(lambda s: U.balanced(U.gen_frames(s, 110)[1]), 1)
    data, valid = U.gen_stream(seed, 110)
    assert U.balanced(valid)
    segs = [(0, len(data))]
    recs, ewords, est, ebad, _, _ = U.oracle_batch(data, segs)
    assert 250 <= len(recs) <= 400 and int(recs["pay_len"].max()) <= 40
    assert int((recs["pay_len"] == 0).sum()) > 0
    w1, st1, bad1, after1, rx1 = _pass(eng, data, segs, "scan")
    rx1.free()
    assert np.array_equal(after1, np.frombuffer(data, np.uint8))   # read-only
    assert np.array_equal(w1, ewords)
    assert list(st1) == list(est) and list(bad1) == list(ebad)
    assert ebad[0] != U.NONE
    w0, st0, bad0, _, rx0 = _pass(eng, data, segs, "step")
    rx0.free()
    assert np.array_equal(w0, w1)
    assert list(st0) == list(est) and list(bad0) == list(ebad)
    # a zero-length record has the identity word
    assert all(int(w) == U.IDENTITY for w, r in zip(w1, recs) if int(r["pay_len"]) == 0)


def _frame(payload: np.ndarray, key: bytes, len64: bool) -> bytes:
    """One masked FIN text frame; len64: the 8-byte length form (14-byte header)."""
    n = len(payload)
    if len64:
        hdr = bytes([0x81, 0x80 | 127]) + n.to_bytes(8, "big") + key
    else:
        assert 126 <= n <= 0xFFFF
        hdr = bytes([0x81, 0x80 | 126]) + n.to_bytes(2, "big") + key
    k = np.frombuffer((key * (n // 4 + 1))[:n], dtype=np.uint8)
    return hdr + (payload ^ k).tobytes()


@pytest.mark.parametrize("len64", [False, True], ids=["pay_off_8", "pay_off_14"])
def test_tile_edges(eng, len64):
    """One text frame of 3 tiles + 5 bytes of 3-byte characters; one byte set
    to FF at every offset from 4 before to 4 after a tile boundary."""
    tile = int(libhv_amd.lib().hvws_utf8_tile())
    n = 3 * tile + 5
    plain = np.frombuffer(("\u20ac" * (n // 3) + "\u00e9").encode(), dtype=np.uint8).copy()
    assert len(plain) == n and n % 3 == 2
    pay_off = 14 if len64 else 8
    key = b"\x9c\x31\xf7\x05"
    boundary = 2 * tile if len64 else tile   # absolute offset in the batch
    data = _frame(plain, key, len64)
    segs = [(0, len(data))]
    w, st, bad, _, rx = _pass(eng, data, segs, "scan")
    rx.free()
    assert [int(x) for x in w] == [U.word(plain.tobytes())] == [0xFFFFFFF0]
    assert int(st[0]) == 0 and int(bad[0]) == U.NONE
    for x in range(boundary - 4, boundary + 5):
        p = plain.copy()
        p[x - pay_off] = 0xFF
        data = _frame(p, key, len64)
        w, st, bad, after, rx = _pass(eng, data, segs, "scan")
        rx.free()
        assert [int(v) for v in w] == [U.word(p.tobytes())] == [0xFFFFFFFF], x
        assert int(st[0]) == U.REJ and int(bad[0]) == 0, x
        assert after.tobytes() == data
    # a character cut by the boundary but whole is fine; a wrong continuation
    # right behind the boundary is not
    for x, b, ok in ((boundary, 0x82, None), (boundary + 1, 0x41, False)):
        p = plain.copy()
        p[x - pay_off] = b
        data = _frame(p, key, len64)
        w, st, bad, _, rx = _pass(eng, data, segs, "scan")
        rx.free()
        assert int(w[0]) == U.word(p.tobytes()), x
        if ok is False:
            assert int(bad[0]) == 0


def test_verdicts_64_segments(eng):
    parts, segs, valid, state_in = [], [], [], []
    at = 0
    for s in range(64):
        d, v = U.gen_stream(100 + s, 4, masked=(s % 4 != 0))
        cut = (7 * s) % 23   # most reads end inside a frame: headers, characters and payloads cut short
        d = d[: len(d) - cut]
        pad = b"" if s % 3 or cut else H.build_frames_ref([(0x1A, b"", None)])   # an unmasked pong behind a whole stream
        parts.append(d + pad)
        segs.append((at, len(d) + len(pad)))
        at += len(d) + len(pad)
        valid += v
        state_in.append(U.REJ if s % 7 == 3 else (U.TEXT_OPEN | 2) if s % 7 == 5 else 0)
    assert U.balanced(valid)
    data = b"".join(parts)
    recs, ewords, est, ebad, firsts, _ = U.oracle_batch(data, segs, None, state_in)
    assert sum(1 for b in ebad if b == U.NONE) >= 8 and sum(1 for b in ebad if b != U.NONE) >= 16
    assert len({int(x) for x in est} - {0, U.REJ}) >= 3   # characters and messages left open
    for how in ("scan", "step"):
        w, st, bad, _, rx = _pass(eng, data, segs, how, None, np.array(state_in, np.uint32))
        rx.free()
        assert np.array_equal(w, ewords), how
        assert list(st) == list(est), how
        assert list(bad) == list(ebad), how
    assert int(ebad[3]) == firsts[3]   # REJECT carried in: the segment's first record


@pytest.mark.parametrize("tail", ["reject_late", "left_open", "hundreds_of_fragments"])
def test_long_segment(eng, tail):
    """One connection with several hundred records in one batch: the fold
    carries its state across every group of records it takes at once."""
    frames, _ = U.gen_frames(21, 120, bad=0.0)
    key = b"\x01\x02\x03\x04"
    if tail == "reject_late":
        frames += [(0x31, b"ok\xc0", key)] + U.gen_frames(22, 10)[0]
    elif tail == "left_open":
        frames += [(0x21, b"a\xf0\x9f", key), (0x2A, b"pong", key)]
    else:   # one message cut at every byte into 180 fragments, a ping in the middle, the last byte wrong
        text = ("\U0001f600\u20ac\u00e9z" * 18).encode()
        text = text[:-1] + b"\xc1"
        for i, b in enumerate(text):
            fl = (1 if i == 0 else 0) | (0x10 if i == len(text) - 1 else 0) | 0x20
            frames.append((fl, bytes([b]), key))
            if i == 90:
                frames.append((0x39, b"", key))
    data = H.build_frames_ref(frames)
    segs = [(0, len(data))]
    recs, ewords, est, ebad, _, _ = U.oracle_batch(data, segs)
    assert len(recs) >= 200
    if tail == "left_open":
        assert (int(est[0]), int(ebad[0])) == (U.TEXT_OPEN | 2, U.NONE)
    elif tail == "reject_late":
        assert int(est[0]) == U.REJ and 180 <= int(ebad[0]) < len(recs) - 5
    else:
        assert int(est[0]) == U.REJ and int(ebad[0]) == len(recs) - 1
    w, st, bad, _, rx = _pass(eng, data, segs, "scan")
    rx.free()
    assert np.array_equal(w, ewords)
    assert (int(st[0]), int(bad[0])) == (int(est[0]), int(ebad[0]))


def _first_invalid(valid):
    return valid.index(False) if False in valid else len(valid)


def test_one_stream_in_tiny_batches(eng):
    """~600 bytes cut into batches of 1, 2, 3, 5, 7, 11 and 64 bytes: headers,
    characters and payloads are cut everywhere; the state word and the parser
    carry ride along.  Same verdict (the rejecting record's frame) and final
    state as the stream in one batch."""
    def wanted(seed):
        d, v = U.gen_stream(seed, 16)
        return U.balanced(v) and _first_invalid(v) >= 4 and 500 <= len(d) <= 800

    seed = _seed_for(wanted, 1)
    data, valid = U.gen_stream(seed, 16)
    assert U.balanced(valid) and _first_invalid(valid) >= 4
    recs, _, est, ebad, _, _ = U.oracle_batch(data, [(0, len(data))])
    assert ebad[0] != U.NONE
    starts = [int(r["hdr_off"]) for r in recs]
    ends = [int(r["pay_off"]) + int(r["pay_len"]) for r in recs]

    def frame_of(pos):   # the frame whose bytes (header start, payload end] hold stream position pos
        return next(j for j in range(len(recs)) if starts[j] < pos <= ends[j])

    want_frame = int(ebad[0])
    sizes = [1, 2, 3, 5, 7, 11, 64]
    at, k = 0, 0
    carry_g, carry_o = None, None
    state_g, state_o = 0, 0
    got_frame = None
    while at < len(data):
        n = min(sizes[k % len(sizes)], len(data) - at)
        k += 1
        chunk = data[at:at + n]
        orec, _, ost, obad, _, ocarry = U.oracle_batch(chunk, [(0, n)], carry_o, [state_o])
        w, st, bad, _, rx = _pass(eng, chunk, [(0, n)], "scan" if k % 2 else "step", carry_g,
                                  np.array([state_g], np.uint32))
        cg, _ = eng.carry(1)
        rx.free()
        assert (int(st[0]), int(bad[0])) == (int(ost[0]), int(obad[0])), (at, n)
        if got_frame is None and int(bad[0]) != U.NONE:
            r = orec[int(bad[0])]
            got_frame = frame_of(at + int(r["pay_off"]) + int(r["pay_len"]))
        carry_g, carry_o = [cg[0]], [ocarry[0]]
        state_g, state_o = int(st[0]), int(ost[0])
        at += n
    assert got_frame == want_frame
    assert state_g == int(est[0]) == U.REJ


def test_valid_stream_in_tiny_batches_carries_open_state(eng):
    """The same cuts over valid text only: the final state is ACCEPT with
    nothing open, and the state word is non-trivial on the way."""
    frames, _ = U.gen_frames(77, 10, bad=0.0)
    data = H.build_frames_ref(frames)
    _, _, est, ebad, _, _ = U.oracle_batch(data, [(0, len(data))])
    assert (int(est[0]), int(ebad[0])) == (0, U.NONE)
    sizes = [1, 2, 3, 5, 7, 11, 64]
    at, k, carry_g, state_g, seen = 0, 0, None, 0, set()
    while at < len(data):
        n = min(sizes[k % len(sizes)], len(data) - at)
        k += 1
        w, st, bad, _, rx = _pass(eng, data[at:at + n], [(0, n)], "scan", carry_g, np.array([state_g], np.uint32))
        cg, _ = eng.carry(1)
        rx.free()
        assert int(bad[0]) == U.NONE, at
        carry_g, state_g = [cg[0]], int(st[0])
        seen.add(state_g)
        at += n
    assert state_g == 0
    assert len(seen & {U.TEXT_OPEN | s for s in range(1, 8)}) >= 3, seen


def test_after_a_run_step(eng):
    """64 segments of equal 200-byte text frames through the RUN path: its
    records are built for the pass, words and verdicts equal the oracle's."""
    import random

    L = libhv_amd.lib()
    r = random.Random(9)
    frames, nvalid = [], 0
    per_seg = 6
    for i in range(64 * per_seg):
        text = ""
        while len(text.encode()) < 200:
            text += r.choice(U.POOL)
        p = text.encode()
        while len(p) > 200:   # drop whole characters from the front, pad with ASCII
            text = text[1:]
            p = text.encode()
        p = p + b"." * (200 - len(p))
        if i % 3 == 1:
            j = r.randrange(200)
            p = p[:j] + bytes([r.choice(U.MUTATIONS)]) + p[j + 1:]
        nvalid += U.is_utf8(p)
        frames.append((0x31, p, bytes(r.randrange(256) for _ in range(4))))
    assert 4 * nvalid >= len(frames) and 4 * (len(frames) - nvalid) >= len(frames)
    data = H.build_frames_ref(frames)
    size = len(data) // len(frames)
    assert size == 208
    segs = [(s * per_seg * size, per_seg * size) for s in range(64)]
    recs, ewords, est, ebad, _, _ = U.oracle_batch(data, segs)
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    old_bound = L.hvws_set_fast_bound(eng.ctx, 1)
    old_run = L.hvws_set_run(eng.ctx, 1)
    try:
        eng.step(rx, len(data), segs)
        assert L.hvws_last_scan_path(eng.ctx) == PATH_RUN
        eng.utf8(rx, len(data), False)
        w = eng.utf8_words()
        st, bad = eng.utf8_result(64)
    finally:
        L.hvws_set_run(eng.ctx, old_run)
        L.hvws_set_fast_bound(eng.ctx, old_bound)
        rx.free()
    assert np.array_equal(w, ewords)
    assert list(st) == list(est) and list(bad) == list(ebad)


def test_pass_queued_behind_pipelined_steps(eng):
    """Pipelined steps A, B, C; the pass over A is held back 20 ms on the
    context stream, so it is still queued when C's scan wants the table set A's
    records live in.  A's words must be A's."""
    seed_a = _seed_for(lambda s: U.balanced(U.gen_frames(s, 40)[1]), 31)
    batches = [U.gen_stream(seed, nmsg)[0] for seed, nmsg in ((seed_a, 40), (seed_a + 1, 25), (seed_a + 2, 55))]
    assert U.balanced(U.gen_stream(seed_a, 40)[1])
    segs = [[(0, len(d) // 2), (len(d) // 2, len(d) - len(d) // 2)] for d in batches]
    ra, ewa, esta, ebada, _, _ = U.oracle_batch(batches[0], segs[0])
    rc, ewc, _, _, _, _ = U.oracle_batch(batches[2], segs[2])
    assert len(ewa) != len(ewc)
    rx = [eng.to_device(np.frombuffer(d, np.uint8)) for d in batches]
    L = libhv_amd.lib()
    try:
        eng.step_resident(rx[0], len(batches[0]), segs[0])
        assert L.hvws_debug_stall(eng.ctx, 20000) == 0
        eng.utf8(rx[0], len(batches[0]), False)
        eng.step_resident(rx[1], len(batches[1]), segs[1])
        eng.step_resident(rx[2], len(batches[2]), segs[2])
        w = eng.utf8_words()
        st, bad = eng.utf8_result(2)
        assert eng.last_kernel_ms() > 0
    finally:
        eng.sync()
        for b in rx:
            b.free()
    assert np.array_equal(w, ewa)
    assert list(st) == list(esta) and list(bad) == list(ebada)


def test_errors():
    L = libhv_amd.lib()
    with libhv_amd.Engine(0) as e:
        data, _ = U.gen_stream(5, 10)
        rx = e.to_device(np.frombuffer(data, np.uint8))
        other = e.alloc(len(data) + 64)
        assert L.hvws_utf8(e.ctx, rx.ptr, len(data), 1, None) == EINVAL       # no scan yet
        assert L.hvws_utf8_count(e.ctx) == -1
        e.scan(rx, len(data), [(0, len(data))])
        assert L.hvws_utf8(e.ctx, other.ptr, len(data), 1, None) == EINVAL    # another buffer
        assert L.hvws_utf8(e.ctx, rx.ptr, len(data) - 1, 1, None) == EINVAL   # another length
        assert L.hvws_utf8(e.ctx, rx.ptr, len(data), 1, None) == 0
        n = L.hvws_utf8_count(e.ctx)
        assert n == L.hvws_frame_count(e.ctx) > 0
        out = np.zeros(4, np.uint32)
        assert L.hvws_get_utf8_words(e.ctx, out.ctypes.data, n - 1, 2) == EINVAL
        assert L.hvws_get_utf8_words(e.ctx, out.ctypes.data, n - 1, 1) == 0
        rx.free()
        other.free()
