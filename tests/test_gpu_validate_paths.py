"""GPU: protocol validation (hvws_set_validation) on every scan path and across
headers cut by a batch end.

The violation bits of a record are produced at eight places in the device code
(the exact state machine, the wave walk's packed speculation, k_verify, the
three sieve emit sites, the door, k_small and its hvws_rx_reads forms, the
one-walk passes' carried-in record); tests/test_gpu_validate.py reaches few of
them.  Here every connection is a stream of whole frames cut once: batch 1
holds [0, cut) of every connection, batch 2 the rest, resumed from the carry
the engine itself handed back for batch 1 (the partial header's classes ride
in the parser's padding byte, which only the library writes).

Expected values come from the CPU alone: the oracle's records for the same
cuts (validation off) and wsvalidate.violations for the classes of the
stream's k-th header.  A record with HVWS_I_HDR gains HVWS_I_INVALID and its
enabled classes; nothing else may change -- offsets, lengths, keys, the other
info bits, the unmasked bytes and the carry are the oracle's."""
from __future__ import annotations

import contextlib
import ctypes
import functools
import random
import struct

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wsvalidate as V
from libhv_amd import synth
from test_gpu_parity import SCAN_MODES, _last_sieve, sieve_low, spec_min   # noqa: F401 -- fixtures

pytestmark = pytest.mark.gpu

I_HDR, I_INVALID, V_SHIFT = 1 << 10, 1 << 14, 16
V_BITS = I_INVALID | (V.V_ALL << V_SHIFT)
PATH_SPEC, PATH_SLACK, PATH_RUN = 3, 5, 7   # include/hvws.h HVWS_PATH_*
FIELDS = ("hdr_off", "pay_off", "pay_len", "length", "key", "info")
V_LATE = V.V_CONTROL | V.V_NONMIN | V.V_LEN64   # classes only known once the length is decoded


# ------------------------------------------------------------ scan modes
def forces_run(mode) -> bool:
    return len(mode) > 4 and mode[4] == 1


@contextlib.contextmanager
def forced(eng, mode, vmask=None):
    """The context's fast bound, speculation, walk-verify and RUN settings as
    `mode` (an entry of test_gpu_parity.SCAN_MODES) asks, set and restored as
    test_gpu_parity._step_checked does, and, if given, its validation classes."""
    L = libhv_amd.lib()
    old_b = L.hvws_set_fast_bound(eng.ctx, mode[1])
    old_s = L.hvws_set_speculation(eng.ctx, mode[2])
    old_v = L.hvws_set_walk_verify(eng.ctx, mode[3] if len(mode) > 3 else -1)
    old_r = L.hvws_set_run(eng.ctx, 1 if forces_run(mode) else 0)
    old_m = L.hvws_set_validation(eng.ctx, vmask) if vmask is not None else None
    try:
        yield
    finally:
        L.hvws_set_fast_bound(eng.ctx, 0 if old_b == 1 << 24 else old_b)
        L.hvws_set_speculation(eng.ctx, old_s)
        L.hvws_set_walk_verify(eng.ctx, old_v)
        L.hvws_set_run(eng.ctx, old_r)
        if old_m is not None:
            L.hvws_set_validation(eng.ctx, old_m)


def scan_step(eng, mode, rx, rx_len, segs, carries):
    """One step of the batch: hvws_step_resident for the pipelined modes."""
    if mode[0].startswith("pipelined"):
        eng.step_resident(rx, rx_len, segs, carries)
    else:
        eng.step(rx, rx_len, segs, carries)


# ------------------------------------------------------------ CPU expectations
def _hlen(data: bytes, off: int) -> int:
    b1 = data[off + 1]
    return 2 + {126: 2, 127: 8}.get(b1 & 127, 0) + (4 if b1 & 128 else 0)


class Conn:
    """One connection: a stream of whole frames and its cut.  Holds, for each
    of its two parts, the oracle's records (offsets relative to the part),
    carry-out, started flag and unmasked bytes, and per record the classes its
    header violates (0 for records without HVWS_I_HDR).  Asserts what the
    construction stands on: the HDR records of the two parts number exactly
    len(violations) and the k-th one's payload starts where the k-th header
    ends."""

    def __init__(self, data: bytes, cut: int):
        assert 1 <= cut <= len(data)
        self.data, self.cut = data, cut
        self.viol = V.violations(data)
        self.parts = (data[:cut], data[cut:])
        r1, st1, s1, o1 = H.scan_segment(self.parts[0])
        r2, st2, s2, o2 = H.scan_segment(self.parts[1], st1)
        self.recs, self.st, self.started, self.out = (r1, r2), (st1, st2), (s1, s2), (o1, o2)
        h1, h2 = (r1["info"] & I_HDR) != 0, (r2["info"] & I_HDR) != 0
        ends = [int(x) for x in r1["pay_off"][h1]] + [int(x) + cut for x in r2["pay_off"][h2]]
        assert ends == [off + _hlen(data, off) for off, _ in self.viol], "HDR records do not line up with the headers"
        classes = np.array([v for _, v in self.viol], np.uint32)
        c1, c2 = np.zeros(len(r1), np.uint32), np.zeros(len(r2), np.uint32)
        c1[h1] = classes[:int(h1.sum())]
        c2[h2] = classes[int(h1.sum()):]
        self.cls = (c1, c2)

    def cut_header_classes(self):
        """Classes of the header the cut falls inside, or None when it falls elsewhere."""
        for off, v in self.viol:
            if off < self.cut < off + _hlen(self.data, off):
                return v
        return None


def _with_bits(recs: np.ndarray, cls: np.ndarray, vmask: int) -> np.ndarray:
    r = recs.copy()
    v = cls & np.uint32(vmask)
    r["info"] |= np.where(v != 0, np.uint32(I_INVALID) | (v << np.uint32(V_SHIFT)), np.uint32(0)).astype(np.uint32)
    return r


def _expect_table(conns, part: int, offs, vmask: int) -> np.ndarray:
    """The batch's expected frame table: each connection's records of `part`
    moved to its segment's offset, validation bits set for vmask."""
    out = []
    for c, off in zip(conns, offs):
        r = _with_bits(c.recs[part], c.cls[part], vmask)
        r["pay_off"] += np.uint64(off)
        r["hdr_off"] = np.where(r["hdr_off"] >= 0, r["hdr_off"] + off, -1)
        out.append(r)
    return np.concatenate(out) if out else np.zeros(0, libhv_amd.FRAME_DTYPE)


def _assert_table(frames: np.ndarray, exp: np.ndarray, tag) -> None:
    assert len(frames) == len(exp), (tag, len(frames), len(exp))
    for f in FIELDS:
        if not np.array_equal(frames[f], exp[f]):
            k = int(np.flatnonzero(frames[f] != exp[f])[0])
            raise AssertionError(f"{tag}: {f} of record {k}: got {int(frames[f][k]):#x}, expected {int(exp[f][k]):#x} "
                                 f"(hdr_off {int(exp['hdr_off'][k])}, info {int(exp['info'][k]):#x})")


def _assert_carry(cout, started, conns, part: int, tag) -> None:
    for i, c in enumerate(conns):
        assert cout[i].fields() == c.st[part].fields(), (tag, i)
        if started is not None:
            assert started[i] == c.started[part], (tag, i)


class Batch:
    """Part `part` of every connection laid back to back, one segment each."""

    def __init__(self, conns, part: int, vmask: int):
        self.conns, self.part, self.vmask = conns, part, vmask
        self.segs, at = [], 0
        for c in conns:
            self.segs.append((at, len(c.parts[part])))
            at += len(c.parts[part])
        self.buf = np.frombuffer(b"".join(c.parts[part] for c in conns), np.uint8).copy()
        self.exp_bytes = np.frombuffer(b"".join(c.out[part] for c in conns), np.uint8)
        self.exp = _expect_table(conns, part, [o for o, _ in self.segs], vmask)

    def step_checked(self, eng, mode, carries):
        """One step under `mode` (the caller holds forced(eng, mode, vmask)):
        records, bytes and carry exact.  Returns (carry-out, path)."""
        L = libhv_amd.lib()
        n, nseg = len(self.buf), len(self.segs)
        slack = mode[2] == 2 and nseg > 1
        rx = eng.to_device(self.buf)
        try:
            if slack:
                # SLACK sizes its regions from the last exact scan: let that be
                # this batch's, so a one-walk pass itself (not its fallback) runs:
                # SLACK, or SPEC where that scan found the uniform estimates hold
                with forced(eng, ("exact", 1, 0)):
                    eng.step(rx, n, self.segs, carries)
                rx.upload(self.buf)
            scan_step(eng, mode, rx, n, self.segs, carries)
            got = rx.download(n)
            frames = eng.frames()
            cout, started = eng.carry(nseg)
            path = L.hvws_last_scan_path(eng.ctx)
        finally:
            rx.free()
        tag = (mode[0], "batch", self.part + 1, "vmask", self.vmask)
        if forces_run(mode) and self.vmask:
            assert path != PATH_RUN, tag   # a step under validation never takes the RUN path
        if slack:
            assert path in (PATH_SLACK, PATH_SPEC), (tag, path)
        _assert_table(frames, self.exp, tag)
        assert np.array_equal(got, self.exp_bytes), tag
        _assert_carry(cout, started, self.conns, self.part, tag)
        return cout, path


def _two_batches(eng, conns, vmask: int):
    """The validated twin of test_gpu_parity._compare_batch: batch 1 and, from
    the engine's own carry, batch 2, through every scan mode.
    Returns {mode name: (path of batch 1, path of batch 2)}."""
    b1, b2 = Batch(conns, 0, vmask), Batch(conns, 1, vmask)
    paths = {}
    for mode in SCAN_MODES:
        with forced(eng, mode, vmask):
            carry, p1 = b1.step_checked(eng, mode, None)
            _, p2 = b2.step_checked(eng, mode, carry)
        paths[mode[0]] = (p1, p2)
    return paths


def _one_batch(eng, conns, vmask: int, after_step=None):
    """Whole connections (cut == len) as one batch through every scan mode."""
    assert all(c.cut == len(c.data) for c in conns)
    b = Batch(conns, 0, vmask)
    paths = {}
    for mode in SCAN_MODES:
        with forced(eng, mode, vmask):
            _, paths[mode[0]] = b.step_checked(eng, mode, None)
            if after_step:
                after_step(mode)
    return paths


def _cut_like_case1(rng: random.Random, data: bytes, in_header: bool, violating_only: bool = False) -> int:
    """A cut inside a randomly chosen frame's header (of a violating frame
    when asked), or at a random byte."""
    if not in_header:
        return rng.randrange(1, len(data))
    vio = V.violations(data)
    pick = [(o, v) for o, v in vio if v] if violating_only else vio
    off, _ = pick[rng.randrange(len(pick))]
    return off + rng.randint(1, _hlen(data, off) - 1)


# ------------------------------------------------- 1. many connections, every mode
@functools.lru_cache(maxsize=None)
def _random_conns():
    rng = random.Random(4100)
    conns = []
    for i in range(37):
        data, viol = V.random_stream(100 + i, 40, tail_len64=(i % 5 == 0))
        assert [v for _, v in V.violations(data)] == viol
        # odd i: inside a header -- of any frame, or (every other one) of a
        # violating frame, so that enough cut headers carry classes
        conns.append(Conn(data, _cut_like_case1(rng, data, i % 2 == 1, i % 4 == 1)))
    return conns


@pytest.mark.parametrize("vmask", [V.V_ALL, V_LATE], ids=["all", "late_classes"])
def test_many_connections_every_mode(eng, vmask):
    conns = _random_conns()
    cut = [c.cut_header_classes() for c in conns]
    assert sum(v is not None for v in cut) >= 18
    assert sum(bool(v) for v in cut) >= 10, cut                 # cut headers of violating frames
    assert sum(bool(v and v & V_LATE) for v in cut) >= 3, cut   # ... some only known once the length is decoded
    nviol = sum(bool(v) for c in conns for _, v in c.viol)
    nfr = sum(len(c.viol) for c in conns)
    assert 4 * nviol >= nfr, (nviol, nfr)
    paths = _two_batches(eng, conns, vmask)
    # mixed sizes: the exact large-batch path and SLACK's own walk and compaction ran
    assert paths["count_read"] == (1, 1), paths   # HVWS_PATH_COUNT_READ_EMIT
    for m in ("slack", "slack_noverify", "pipelined_slack", "pipelined_slack_verify"):
        assert paths[m] == (PATH_SLACK, PATH_SLACK), paths


# ------------------------------------------------- 2. every header, every cut
def _header(b0: int, n: int, masked: bool, enc: int, key: bytes = b"\x5a\xc3\x17\xe9") -> bytes:
    """A frame header as it is written: enc 0/1/2 = 7-bit, 16-bit, 64-bit
    length form, whatever n needs."""
    len7 = n if enc == 0 else (126 if enc == 1 else 127)
    ext = b"" if enc == 0 else (struct.pack(">H", n) if enc == 1 else struct.pack(">Q", n))
    return bytes([b0, (0x80 if masked else 0) | len7]) + ext + (key if masked else b"")


def _class_headers():
    """(name, header bytes, payload length or None for the 2^63 header, classes):
    every class with one header of each size it can have -- 2, 4, 10 bytes
    unmasked, 6, 8, 14 masked.  The 64-bit forms announce 300 bytes (so they
    also violate NONMIN) but for the 2^63 + 3 ones."""
    R, O, C, L64, NM, UM = V.V_RSV, V.V_OPCODE, V.V_CONTROL, V.V_LEN64, V.V_NONMIN, V.V_UNMASKED
    out = []
    for enc, n in ((0, 5), (1, 300), (2, 300)):
        nm = NM if enc == 2 else 0
        for masked in (True, False):
            um = 0 if masked else UM
            sz = {0: 2, 1: 4, 2: 10}[enc] + (4 if masked else 0)
            out.append((f"rsv1_text_{sz}", _header(0xC1, n, masked, enc), n, R | nm | um))
            # 0xB is a control opcode: its 300-byte forms also break the 125-byte limit
            out.append((f"opcode_b_{sz}", _header(0x8B, n, masked, enc), n, O | (C if n > 125 else 0) | nm | um))
            out.append((f"ping_nofin_{sz}", _header(0x09, n, masked, enc), n, C | nm | um))
            if not masked:
                out.append((f"unmasked_binary_{sz}", _header(0x82, n, False, enc), n, UM | nm))
    out.append(("ping_126_len16", _header(0x89, 126, True, 1), 126, C))
    out.append(("ping_126_len16_unmasked", _header(0x89, 126, False, 1), 126, C | UM))
    out.append(("len16_of_5", _header(0x82, 5, True, 1), 5, NM))
    out.append(("len16_of_5_unmasked", _header(0x82, 5, False, 1), 5, NM | UM))
    out.append(("len64_of_300", _header(0x82, 300, True, 2), 300, NM))
    out.append(("len64_of_300_unmasked", _header(0x82, 300, False, 2), 300, NM | UM))
    out.append(("len64_2p63", _header(0x82, (1 << 63) + 3, True, 2), None, L64))
    out.append(("len64_2p63_unmasked", _header(0x82, (1 << 63) + 3, False, 2), None, L64 | UM))
    out.append(("rsv_opcode_unmasked", _header(0xF3, 9, False, 0), 9, R | O | UM))
    return out


@functools.lru_cache(maxsize=None)
def _header_conns():
    """One connection per (header, cut), the cut at every byte inside the
    header.  The header is followed by its payload and one valid frame (the
    2^63 one by a few bytes of a body that never ends); every other
    connection has a valid frame in front, so that batch 1 is not only the
    partial header."""
    rng = random.Random(4200)
    valid = lambda: _header(0x81, 7, True, 0, rng.randbytes(4)) + rng.randbytes(7)
    conns, seen = [], {}
    for name, hdr, n, classes in _class_headers():
        for cut in range(1, len(hdr)):
            pre = valid() if cut % 2 == 0 else b""
            body = rng.randbytes(n) + valid() if n is not None else rng.randbytes(11)
            c = Conn(pre + hdr + body, len(pre) + cut)
            k = 1 if pre else 0
            assert c.viol[k] == (len(pre), classes), (name, c.viol[k], classes)
            assert c.cut_header_classes() == classes
            conns.append(c)
        seen.setdefault(classes, set()).add(len(hdr))
    # every class at every header size it can have
    sizes = {b: set() for b in (V.V_RSV, V.V_OPCODE, V.V_CONTROL, V.V_LEN64, V.V_NONMIN, V.V_UNMASKED)}
    for classes, szs in seen.items():
        for b in sizes:
            if classes & b:
                sizes[b] |= szs
    assert sizes[V.V_RSV] == sizes[V.V_OPCODE] == sizes[V.V_CONTROL] == {2, 4, 6, 8, 10, 14}
    assert sizes[V.V_LEN64] == {10, 14} and sizes[V.V_NONMIN] == {4, 8, 10, 14} and sizes[V.V_UNMASKED] == {2, 4, 10}
    return conns


def test_every_header_every_cut(eng):
    conns = _header_conns()
    assert len(conns) >= 70
    _two_batches(eng, conns, V.V_ALL)


# ------------------------------------------------- 3. uniform runs
def _run_frame(kind: str, rng: random.Random) -> bytes:
    """One frame of a uniform run: 106 bytes but for the 16-bit form (108)."""
    key = rng.randbytes(4)
    if kind == "valid":
        return _header(0x82, 100, True, 0, key) + rng.randbytes(100)
    if kind == "unmasked":
        return _header(0x82, 104, False, 0) + rng.randbytes(104)
    if kind == "rsv1":
        return _header(0xC2, 100, True, 0, key) + rng.randbytes(100)
    if kind == "opcode_b":
        return _header(0x8B, 100, True, 0, key) + rng.randbytes(100)
    if kind == "ping_nofin":
        return _header(0x09, 100, True, 0, key) + rng.randbytes(100)
    if kind == "len16_of_100":
        return _header(0x82, 100, True, 1, key) + rng.randbytes(100)
    raise KeyError(kind)


RUN_FRAMES = 1200
RUN_CLASSES = {"unmasked": V.V_UNMASKED, "rsv1": V.V_RSV, "opcode_b": V.V_OPCODE, "ping_nofin": V.V_CONTROL,
               "len16_of_100": V.V_NONMIN}
# 13 connections at frame boundaries of the one run: two long ones, so that
# either side of their cut has more than 256 frames (k_verify's threshold in
# the verify256 parametrisation), and short ones between them
RUN_CONN_FRAMES = [11] * 5 + [540] + [11] * 5 + [540] + [10]
assert sum(RUN_CONN_FRAMES) == RUN_FRAMES and len(RUN_CONN_FRAMES) == 13


def _run_conns(frames, seed):
    """(the run as one whole connection, the run as 13 connections each cut
    once: odd ones inside a header, the long ones near their middle)."""
    rng = random.Random(seed)
    whole = Conn(b"".join(frames), sum(len(f) for f in frames))
    conns, at = [], 0
    for i, nf in enumerate(RUN_CONN_FRAMES):
        part = frames[at:at + nf]
        at += nf
        data = b"".join(part)
        k = rng.randrange(262, 278) if nf > 256 else rng.randrange(nf)   # the frame the cut falls in
        off = sum(len(f) for f in part[:k])
        if i % 2:
            cut = off + rng.randint(1, _hlen(data, off) - 1)
        else:
            cut = off + rng.randrange(1, len(part[k]))
        conns.append(Conn(data, cut))
    assert sum(c.cut_header_classes() is not None for c in conns) >= 6
    return whole, conns


@pytest.mark.parametrize("kind", sorted(RUN_CLASSES))
def test_uniform_run_every_frame_violates(eng, spec_min, kind):
    rng = random.Random(4300 + sorted(RUN_CLASSES).index(kind))
    whole, conns = _run_conns([_run_frame(kind, rng) for _ in range(RUN_FRAMES)], 4310)
    assert [v for _, v in whole.viol] == [RUN_CLASSES[kind]] * RUN_FRAMES
    assert sum(bool(c.cut_header_classes()) for c in conns) >= 6
    _one_batch(eng, [whole], V.V_ALL)
    _two_batches(eng, conns, V.V_ALL)


@pytest.mark.parametrize("at", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("odd", ["rsv1", "unmasked"])
def test_uniform_run_one_frame_violates(eng, spec_min, odd, at):
    """One same-stride violating frame in a run of valid ones: the run holds,
    only that prediction's bits differ."""
    rng = random.Random(4400 + at)
    frames = [_run_frame("valid", rng) for _ in range(RUN_FRAMES)]
    frames[at] = _run_frame(odd, rng)
    assert len({len(f) for f in frames}) == 1
    whole, conns = _run_conns(frames, 4410 + at)
    exp = [0] * RUN_FRAMES
    exp[at] = RUN_CLASSES[odd]
    assert [v for _, v in whole.viol] == exp
    _one_batch(eng, [whole], V.V_ALL)
    paths = _two_batches(eng, conns, V.V_ALL)
    assert paths["speculate"] == (PATH_SPEC, PATH_SPEC), paths


# ------------------------------------------------- 4. sieve handoff
@functools.lru_cache(maxsize=None)
def _sieved_stream():
    plan = synth.mixed_plan(1 << 20, 72, lo=1, hi=5000)
    base = H.synth_cpu(plan).tobytes()
    vio = V.violations(base)
    assert len(vio) == plan.n == 2981 and not any(v for _, v in vio)   # a violation-free base
    offs = [o for o, _ in vio]
    nearest = lambda frac: min(range(len(offs)), key=lambda k: abs(offs[k] - frac * len(base)))
    k1, k3 = nearest(0.3), nearest(0.97)
    rng = random.Random(4500)
    bad = {}
    for k in (k1, k1 + 5, k3):
        bad[k], v = V.make_frame(rng, p_bad=1.0)
        assert v
    assert k1 + 5 < k3
    parts, at = [], 0
    for k in sorted(bad):
        parts += [base[at:offs[k]], bad[k]]
        at = offs[k]
    parts.append(base[at:])
    data = b"".join(parts)
    c = Conn(data, len(data))
    assert sum(bool(v) for _, v in c.viol) == 3 and len(c.viol) == plan.n + 3
    assert c.viol[k1][0] == offs[k1] and c.viol[k1][1]
    return c, offs[k1]


def test_sieve_hands_over_at_a_violating_frame(eng, sieve_low):
    """The sieve's link walks stop at implausible headers: its chain ends at or
    before the first violating frame and the exact walk emits the rest, the
    violating frames among it."""
    conn, first_bad = _sieved_stream()

    def sieve_state(mode):
        active, _, npath, pend = _last_sieve(eng)
        assert active == 1 and npath > 0 and pend <= first_bad, (mode[0], active, npath, pend, first_bad)

    paths = _one_batch(eng, [conn], V.V_ALL, after_step=sieve_state)
    assert set(paths.values()) == {2}, paths   # HVWS_PATH_SINGLE


# ------------------------------------------------- 5. hvws_rx_reads
@contextlib.contextmanager
def _validation(eng, vmask):
    L = libhv_amd.lib()
    old = L.hvws_set_validation(eng.ctx, vmask)
    try:
        yield
    finally:
        L.hvws_set_validation(eng.ctx, old)


class Reads:
    """A pinned arena holding one read per connection, laid out with gaps at
    every alignment; rank[k] is the place of table entry k in address order."""

    def __init__(self, eng, nbytes_max, rank):
        self.eng, self.rank = eng, rank
        L = libhv_amd.lib()
        self.size = nbytes_max + 48 * len(rank) + 64
        self.base = L.hvws_host_alloc(eng.ctx, self.size)
        assert self.base, L.hvws_last_error()
        self.carry = (libhv_amd.WsParser * len(rank))()
        for k in range(len(rank)):
            L.websocket_parser_init(ctypes.byref(self.carry[k]))

    def free(self):
        libhv_amd.lib().hvws_host_free(self.eng.ctx, self.base)

    def run(self, parts, carries=None):
        """hvws_rx_reads over `parts` (table order), from `carries` if given,
        else from this object's own (its last call's carry-out).
        Returns (frames, unmasked parts, carry-out)."""
        L = libhv_amd.lib()
        n = len(parts)
        assert n == len(self.rank) and all(len(p) <= 32 << 10 for p in parts)
        if carries is not None:
            for k in range(n):
                ctypes.memmove(ctypes.byref(self.carry[k]), ctypes.byref(carries[k]), ctypes.sizeof(libhv_amd.WsParser))
        offs, at = [0] * n, 0
        for j, k in enumerate(sorted(range(n), key=lambda k: self.rank[k])):
            at += (7 * j) % 41
            offs[k] = at
            at += len(parts[k])
        assert at <= self.size
        for k in range(n):
            ctypes.memmove(self.base + offs[k], parts[k], len(parts[k]))
        reads = (ctypes.c_void_p * n)(*[self.base + o for o in offs])
        lens = (ctypes.c_uint64 * n)(*[len(p) for p in parts])
        assert L.hvws_rx_reads(self.eng.ctx, reads, lens, self.carry, n, 1) == 0, L.hvws_last_error()
        frames = self.eng.frames()
        outs = [ctypes.string_at(self.base + offs[k], len(parts[k])) for k in range(n)]
        return frames, outs, [self.carry[k] for k in range(n)]


@functools.lru_cache(maxsize=None)
def _read_conns():
    rng = random.Random(4600)
    conns = []
    for i in range(24):
        data, _ = V.random_stream(300 + i, 20, tail_len64=(i % 5 == 0))
        conns.append(Conn(data, _cut_like_case1(rng, data, i % 2 == 1, i % 4 == 1)))
    assert all(len(p) <= 32 << 10 for c in conns for p in c.parts)
    return conns


@pytest.mark.parametrize("order", ["address", "shuffled"])
def test_rx_reads_two_rounds(eng, order):
    conns = _read_conns()
    cut = [c.cut_header_classes() for c in conns]
    assert sum(bool(v) for v in cut) >= 6, cut
    n = len(conns)
    rank = list(range(n))
    if order == "shuffled":
        random.Random(4601).shuffle(rank)
    reads = Reads(eng, max(sum(len(c.parts[p]) for c in conns) for p in (0, 1)), rank)
    try:
        with _validation(eng, V.V_ALL):
            for part in (0, 1):
                frames, outs, cout = reads.run([c.parts[part] for c in conns])
                _, started = eng.carry(n)
                tag = (order, "round", part + 1)
                _assert_table(frames, _expect_table(conns, part, [0] * n, V.V_ALL), tag)   # offsets relative to the read
                assert outs == [c.out[part] for c in conns], tag
                _assert_carry(cout, started, conns, part, tag)
    finally:
        reads.free()


# ------------------------------------------------- 6. one meaning of the carry across paths
# Each path takes part `part` of every connection from `carries`, checks its
# records and bytes and returns the carry it hands back (the library's own
# structs, padding byte included).
def _via_rx_batch(limit):
    def run(eng, conns, part, carries, tag):
        L = libhv_amd.lib()
        b = Batch(conns, part, V.V_ALL)
        host = b.buf.copy()
        old = L.hvws_set_small_batch_limit(eng.ctx, limit)
        try:
            cout = eng.rx_batch(host, b.segs, carries, True)
            frames = eng.frames()
        finally:
            L.hvws_set_small_batch_limit(eng.ctx, old)
        _assert_table(frames, b.exp, tag)
        assert np.array_equal(host, b.exp_bytes), tag
        return cout
    return run


def _via_step(mode):
    def run(eng, conns, part, carries, tag):
        with forced(eng, mode):
            return Batch(conns, part, V.V_ALL).step_checked(eng, mode, carries)[0]
    return run


def _via_rx_reads(eng, conns, part, carries, tag):
    n = len(conns)
    reads = Reads(eng, sum(len(c.parts[part]) for c in conns), list(range(n)))
    try:
        frames, outs, _ = reads.run([c.parts[part] for c in conns], carries)
        keep = (libhv_amd.WsParser * n)()   # a copy: the arena's carry table goes with it
        ctypes.memmove(keep, reads.carry, ctypes.sizeof(keep))
    finally:
        reads.free()
    _assert_table(frames, _expect_table(conns, part, [0] * n, V.V_ALL), tag)
    assert outs == [c.out[part] for c in conns], tag
    return [keep[k] for k in range(n)]


CARRY_PATHS = {"rx_batch_small": _via_rx_batch(0), "rx_batch_general": _via_rx_batch((1 << 64) - 1),
               "step_default": _via_step(("default", 0, -1)), "step_slack_noverify": _via_step(("slack_noverify", 1, 2, 0)),
               "rx_reads": _via_rx_reads}


def _run_part(eng, name, conns, part, carries):
    tag = (name, "batch", part + 1)
    cout = CARRY_PATHS[name](eng, conns, part, carries, tag)
    _assert_carry(cout, None, conns, part, tag)
    return cout


@pytest.mark.parametrize("first", sorted(CARRY_PATHS))
def test_carry_means_the_same_in_every_path(eng, first):
    """A connection's reads move between the paths from one poll iteration to
    the next: batch 1 through `first`, batch 2 through each of the five, from
    `first`'s carry."""
    conns = _header_conns()
    with _validation(eng, V.V_ALL):
        carry = _run_part(eng, first, conns, 0, None)
        keep = (libhv_amd.WsParser * len(conns))()
        for k, st in enumerate(carry):
            ctypes.memmove(ctypes.byref(keep[k]), ctypes.byref(st), ctypes.sizeof(libhv_amd.WsParser))
        for second in sorted(CARRY_PATHS):
            try:
                _run_part(eng, second, conns, 1, [keep[k] for k in range(len(conns))])
            except AssertionError as e:
                raise AssertionError(f"batch 1 through {first}, batch 2 through {second}: {e}") from e


# ------------------------------------------------- 7. RUN and validation
def test_run_step_keeps_the_mask_it_ran_under(eng):
    """A RUN step builds its records when they are first read: they must be
    those of the classes in force when the step ran (none -- a step under
    validation never takes the RUN path), not of a mask set in between."""
    L = libhv_amd.lib()
    rng = random.Random(4700)
    per_seg, nseg = 6, 64
    frames = []
    for i in range(nseg * per_seg):
        b0 = 0xC1 if i % 4 == 3 else 0x81   # every fourth frame has RSV1 set
        frames.append(_header(b0, 200, True, 1, rng.randbytes(4)) + rng.randbytes(200))
    assert {len(f) for f in frames} == {208}
    conns = [Conn(b"".join(frames[s * per_seg:(s + 1) * per_seg]), per_seg * 208) for s in range(nseg)]
    assert [v for c in conns for _, v in c.viol] == [V.V_RSV if i % 4 == 3 else 0 for i in range(len(frames))]
    off, on = Batch(conns, 0, 0), Batch(conns, 0, V.V_ALL)
    assert np.array_equal(off.exp["info"] & ~np.uint32(V_BITS), off.exp["info"])
    mode = ("run", 1, 1, -1, 1)
    with forced(eng, mode, 0):
        rx = eng.to_device(off.buf)
        try:
            eng.step(rx, len(off.buf), off.segs, None)
            assert L.hvws_last_scan_path(eng.ctx) == PATH_RUN
            L.hvws_set_validation(eng.ctx, V.V_ALL)
            got = rx.download(len(off.buf))
            recs = eng.frames()
            cout, started = eng.carry(nseg)
        finally:
            rx.free()
        assert not np.any(recs["info"] & np.uint32(V_BITS))
        _assert_table(recs, off.exp, "RUN step read under a later mask")
        assert np.array_equal(got, off.exp_bytes)
        _assert_carry(cout, started, conns, 0, "RUN step read under a later mask")
        # the same batch stepped under the mask, RUN still forced: not RUN, and
        # HVWS_V_RSV exactly on the RSV1 frames
        assert L.hvws_set_validation(eng.ctx, V.V_ALL) == V.V_ALL
        _, path = on.step_checked(eng, mode, None)
        assert path != PATH_RUN
        hdr = (on.exp["info"] & I_HDR) != 0
        assert [int(x) >> V_SHIFT & 63 for x in on.exp["info"][hdr]] == \
            [V.V_RSV if i % 4 == 3 else 0 for i in range(len(frames))]
