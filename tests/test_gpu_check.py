"""GPU: hvws_check and hvws_replies_checked (include/hvws.h) against the rules
restated in tests/wscheck.py: the named streams whole and cut inside the
offending frame, each class alone, a long connection against the same records
spread over many, behind every scan path, the calling rules, and a server turn
that fails one connection and closes the other.

The named streams carry their own settings (validation classes, max_message);
streams of one setting share a batch, each as a connection of its own."""
from __future__ import annotations

import numpy as np
import pytest

import libhv_amd
import passcases as P
import wscheck as C
import wsharness as H
import wsrfc as R
import wssend as S
from test_gpu_parity import spec_min   # noqa: F401 -- a fixture
from test_gpu_passes_paths import _ALL, _ALL_IDS, _learn, _scan, _wanted_path
from test_gpu_validate_paths import forced

pytestmark = pytest.mark.gpu

EINVAL = -2
CAP = 4096
POLICY = S.R_SERVER | S.R_ECHO
TABLE = C.table()


def _groups():
    """The named streams by (validation classes, max_message)."""
    out = {}
    for st in TABLE:
        out.setdefault((st.vmask, st.max_message), []).append(st)
    return sorted(out.items())


GROUPS = _groups()
GROUP_IDS = [f"v{v}_max{m}" for (v, m), _ in GROUPS]


def _copy(p):
    return libhv_amd.WsParser.from_buffer_copy(bytes(p))


class Checks:
    """A chain of batches on the device: scan (under the chain's validation
    classes, from the engine's own parser carry), hvws_utf8, hvws_messages_rfc,
    hvws_check; records, pieces, bad[] and the whole verdict of every batch
    against wscheck.Checked."""

    def __init__(self, eng, nconn: int, classes: int = C.C_ALL, max_message: int = 0, vmask: int = 0, cap: int = CAP):
        self.eng, self.n, self.cap = eng, nconn, cap
        self.ck = C.Checked(nconn, classes, max_message, vmask)
        self.outs = [eng.alloc(cap + 64), eng.alloc(cap + 64)]
        self.gcarry = [None] * nconn
        self.prev_len = 0
        self.last = None

    def batch(self, reads, after=None):
        eng, ck, k = self.eng, self.ck, self.ck.ch.batches
        L = libhv_amd.lib()
        data, segs, conns, _, st = ck.ch.inputs(reads)
        want = ck.oracle(reads)
        nseg = len(segs)
        rx = eng.to_device(np.frombuffer(data, np.uint8))
        cur, old = self.outs[k % 2], self.outs[(k + 1) % 2]
        was = L.hvws_set_validation(eng.ctx, ck.vmask)
        try:
            eng.scan(rx, len(data), segs, [self.gcarry[c] for c in conns])
            eng.utf8(rx, len(data), True, ck.u8[conns])
            eng.messages_rfc(rx, len(data), True, cur, self.cap, st, old if k else None, self.prev_len)
            eng.check(ck.classes, ck.max_message, ck.ck[conns])
            got = eng.check_result(nseg)
            assert eng.frames()["info"].tolist() == [x for seg in want.infos for x in seg], k
            assert eng.utf8_result(nseg)[1].tolist() == want.u8[1].tolist(), k
            assert eng.message_table().tolist() == want.rfc[1].tolist(), k
            for name, g, w in zip(("state_out", "fail_rec", "why", "code"), got, want.verdict):
                assert g.tolist() == w.tolist(), (name, k)
            cout, _ = eng.carry(nseg)
            for i, c in enumerate(conns):
                self.gcarry[c] = _copy(cout[i])
            if after:
                after(want, cur, data, nseg)
        finally:
            L.hvws_set_validation(eng.ctx, was)
            eng.sync()
            rx.free()
        ck.take(want, reads)
        self.prev_len = len(want.rfc[0])
        self.last = want
        return want

    def free(self):
        for b in self.outs:
            b.free()


def _expected(ck: C.Checked, streams) -> None:
    """Every stream's first failure is the table's."""
    for c, st in enumerate(streams):
        f = ck.failed[c]
        if st.want is None:
            assert f is None, (st.name, f)
        elif st.by_piece:
            assert f is not None and (f[1], f[2]) == (st.msg, st.want[1]), (st.name, f)
        else:
            assert f is not None and (f[0], f[2]) == st.want, (st.name, f)
    assert ck.sticky_ok


# --------------------------------- 1. the named streams, whole
@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_named_streams_one_batch(eng, group):
    (vmask, max_message), streams = group
    t = Checks(eng, len(streams), C.C_ALL, max_message, vmask)
    try:
        want = t.batch([st.data for st in streams])
        _expected(t.ck, streams)
        for c, st in enumerate(streams):
            if st.why is not None:
                assert int(want.verdict[2][c]) == st.why, st.name
        # failed is sticky, over an empty read (no records) and over a PING; the others carry their open bit
        ping = C.B([(9 | C.FIN, b"again")])
        again = t.batch([b"" if c % 2 else ping for c in range(len(streams))])
        _expected(t.ck, streams)
        for c, st in enumerate(streams):
            assert (int(again.verdict[0][c]) == C.CK_FAILED) == (st.want is not None), st.name
    finally:
        t.free()


# --------------------------------- 2. cut inside the offending frame
def _frame_span(st: C.Stream):
    """(first header byte, first payload byte, end) of the offending frame (a
    clean stream: its last frame), the end clipped to the stream."""
    recs = H.scan_segment(st.data)[0]
    r = recs[st.want[0] if st.want is not None and not st.by_piece else len(recs) - 1]
    a, b = int(r["hdr_off"]), int(r["pay_off"])
    return a, b, min(b + int(r["length"]), len(st.data))


def _positions(st: C.Stream):
    a, b, e = _frame_span(st)
    return list(range(a + 1, e)) or [a + 1]   # header-interior, the header's end, body-interior


@pytest.mark.parametrize("pieces", [2, 3])
@pytest.mark.parametrize("group", GROUPS, ids=GROUP_IDS)
def test_named_streams_cut_inside_the_offending_frame(eng, group, pieces):
    """Round j cuts every stream of the group at its j-th position inside the
    offending frame (a shorter list wraps around): two batches, or three with a
    middle batch of one byte -- a Close body cut after its first byte arrives by
    the control class's carry."""
    (vmask, max_message), streams = group
    pos = [_positions(st) for st in streams]
    assert any(a + 1 < b for a, b, _ in map(_frame_span, streams))   # some header is cut inside
    for j in range(max(len(p) for p in pos)):
        t = Checks(eng, len(streams), C.C_ALL, max_message, vmask)
        try:
            cuts = []
            for st, p in zip(streams, pos):
                k = p[j % len(p)]
                cuts.append([0, k, len(st.data)] if pieces == 2 else [0, k, min(k + 1, len(st.data)), len(st.data)])
            for b in range(pieces):
                reads = [st.data[c[b]:c[b + 1]] for st, c in zip(streams, cuts)]
                if any(reads):   # (a stream cut before its last byte leaves nothing for a third batch)
                    t.batch(reads)
            _expected(t.ck, streams)
        finally:
            t.free()


# --------------------------------- 3. each class alone
@pytest.mark.parametrize("classes", [0] + list(C.CLASSES))
def test_each_class_alone(eng, classes):
    """A violation of a disabled class is not reported; classes = 0 fails nothing."""
    seen = 0
    for (vmask, max_message), streams in GROUPS:
        t = Checks(eng, len(streams), classes, max_message, vmask)
        try:
            want = t.batch([st.data for st in streams])
            why = want.verdict[2].tolist()
            assert all(w in (0, classes) for w in why), why
            seen += sum(1 for w in why if w)
            for st, w in zip(streams, why):
                if st.why is not None and st.name != "second_violation_ignored":
                    assert w == st.why & classes, (st.name, w)
        finally:
            t.free()
    assert seen > 0 if classes else seen == 0


# --------------------------------- 4. one long connection and the same records spread
def _spread_frames():
    """5000 one-byte TEXT frames; record 1023 leaves its message open and
    record 1024 continues it (across the scan's first block boundary); record
    4097 is a lone CONTINUE."""
    frames = []
    for r in range(5000):
        fl = 1 | C.FIN
        if r == 1023:
            fl = 1
        elif r in (1024, 4097):
            fl = 0 | C.FIN
        frames.append(H.build_frames_ref([(fl | C.MASK, bytes([65 + r % 26]), C.KEY)]))
    return frames


def test_one_long_connection(eng):
    frames = _spread_frames()
    t = Checks(eng, 1, cap=40960)
    try:
        want = t.batch([b"".join(frames)])
        assert want.verdict[1].tolist() == [4097] and want.verdict[3].tolist() == [1002]
    finally:
        t.free()


def test_the_same_records_spread_over_connections(eng):
    """Connection 1024's lone CONTINUE must not see connection 1023's open message."""
    frames = _spread_frames()
    t = Checks(eng, len(frames), cap=40960)
    try:
        want = t.batch(frames)
        fail = want.verdict[1]
        assert np.flatnonzero(fail != np.uint64(C.NONE)).tolist() == [1024, 4097]
        assert int(want.verdict[0][1023]) == C.CK_OPEN
    finally:
        t.free()


# --------------------------------- 5. behind every scan path
@pytest.mark.parametrize("mode,how", _ALL, ids=_ALL_IDS)
def test_check_behind_every_scan_path(spec_min, mode, how):
    """passcases.case1 (40 mixed connections cut once) under every scan mode:
    hvws_utf8, hvws_messages_rfc and hvws_check behind the forced path -- after a
    RUN step the records are built first -- both batches, the second from the
    first's verdicts; max_message = 200 so that the size class takes part.  A
    context of its own: a forced RUN step over mixed frames fails its hypothesis,
    and the context then holds RUN back for its next 16 steps."""
    with libhv_amd.Engine(0) as own:
        _check_behind(own, mode, how)


def _check_behind(eng, mode, how):
    case = P.case1()
    st, prev, ck_in, carries = P.fresh(len(case.conns), case.raw), None, None, None
    whys = set()
    with forced(eng, mode):
        for data, segs in case.batches:
            nseg = len(segs)
            rx = eng.to_device(np.frombuffer(data, np.uint8))
            run = None
            try:
                if "slack" in mode[0]:
                    _learn(eng, rx, data, segs, carries)
                path = _scan(eng, mode, how, rx, len(data), segs, carries)
                assert path == _wanted_path(mode, uniform=False), (mode[0], how, path)
                run = P.Run(eng, rx, data, segs, carries, how, st, prev)
                e = run.e
                run.q_utf8()
                run.q_rfc()
                eng.check(C.C_ALL, 200, ck_in)
                got = eng.check_result(nseg)
                ends = list(e.firsts[1:]) + [len(e.recs)]
                infos = [[int(x) for x in e.recs["info"][a:b]] for a, b in zip(e.firsts, ends)]
                lens = [[int(x) for x in e.recs["length"][a:b]] for a, b in zip(e.firsts, ends)]
                want = C.check_batch(infos, lens, e.firsts, e.rfc[1], e.rfc[0], ck_in, C.C_ALL, 200, e.bad)
                for name, g, w in zip(("state_out", "fail_rec", "why", "code"), got, want):
                    assert g.tolist() == w.tolist(), (name, mode[0], how)
                whys |= set(want[2].tolist())
                eng.sync()
                run.out_m.free()
                run.out_j.free()
                if prev is not None:
                    prev.free()
                st, prev, ck_in, carries = e.next(), P.Prev(None, 0, run.out_r, len(e.rfc[0])), want[0], e.carry
                run = None
            finally:
                eng.sync()
                if run:
                    run.free()
                rx.free()
    if prev is not None:
        prev.free()
    assert 0 in whys and len(whys) >= 4, whys   # clean connections and several kinds of failure


# --------------------------------- 6. the calling rules
def test_calling_rules(eng):
    L = libhv_amd.lib()
    data = C.B([(1 | C.FIN, b"hi"), (9 | C.FIN, b"p")])
    n, segs = len(data), [(0, len(data))]
    rx = eng.to_device(np.frombuffer(data, np.uint8))
    out = eng.alloc(CAP)
    word = np.zeros(1, np.uint32)
    try:
        with libhv_amd.Engine(0) as fresh:   # before any message call
            assert L.hvws_check(fresh.ctx, C.C_ALL & ~C.C_TEXT_UTF8, 0, None) == EINVAL
            assert L.hvws_replies_checked(fresh.ctx, POLICY, None) == EINVAL
            assert not L.hvws_check_device(fresh.ctx)
        eng.scan(rx, n, segs)
        eng.messages(rx, n, True, out, CAP)
        assert L.hvws_check(eng.ctx, C.C_SEQUENCE, 0, None) == EINVAL
        eng.messages_joined(rx, n, True, out, CAP)
        assert L.hvws_check(eng.ctx, C.C_SEQUENCE, 0, None) == EINVAL
        eng.messages_rfc(rx, n, True, out, CAP)
        assert L.hvws_replies_checked(eng.ctx, POLICY, None) == EINVAL            # no check on this message call
        assert L.hvws_check(eng.ctx, C.C_TEXT_UTF8, 0, None) == EINVAL              # no hvws_utf8 on this scan
        assert L.hvws_check(eng.ctx, 1 << 6, 0, None) == EINVAL                     # no such class
        word[0] = 4
        assert L.hvws_check(eng.ctx, C.C_SEQUENCE, 0, word.ctypes.data) == EINVAL   # bit 2 of a state word
        word[0] = C.CK_OPEN
        eng.check(C.C_SEQUENCE, 0, word)
        assert [v.tolist() for v in eng.check_result(1)] == [[C.CK_FAILED], [0], [C.C_SEQUENCE], [1002]]
        assert L.hvws_check_device(eng.ctx)
        eng.replies_checked(POLICY)
        assert eng.reply_flags(1).tolist() == [C.RF_FAILED | C.RF_CLOSED] and len(eng.reply_table()[0]) == 0
        ms = eng.last_kernel_ms()
        eng.check(C.C_SEQUENCE, 0, None)
        assert eng.last_kernel_ms() >= 0 and ms >= 0
        # an hvws_utf8 of an earlier scan does not serve; one of this scan does
        eng.utf8(rx, n, True)
        eng.check(C.C_ALL, 0, None)
        eng.scan(rx, n, segs)
        assert L.hvws_check(eng.ctx, C.C_SEQUENCE, 0, None) == EINVAL               # a scan since hvws_messages_rfc
        eng.messages_rfc(rx, n, True, out, CAP)
        assert L.hvws_check(eng.ctx, C.C_ALL, 0, None) == EINVAL                    # hvws_utf8 ran over the scan before
        assert L.hvws_replies_checked(eng.ctx, POLICY, None) == EINVAL              # the check was another call's
        eng.check(C.C_ALL & ~C.C_TEXT_UTF8, 0, None)
        assert [v.tolist() for v in eng.check_result(1)] == [[0], [C.NONE], [0], [0]]
    finally:
        eng.sync()
        rx.free()
        out.free()


# --------------------------------- 7. the server turn
def test_turn_fails_one_connection_and_closes_the_other(eng):
    """A: TEXT "hi", PING, a Close of code 1005, PING.  B: the same with a good
    Close.  hvws_replies_checked + hvws_send_messages: A's bytes are the echo and
    the first PONG, flags FAILED | CLOSED; B's the echo, the PONG and the Close
    echo, flags CLOSED.  hvws_replies on the same batch still gives today's
    tables (wsrfc.replies_of unchanged): A's Close is echoed."""
    a = C.B([(1 | C.FIN, b"hi"), (9 | C.FIN, b"p1"), C.close(1005), (9 | C.FIN, b"p2")])
    b = C.B([(1 | C.FIN, b"hi"), (9 | C.FIN, b"p1"), C.close(1000), (9 | C.FIN, b"p2")])
    frames = lambda msgs: S.expected([(fl, d, 0) for fl, d in msgs], 0, False)[0]
    tx = eng.alloc(2 * CAP)
    moff = eng.alloc(8 * 1024)
    t = Checks(eng, 2)

    def turn(want, cur, data, nseg):
        table = want.rfc[1]
        out = want.rfc[0]
        for checked in (True, False):
            if checked:
                eng.replies_checked(POLICY)
                rep, answered, fc, flags = C.replies_checked_of(table, nseg, POLICY, want.verdict[1])
            else:
                eng.replies(POLICY)
                rep, answered, fc, flags = R.replies_of(table, nseg, POLICY)
            d_table, d_n, n = eng.replies_device()
            nbytes, _ = eng.send_messages(tx, 2 * CAP, cur, CAP, d_table, n, d_n, 0, False, moff)
            got_table, piece = eng.reply_table()
            assert [tuple(int(x) for x in r) for r in got_table.tolist()] == rep, checked
            assert piece.tolist() == answered, checked
            first, count = eng.segment_replies(nseg)
            assert (first.tolist(), count.tolist()) == (fc[0], fc[1]), checked
            assert eng.reply_flags(nseg).tolist() == flags, checked
            offs = moff.download(8 * (len(rep) + 1), np.uint64).tolist()
            sent = bytes(tx.download(nbytes))
            per = [sent[offs[int(first[s])]: offs[int(first[s]) + int(count[s])]] for s in range(nseg)]
            pong, echo = (10 | C.FIN, b"p1"), (1 | C.FIN, b"hi")
            if checked:
                assert per[0] == frames([echo, pong]) and flags[0] == C.RF_FAILED | C.RF_CLOSED
            else:
                assert per[0] == frames([echo, pong, C.close(1005)]) and flags[0] == C.RF_CLOSED
            assert per[1] == frames([echo, pong, C.close(1000)]) and flags[1] == C.RF_CLOSED

    try:
        want = t.batch([a, b], after=turn)
        assert want.verdict[1].tolist() == [2, C.NONE] and want.verdict[3].tolist() == [1002, 0]
    finally:
        t.free()
        tx.free()
        moff.free()
