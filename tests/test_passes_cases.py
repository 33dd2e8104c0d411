"""CPU: the cases of tests/passcases.py are what they claim -- the cuts, the
frame mixes, the verdicts, the alignments and the record counts that send a
batch down its scan path -- and cutting a stream changes no message: the
two-batch oracles deliver what the uncut stream does."""
from __future__ import annotations

import numpy as np

import passcases as P
import wsharness as H
import wsmsg as M
import wsrfc as R
import wsutf8 as U


def _two_batches(case: P.Case):
    """(Expect of batch 1, Expect of batch 2 from batch 1's states, Expect of the uncut streams)."""
    n = len(case.conns)
    e1 = P.expect(*case.batches[0], None, P.fresh(n, case.raw))
    st = e1.next()
    e2 = P.expect(*case.batches[1], st.parser, st)
    return e1, e2, P.expect(*case.whole, None, P.fresh(n, case.raw))


def _frame_flags(conn: bytes):
    return [int(x) & 0x3F for x in H.scan_segment(conn)[0]["info"]]


def test_case1_is_what_it_claims():
    case = P.case1()
    n = len(case.conns)
    assert n == 40 and case.cuts_in_header() >= 15
    ping_inside = close_then_more = 0
    illegal = set()
    for k, c in enumerate(case.conns):
        flags = _frame_flags(c)
        assert len(flags) == 40
        is_open = inside = False
        for fl in flags:
            if fl & 0xF < 8:
                if bool(fl & 0xF) == is_open:   # a new opcode inside a message, or a lone continuation
                    illegal.add(k)
                is_open = not fl & M.FIN
            elif fl & 0xF == 9 and is_open:
                inside = True
        ping_inside += inside
        close_then_more += 8 in [fl & 0xF for fl in flags[:-1]]
    assert ping_inside >= 8 and close_then_more >= 5, (ping_inside, close_then_more)
    assert illegal == set(case.raw) and len(illegal) == 4, (illegal, case.raw)   # only these skip the rec / bad join
    e1, e2, _ = _two_batches(case)
    rejected = sum(int(x) == U.REJ for x in e2.u8)
    assert rejected >= 10 and n - rejected >= 10, rejected
    d1 = e1.rfc[3]["data"]   # a text message open across the boundary (a REJECT word hides HVWS_U8_TEXT_OPEN)
    assert int(((d1["open"] == 1) & (d1["opcode"] == 1)).sum()) >= 5, d1.tolist()
    assert sum(bool(int(x) & U.TEXT_OPEN) for x in e1.u8) >= 3, e1.u8
    assert any(ln == 0 for _, ln in case.batches[1][1])
    mis = set()
    for e in (e1, e2):
        lens = e.recs["pay_len"].astype(np.int64)
        out_off = np.cumsum(lens) - lens
        mis |= {int(x) for x in ((e.recs["pay_off"].astype(np.int64) - out_off) % 16)[lens > 0]}
    assert len(mis) >= 12, sorted(mis)
    # payloads of 0 to 300 bytes, some frames unmasked, some empty
    infos = np.concatenate([H.scan_segment(c)[0]["info"] for c in case.conns])
    lens = np.concatenate([H.scan_segment(c)[0]["pay_len"] for c in case.conns])
    assert int(lens.max()) <= 300 and int((lens == 0).sum()) > 50 and int(((infos & M.MASK) == 0).sum()) > 50


def test_case2_frames_of_a_connection_have_one_size():
    case = P.case2()
    assert len(case.conns) == 32
    for c, cut in zip(case.conns, case.cuts):
        hs = P.headers(c)
        assert len(hs) == 48 and len(c) == 48 * 208
        assert [a for a, _ in hs] == list(range(0, len(c), 208)) and all(b - a == 8 for a, b in hs)
        assert all(fl & M.MASK for fl in _frame_flags(c))
        assert cut % 208 != 0   # inside a frame
    assert case.cuts_in_header() == 16
    e1, e2, _ = _two_batches(case)
    rejected = sum(int(x) == U.REJ for x in e2.u8)
    assert rejected >= 8 and len(case.conns) - rejected >= 8, rejected


def test_case3_dense_segment_outgrows_its_region():
    (thin, tsegs), (dense, dsegs) = P.case3()
    assert len(tsegs) == len(dsegs) == 16
    counts = lambda data, segs: [len(H.scan_segment(data[o:o + n])[0]) for o, n in segs]
    assert counts(thin, tsegs) == [2] * 16
    d = counts(dense, dsegs)
    assert d[7] > 1.5 * 2 + 16 and d[:7] + d[8:] == [2] * 15, d


def test_case4_streams():
    data = P.case4_checked()
    nfr = len(P.headers(data))
    # the record bound exceeds the table sized from the first guess, so the count is checked; the records fit
    assert len(data) // 2 + 3 > P.Overflow.FIRST_TABLE > nfr
    assert 900 <= len(data) // nfr <= 1200, len(data) // nfr
    clean, quirks, cut = P.case4_sieved()
    assert 230 << 10 <= len(clean) <= 290 << 10
    for fl, (a, b), (_, nxt) in zip(_frame_flags(clean), P.headers(clean), P.headers(clean)[1:] + [(0, len(clean))]):
        assert fl & M.MASK and fl & 0xF in (0, 1, 2, 8, 9, 10)
        assert fl & 0xF < 8 or (fl & M.FIN and nxt - b <= 125 + 14)
    qf = _frame_flags(quirks)
    assert len(qf) == len(_frame_flags(clean)) + 2 and sum(not fl & M.MASK for fl in qf) == 1
    a, b = P.headers(clean)[-1]
    assert a < cut < b


def test_case4_overflow_stream_and_its_numpy_expectation():
    ov = P.overflow()
    data = ov.wire.tobytes()
    recs, _, _, plain = H.scan_segment(data)
    assert len(recs) == ov.n > ov.FIRST_TABLE > 1 << 20
    want = np.uint32(M.I_HDR | M.I_END | M.FIN)
    assert np.all(recs["info"] & want == want)
    assert np.array_equal(recs["pay_len"], ov.lens) and np.array_equal(np.frombuffer(plain, np.uint8), ov.plain)
    k = 5000
    part = data[:int(ov.off[k])]
    out, table, (first, count), st, words, u8, bad = ov.expect(k)
    mout, mtable, (mfirst, mcount), mst = M.oracle_batch(part, [(0, len(part))])
    assert out == mout and table.tolist() == mtable.tolist()
    assert (first.tolist(), count.tolist(), st.tolist()) == (mfirst.tolist(), mcount.tolist(), mst.tolist())
    _, uwords, ust, ubad, _, _ = U.oracle_batch(part, [(0, len(part))])
    assert np.array_equal(words, uwords) and u8.tolist() == ust.tolist() and bad.tolist() == ubad.tolist()
    assert int((ov.lens[:k] > 0).sum()) > 500 and int((ov.lens[:k] == 0).sum()) > 3000


def _logs(n, *expects):
    """Per connection: the RFC form's whole messages [(is control, opcode, bytes)] and what a caller of
    hvws_messages joins from its pieces [(opcode, bytes)], over the batches in order."""
    rfc = [[] for _ in range(n)]
    joiners = [M.Joiner() for _ in range(n)]
    for e in expects:
        for seg, ctl, op, body in R.messages_of(e.rfc[0], e.rfc[1]):
            rfc[seg].append((ctl, op, body))
        out, table, (first, count), _ = e.msg
        for s in range(n):
            joiners[s].feed(out, table[int(first[s]): int(first[s]) + int(count[s])])
    assert all(j.totals_ok for j in joiners)
    return rfc, [j.msgs for j in joiners]


def test_cutting_a_stream_changes_no_message():
    for case in (P.case1(), P.case2()):
        n = len(case.conns)
        e1, e2, whole = _two_batches(case)
        cut_rfc, cut_msgs = _logs(n, e1, e2)
        whole_rfc, whole_msgs = _logs(n, whole)
        assert cut_rfc == whole_rfc
        assert cut_msgs == whole_msgs
        assert sum(len(x) for x in whole_msgs) > 10 * n
        # the verdicts do not depend on the cut either
        assert [int(x) for x in e2.u8] == [int(x) for x in whole.u8]
