"""CPU: the rules of hvws_check (include/hvws.h) as tests/wscheck.py restates
them -- the named streams' verdicts, and that a verdict does not depend on
where the batches cut the stream: (failed, close code, stream ordinal of the
failing frame) is the same fed whole, byte by byte and in random chunks, and a
failed connection stays failed in every later batch.

The size class's by-piece form is batch-granular by contract: its failing
record is the last one the open piece has in the batch that crossed the limit,
so there the data message's ordinal is compared instead of the frame's, and the
random streams that exercise it hold no other violation (an earlier batch end
can otherwise put the size verdict ahead of a violation that a larger batch
finds first)."""
from __future__ import annotations

import random

import pytest

import wscheck as C
import wsrfc as R
import wssend as S
import wsvalidate as V

TABLE = C.table()
IDS = [s.name for s in TABLE]


def _cuts(n: int, seed: int):
    r = random.Random(seed)
    out = []
    while sum(out) < n:
        out.append(r.randint(0, 9))
    return out


def _feedings(stream, classes, max_message, vmask, seeds=(1, 2)):
    n = len(stream)
    yield "whole", C.feed(stream, [n], classes, max_message, vmask)
    yield "bytes", C.feed(stream, [1] * n, classes, max_message, vmask)
    for k in seeds:
        yield f"chunks{k}", C.feed(stream, _cuts(n, k), classes, max_message, vmask)


def _verdict(ck: C.Checked, by_piece: bool):
    f = ck.failed[0]
    if f is None:
        return None
    return (f[1] if by_piece else f[0], f[2])


@pytest.mark.parametrize("st", TABLE, ids=IDS)
def test_named_stream_verdict(st):
    ck = C.feed(st.data, [len(st.data)], C.C_ALL, st.max_message, st.vmask)
    f = ck.failed[0]
    if st.want is None:
        assert f is None and int(ck.ck[0]) & C.CK_FAILED == 0
        return
    assert f is not None and (f[0], f[2]) == st.want, f
    assert int(ck.ck[0]) == C.CK_FAILED
    if st.why is not None:
        assert f[3] == st.why, f
    if st.by_piece:
        assert f[1] == st.msg


@pytest.mark.parametrize("st", TABLE, ids=IDS)
def test_named_stream_cut_invariance(st):
    want = None if st.want is None else ((st.msg, st.want[1]) if st.by_piece else st.want)
    for how, ck in _feedings(st.data, C.C_ALL, st.max_message, st.vmask):
        assert _verdict(ck, st.by_piece) == want, (how, ck.failed[0])
        assert ck.sticky_ok, how
        if want is None:
            assert int(ck.ck[0]) & C.CK_FAILED == 0, how
        else:
            assert int(ck.ck[0]) == C.CK_FAILED, how


def test_open_bit_is_carried_between_batches():
    """TEXT (no FIN) | CONTINUE + FIN | CONTINUE: the second batch is clean only
    because of the carried bit, the third fails because it was cleared."""
    a, b, c = C.B([(1, b"a")]), C.B([(0 | C.FIN, b"b")]), C.B([(0 | C.FIN, b"c")])
    ck = C.Checked(1)
    assert ck.run([a]).verdict[0].tolist() == [C.CK_OPEN]
    assert ck.run([b]).verdict[0].tolist() == [0] and ck.failed[0] is None
    w = ck.run([c])
    assert w.verdict[0].tolist() == [C.CK_FAILED] and w.verdict[2].tolist() == [C.C_SEQUENCE]
    # sticky, also over an empty read: fail_rec is the first record index
    w = ck.run([b""])
    assert [v.tolist() for v in w.verdict] == [[C.CK_FAILED], [0], [0], [0]]


@pytest.mark.parametrize("seed", range(12))
def test_random_stream_cut_invariance(seed):
    stream, _ = C.gen_stream(seed)
    got = {how: (_verdict(ck, False), ck.sticky_ok) for how, ck in _feedings(stream, C.C_ALL, 0, V.V_ALL)}
    assert len(set(got.values())) == 1 and got["whole"][1], got


def test_random_streams_fail_in_many_ways():
    seen, clean_prefix = set(), 0
    for seed in range(12):
        stream, nclean = C.gen_stream(seed)
        f = C.feed(stream, [len(stream)], C.C_ALL, 0, V.V_ALL).failed[0]
        if f:
            seen.add(f[3])
            assert f[0] >= nclean, (seed, f)   # the prefix is clean
            clean_prefix += 1
    assert len(seen) >= 4 and clean_prefix >= 8, seen


@pytest.mark.parametrize("seed", range(6))
def test_size_by_piece_cut_invariance(seed):
    """Well-formed fragmented traffic against a limit its larger messages cross."""
    stream = C.gen_fragmented(100 + seed)
    got = {how: (_verdict(ck, True), ck.sticky_ok) for how, ck in _feedings(stream, C.C_ALL, 12, 0)}
    assert len(set(got.values())) == 1 and got["whole"][1], got


def test_size_streams_do_fail():
    assert sum(1 for seed in range(6)
               if C.feed(C.gen_fragmented(100 + seed), [10 ** 6], C.C_ALL, 12).failed[0]) >= 4


def test_each_class_alone_and_none():
    for st in TABLE:
        if st.want is None or st.why is None:
            continue
        n = len(st.data)
        assert C.feed(st.data, [n], 0, st.max_message, st.vmask).failed[0] is None, st.name
        for c in C.CLASSES:
            f = C.feed(st.data, [n], c, st.max_message, st.vmask).failed[0]
            if st.name == "second_violation_ignored":
                continue   # its later frames break other classes
            if st.why & c:
                assert f is not None and f[3] == c and f[2] == C.CODE[c], (st.name, c, f)
            else:
                assert f is None, (st.name, c, f)


def test_replies_stop_at_the_failure():
    """TEXT "hi", PING, a Close with code 1005, PING: the echo and the first PONG
    only; the same with a good Close: its echo too, and nothing after it."""
    policy = S.R_SERVER | S.R_ECHO
    bad = C.B([(1 | C.FIN, b"hi"), (9 | C.FIN, b"p1"), C.close(1005), (9 | C.FIN, b"p2")])
    good = C.B([(1 | C.FIN, b"hi"), (9 | C.FIN, b"p1"), C.close(1000), (9 | C.FIN, b"p2")])
    ck = C.Checked(2)
    w = ck.run([bad, good])
    _, fail, why, code = w.verdict
    assert fail.tolist() == [2, C.NONE] and why.tolist() == [C.C_CLOSE_BODY, 0] and code.tolist() == [1002, 0]
    out, table = w.rfc[0], w.rfc[1]
    rep, _, (first, count), flags = C.replies_checked_of(table, 2, policy, fail)
    got = [[(fl, out[o:o + ln]) for o, ln, fl, _ in rep[first[s]:first[s] + count[s]]] for s in range(2)]
    assert got[0] == [(1 | C.FIN, b"hi"), (10 | C.FIN, b"p1")]
    assert got[1] == [(1 | C.FIN, b"hi"), (10 | C.FIN, b"p1"), (8 | C.FIN, C.close(1000)[1])]
    assert flags == [C.RF_FAILED | C.RF_CLOSED, C.RF_CLOSED]
    # hvws_replies itself still echoes the bad Close
    rep0, _, (f0, c0), fl0 = R.replies_of(table, 2, policy)
    assert [fl for _, _, fl, _ in rep0[f0[0]:f0[0] + c0[0]]] == [1 | C.FIN, 10 | C.FIN, 8 | C.FIN] and fl0 == [1, 1]
