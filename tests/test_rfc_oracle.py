"""CPU: the RFC-form oracle (tests/wsrfc.py).  The Q5 stream; parity with the
message layer on streams whose control frames lie between messages (there the
reference's rule and RFC 6455's agree); independence of where single-segment
batches cut a stream with control frames inside messages; and, without control
records, equality with the joined form's oracle apart from the Q6 opcode."""
from __future__ import annotations

import random

import numpy as np

import wsharness as H
import wsjoin as J
import wsmsg as M
import wsrfc as R

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])

Q5 = [(1 | MASK, b"AB", KEY), (9 | FIN | MASK, b"PING", KEY), (0 | FIN | MASK, b"CD", KEY)]


def _cuts(rng: random.Random, n: int):
    yield "whole", [n]
    yield "bytes", [1] * n
    reads, tot = [], 0
    while tot < n:
        c = rng.choice([0, 0, rng.randint(1, 7), rng.randint(1, 40), rng.randint(1, 400)])
        c = min(c, n - tot)
        reads.append(c)
        tot += c
    yield "random", reads


def test_q5_stream_keeps_the_ping_out_of_the_text():
    data = H.build_frames_ref(Q5)
    assert H.run_messages("oracle", data, [len(data)])[0] == [(9, b"ABPING"), (9, b"CD")]   # the reference's rule
    for cut in range(len(data) + 1):
        ch = R.run_stream(data, [cut, len(data) - cut])
        assert ch.data_log[0] == [(1, b"ABCD")], cut
        assert ch.ctl_log[0] == [(9, b"PING")], cut
        assert ch.merged[0] == [(9, b"PING"), (1, b"ABCD")], cut
        assert ch.totals_ok
    ch = R.run_stream(data, [1] * len(data))
    assert (ch.data_log[0], ch.ctl_log[0]) == ([(1, b"ABCD")], [(9, b"PING")])
    st = ch.state[0]
    assert tuple(st["data"]) == (0, 1, 0) and tuple(st["ctl"]) == (0, 9, 0) and int(st["data_off"]) == 0


def _between_frames(rng: random.Random, nmsg: int):
    """Messages of 1-4 fragments, the first with opcode 1 or 2, and final control
    frames only between them: by construction, so no stream is left out."""
    out = []
    for _ in range(nmsg):
        while rng.random() < 0.4:
            n = rng.choice([0, 1, rng.randrange(126)])
            out.append((rng.choice([8, 9, 9, 10]) | FIN | (0 if rng.random() < 0.1 else MASK), rng.randbytes(n),
                        rng.randbytes(4)))
        k = rng.randrange(1, 5)
        for j in range(k):
            n = rng.choice([0, 1, rng.randrange(126), rng.randrange(301)])
            fl = (rng.choice([1, 2]) if j == 0 else 0) | (FIN if j == k - 1 else 0) | (0 if rng.random() < 0.1 else MASK)
            out.append((fl, rng.randbytes(n), rng.randbytes(4)))
    return out


def test_parity_with_the_message_layer_when_control_frames_lie_between_messages():
    rng = random.Random(6455)
    nmsgs = nctl = 0
    for i in range(150):
        frames = _between_frames(rng, rng.randrange(1, 6))
        assert frames[0][0] & 0xF   # the first frame latches an opcode
        data = H.build_frames_ref(frames)
        cutoff = rng.choice([len(data), len(data), rng.randrange(len(data) + 1)])   # some end inside a frame
        data = data[:cutoff]
        for how, reads in _cuts(rng, len(data)):
            want = H.run_messages("oracle", data, reads if reads else [0])[0]
            ch = R.run_stream(data, reads)
            assert ch.merged[0] == want, (i, how)
            assert ch.totals_ok
        nmsgs += len(ch.data_log[0])
        nctl += len(ch.ctl_log[0])
    assert nmsgs > 200 and nctl > 100


def test_logs_do_not_depend_on_the_cuts():
    rng = random.Random(54)
    inside = 0
    for i in range(60):
        frames = J.mixed_frames(rng, rng.randrange(2, 8), p_close=0.08, max_len=60)
        data = H.build_frames_ref(frames)
        whole = R.run_stream(data, [len(data)])
        dlog, clog = whole.data_log[0], whole.ctl_log[0]
        # a control frame inside a message: the reference's rule gives another log
        inside += H.run_messages("oracle", data, [max(len(data), 1)])[0] != whole.merged[0]
        if i < 12:   # every cut position of a short stream
            for cut in range(len(data) + 1):
                ch = R.run_stream(data, [cut, len(data) - cut])
                assert (ch.data_log[0], ch.ctl_log[0]) == (dlog, clog), (i, cut)
        for how, reads in _cuts(rng, len(data)):
            ch = R.run_stream(data, reads)
            assert (ch.data_log[0], ch.ctl_log[0]) == (dlog, clog), (i, how)
            assert ch.totals_ok
            if how == "bytes":   # a control frame's pending bytes were carried
                assert all(op >= 8 for op, _ in clog) and all(op < 8 for op, _ in dlog)
    assert inside > 10


def test_without_control_records_it_is_the_joined_form():
    rng = random.Random(99)
    q6 = pieces = 0
    for i in range(80):
        frames = []
        for _ in range(rng.randrange(1, 9)):
            n = rng.choice([0, 1, rng.randrange(126), rng.randrange(301)])
            frames.append((rng.choice([0, 0, 1, 2, 3]) | (FIN if rng.random() < 0.6 else 0)
                           | (0 if rng.random() < 0.1 else MASK), rng.randbytes(n), rng.randbytes(4)))
        data = H.build_frames_ref(frames)
        for how, reads in _cuts(rng, len(data)):
            a, b = J.Chain(1), R.Chain(1)
            at = 0
            for n in reads:
                part = data[at:at + n]
                at += n
                want, got = a.run([part]), b.run([part])
                assert got[0] == want[0], (i, how, at)
                assert len(got[1]) == len(want[1])
                for f in ("off", "len", "total", "rec", "seg"):
                    assert np.array_equal(got[1][f], want[1][f]), (i, how, at, f)
                for g, w in zip(got[1], want[1]):
                    gi, wi = int(g["info"]), int(w["info"])
                    pieces += 1
                    if wi & 0xF == 8:   # no data frame has opcode 8: nothing was latched (Q6)
                        q6 += 1
                        assert gi == wi & ~0xF, (i, how, at)
                    else:
                        assert gi == wi, (i, how, at)
                assert got[2][0].tolist() == want[2][0].tolist() and got[2][1].tolist() == want[2][1].tolist()
                st = got[3][0]
                assert tuple(int(x) for x in st["data"]) == tuple(int(x) for x in want[3][0]), (i, how, at)
                assert int(st["data_off"]) == int(want[4][0])
                assert tuple(int(x) for x in st["ctl"]) == (0, 0, 0) and int(st["ctl_off"]) == 0
    assert q6 > 20 and pieces > 1000
