"""CPU: the joined-form oracle (tests/wsjoin.py) against the message layer.
Every stream of streams.quirk_streams() and 300 random ones, each cut three
ways (whole, 1-byte reads, random reads with empty ones), chained through
wsjoin.Chain: the HVWS_M_END pieces are the onMessage log, every piece has
total == len, and the state equals wsmsg.oracle_batch's."""
from __future__ import annotations

import random

import numpy as np

import streams
import wsharness as H
import wsjoin as J
import wsmsg as M

IMPL = "ref" if H.have_ref() else "oracle"


def _inputs():
    out = list(streams.quirk_streams())
    rng = random.Random(2024)
    for i in range(300):
        nf = rng.randrange(1, 9)
        if i % 3 == 0:
            frames = streams.rand_frames(rng, nf, max_len=300, edge=True)
        else:
            frames = J.mixed_frames(rng, nf, p_close=0.08)
        assert all(len(f[1]) <= 300 for f in frames)
        out.append((f"rand{i}", H.build_frames_ref(frames)))
    return out


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


def _frames(data: bytes):
    """(start, end, info) of every frame of a whole stream (the last may be cut short)."""
    recs = H.scan_segment(data)[0]
    return [(int(r["hdr_off"]), int(r["pay_off"]) + int(r["pay_len"]), int(r["info"])) for r in recs]


def _q5_across(frames, bounds) -> bool:
    """A control frame between two fragments, and a cut between the fragment
    before it and its end."""
    fragment_at = None   # start of the last non-final data frame while its message is open
    for a, b, info in frames:
        if info & 8:
            if fragment_at is not None and info & M.FIN and any(fragment_at < c < b for c in bounds):
                return True
        else:
            fragment_at = None if info & M.FIN else a
    return False


def _close_split(frames, bounds) -> bool:
    return any((info & 0xF) == 8 and any(a < c < b for c in bounds) for a, b, info in frames)


def test_chained_pieces_are_the_message_log():
    rng = random.Random(7)
    seen = {"span3": False, "q5": False, "empty_carrying": False, "close_split": False}
    nmsgs = 0
    for name, data in _inputs():
        log = H.run_messages(IMPL, data, [max(len(data), 1)])[0]
        nmsgs += len(log)
        frames = _frames(data)
        for how, reads in _cuts(rng, len(data)):
            ch = J.Chain(1)
            at = 0
            for n in reads:
                part = data[at:at + n]
                pend_in = int(ch.state["pending"][0])
                want_state = M.oracle_batch(part, [(0, n)], ch.carry, ch.state)[3]
                res = ch.run([part])
                at += n
                assert np.array_equal(res[3], want_state), (name, how, at)
                assert all(int(p["total"]) == int(p["len"]) for p in res[1]), (name, how, at)
                assert len(res[0]) == sum(int(p["len"]) for p in res[1]), (name, how, at)   # the table is dense
                if n == 0 and pend_in:
                    seen["empty_carrying"] = True
                    assert len(res[1]) == 1 and int(res[1][0]["rec"]) == J.NOREC and res[0] == ch.prev
            assert at == len(data)
            assert ch.logs[0] == log, (name, how)
            assert ch.totals_ok
            bounds = set(np.cumsum(reads).tolist())
            seen["span3"] |= ch.max_span >= 3
            seen["q5"] |= _q5_across(frames, bounds)
            seen["close_split"] |= _close_split(frames, bounds)
    assert nmsgs > 500
    assert all(seen.values()), seen
