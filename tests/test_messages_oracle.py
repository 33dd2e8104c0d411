"""CPU: tests/wsmsg.py -- the message rule hvws_messages implements, restated
over frame records -- against the message layer itself: the pieces of a stream,
joined over batches, are the onMessage log of oracle/ws_msg.cpp and, where it
was built, of the compiled reference.  Every quirk stream and 300 random
streams; whole, in 1-byte reads and in random reads."""
from __future__ import annotations

import random

import pytest

import streams
import wsharness as H
import wsmsg as M

IMPLS = ["oracle"] + (["ref"] if H.have_ref() else [])


def _cases():
    out = list(streams.quirk_streams())
    rng = random.Random(20240611)
    for i in range(300):
        out.append((f"rand{i}", streams.rand_stream(rng, rng.randint(1, 8), max_len=rng.choice([5, 40, 140]))))
    return out


CASES = _cases()


def _cuts(name: str, data: bytes):
    rng = random.Random(len(data) * 7919 + sum(name.encode()))
    return [("whole", [max(len(data), 1)]), ("bytes", [1] * len(data) or [1]),
            ("chunks", streams.rand_chunks(rng, len(data), rng.choice(["rand", "small"])))]


@pytest.mark.parametrize("lo", range(0, len(CASES), 40))
def test_joined_pieces_are_the_message_log(lo):
    for name, data in CASES[lo:lo + 40]:
        for cut, chunks in _cuts(name, data):
            want = {impl: H.run_messages(impl, data, chunks)[0] for impl in IMPLS}
            got, j = M.run_stream(data, chunks)
            for impl in IMPLS:
                assert got == want[impl], (name, cut, impl)
            assert j.totals_ok, (name, cut)   # total = pending carried in + len, at every piece


def test_quirks_by_name():
    q = dict(streams.quirk_streams())
    log = lambda n: M.run_stream(q[n], [max(len(q[n]), 1)])[0]
    assert log("q5_control_between_fragments") == [(9, b"ABPING"), (9, b"CD")]
    assert log("q6_lone_continue") == [(8, b"orphan")]
    assert log("q7_zero_length") == [(1, b""), (2, b""), (2, b"x")]
    assert log("fragments") == [(1, b"Hello!")]
    assert log("empty") == []


def test_piece_table_of_one_batch():
    """Two segments, the first cut inside a message: a trailing open piece, then
    a fresh connection; state and first / count as the header lays them out."""
    k = b"\x01\x02\x03\x04"
    a = H.build_frames_ref([(0x31, b"one", k), (0x21, b"tw", k), (0x39, b"", k)])
    b = H.build_frames_ref([(0x10, b"o!", None)])
    out, pieces, (first, count), st = M.oracle_batch(a + b, [(0, len(a)), (len(a), len(b))], None,
                                                     M.states([M.FRESH, (2, 1, 1)]))
    assert out == b"onetwo!"
    assert [tuple(int(x) for x in p) for p in pieces] == [
        (0, 3, 3, 0, 0, 1 | M.M_END), (3, 2, 2, 2, 0, 9 | M.M_END), (5, 2, 4, 3, 1, 1 | M.M_END | M.M_CONT)]
    assert list(first) == [0, 2] and list(count) == [2, 1]
    assert [tuple(int(x) for x in s) for s in st] == [(0, 9, 0), (0, 1, 0)]
