"""CPU: the send-side oracle (tests/wssend.py) against the reference.  The
fragment plan's arithmetic, hvws_frag_key's known answers, the planned and
built streams fed back through the reference's own message layer, and the
server's reply rule on the quirk streams and on hand-written cases.  Also
the new entry points' exports and signatures."""
from __future__ import annotations

import random

import numpy as np
import pytest

import libhv_amd
import streams
import wsharness as H
import wsmsg
import wssend as S

FIN, MASK = S.FIN, S.MASK
IMPL = "ref" if H.have_ref() else "oracle"

FRAGS = [1, 2, 7, 125, 126, 127, 65535, 65536]


def _lens(F):
    return [0, 1, F - 1, F, F + 1, 2 * F - 1, 2 * F, 2 * F + 1]


def test_frag_key_known_answers():
    assert S.frag_key(0x12345678, 0) == 0x12345678
    assert S.frag_key(0x12345678, 1) == 0x047660EA
    assert S.frag_key(0x12345678, 2) == 0x6072B3DC
    assert S.frag_key(0, 1) == 0x92CA2F0E
    assert S.frag_key(0xFFFFFFFF, 0xFFFFFFFF) == 0x3B66B2AA


@pytest.mark.parametrize("F", FRAGS)
def test_plan_counts_and_bytes(F):
    for L in _lens(F):
        for masked in (False, True):
            for fin in (0, FIN):
                p = S.plan(L, 2 | fin, F)
                nfr, nbytes = S.closed_form(L, F, masked)
                assert len(p) == max(1, -(-L // F)) == nfr, (L, F)
                assert sum(S.hdr_len(n, masked) + n for _, n, _ in p) == nbytes, (L, F, masked)
                assert sum(n for _, n, _ in p) == L and [o for o, _, _ in p] == [j * F for j in range(len(p))]
                if len(p) == 1:
                    assert p[0][2] == 2 | fin            # the single frame keeps send()'s fin
                else:                                    # a fragmented message always ends with FIN
                    assert [fl for _, _, fl in p] == [2] + [0] * (len(p) - 2) + [FIN]
                    assert all(n == F for _, n, _ in p[:-1]) and 1 <= p[-1][1] <= F
    assert S.plan(65536, 1 | FIN, 0) == [(0, 65535, 1), (65535, 1, FIN)]   # fragment 0 = the reference's 65535


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("F", [1, 7, 126, 65535, 65536])
def test_planned_streams_parse_back_to_the_messages(F, masked):
    """Independent of the plan's own arithmetic: the reference's parser and
    message layer, fed the built frames in one chunk, deliver the messages."""
    rng = random.Random(F * 2 + masked)
    msgs = []
    for L in _lens(F):
        msgs.append((rng.choice([1, 2, 9, 10]) | FIN, rng.randbytes(L), rng.getrandbits(32)))
    data, offs, nfr = S.expected(msgs, F, masked)
    assert nfr == sum(S.closed_form(len(d), F, masked)[0] for _, d, _ in msgs)
    assert offs[-1] == len(data) == sum(S.closed_form(len(d), F, masked)[1] for _, d, _ in msgs)
    got, _, _, _ = H.run_messages(IMPL, data, [len(data)])
    assert got == [(f & 0xF, d) for f, d, _ in msgs]


def test_masked_fragments_use_frag_key():
    frames = S.planned_frames([(2 | FIN, bytes(range(20)), 0x12345678)], 7, True)[0]
    assert [k for _, _, k in frames] == [S.frag_key(0x12345678, j).to_bytes(4, "little") for j in range(3)]
    assert all(fl & MASK for fl, _, _ in frames)


def _server(msgs, policy=S.R_SERVER, closed=False):
    return S.replies_of_messages(msgs, policy, closed)


def test_reply_rule_hand_written():
    k = bytes([1, 2, 3, 4])
    B = H.build_frames_ref
    # Q5: a ping between two fragments: onMessage reports (9, "ABPING") and (9, "CD")
    data = B([(1 | MASK, b"AB", k), (9 | FIN | MASK, b"PING", k), (0 | FIN | MASK, b"CD", k)])
    msgs = H.run_messages(IMPL, data, [len(data)])[0]
    assert _server(msgs) == ([(10 | FIN, b"ABPING"), (10 | FIN, b"CD")], False)
    # a close followed by a ping: one reply, the channel is closed
    data = B([(8 | FIN | MASK, b"\x03\xe8bye", k), (9 | FIN | MASK, b"late", k)])
    msgs = H.run_messages(IMPL, data, [len(data)])[0]
    assert _server(msgs) == ([(8 | FIN, b"\x03\xe8bye")], True)
    # Q6: a lone FIN CONTINUE on a fresh connection reports 8 and closes
    data = B([(0 | FIN | MASK, b"orphan", k), (1 | FIN | MASK, b"text", k)])
    msgs = H.run_messages(IMPL, data, [len(data)])[0]
    assert msgs[0] == (8, b"orphan")
    assert _server(msgs, S.R_SERVER | S.R_ECHO) == ([(8 | FIN, b"orphan")], True)
    # echo only with the policy bit; pongs and unknown opcodes are not answered
    msgs = [(1, b"t"), (2, b"b"), (10, b"pong"), (3, b"?"), (9, b"p")]
    assert _server(msgs)[0] == [(10 | FIN, b"p")]
    assert _server(msgs, S.R_SERVER | S.R_ECHO)[0] == [(1 | FIN, b"t"), (2 | FIN, b"b"), (10 | FIN, b"p")]
    assert _server(msgs, 0) == ([], False)
    assert _server(msgs, S.R_SERVER, closed=True) == ([], True)


@pytest.mark.parametrize("policy", [S.R_SERVER, S.R_SERVER | S.R_ECHO, 0])
def test_reply_rule_on_quirk_streams(policy):
    """The rule over the piece table equals the rule over the reference's
    onMessage log, stream by stream (one fresh segment each)."""
    for name, data in streams.quirk_streams():
        if name == "q4_len_2p63":
            continue   # never completes: no message either way
        out, pieces, _, _ = wsmsg.oracle_batch(data, [(0, len(data))])
        msgs = H.run_messages(IMPL, data, [max(len(data), 1)])[0]
        want, closed = S.replies_of_messages(msgs, policy)
        rep, answered, (first, count), flags = S.replies_of_pieces(pieces, 1, policy)
        assert [(fl, out[o:o + n]) for o, n, fl, _ in rep] == want, name
        assert (first, count) == ([0], [len(want)]) and flags == [S.RF_CLOSED if closed else 0], name
        assert all(int(pieces[p]["info"]) & S.M_END for p in answered), name


def test_reply_rule_deferred_and_closed_in():
    k = bytes([9, 8, 7, 6])
    B = H.build_frames_ref
    # segment 0 completes a ping begun in an earlier batch, then a ping of its own;
    # segment 1 completes a close begun earlier, then a ping; segment 2 arrives closed
    s0 = B([(0 | FIN | MASK, b"tail", k), (9 | FIN | MASK, b"own", k)])
    s1 = B([(0 | FIN | MASK, b"bye", k), (9 | FIN | MASK, b"late", k)])
    s2 = B([(9 | FIN | MASK, b"ignored", k)])
    data = s0 + s1 + s2
    segs = [(0, len(s0)), (len(s0), len(s1)), (len(s0) + len(s1), len(s2))]
    st = wsmsg.states([(5, 9, 1), (2, 8, 1), wsmsg.FRESH])
    out, pieces, _, _ = wsmsg.oracle_batch(data, segs, None, st)
    rep, answered, (first, count), flags = S.replies_of_pieces(pieces, 3, S.R_SERVER, [0, 0, 1])
    assert [(fl, out[o:o + n]) for o, n, fl, _ in rep] == [(10 | FIN, b"own")]
    assert answered == [1] and first == [0, 1, 1] and count == [1, 0, 0]
    assert flags == [S.RF_DEFERRED, S.RF_DEFERRED | S.RF_CLOSED, S.RF_CLOSED]


def test_new_entry_points_exported_with_signatures():
    L = libhv_amd.lib()
    for name in ("hvws_send_messages", "hvws_replies", "hvws_replies_device", "hvws_reply_count_device",
                 "hvws_reply_capacity", "hvws_reply_count", "hvws_get_replies", "hvws_get_segment_replies",
                 "hvws_get_reply_flags"):
        assert hasattr(L, name), name
        assert name in libhv_amd._SIGS, name
    assert libhv_amd.TX_MSG_DTYPE.itemsize == 24
    assert (libhv_amd.R_PONG, libhv_amd.R_CLOSE, libhv_amd.R_ECHO) == (S.R_PONG, S.R_CLOSE, S.R_ECHO)
    assert np.dtype(libhv_amd.TX_MSG_DTYPE).names == ("off", "len", "flags", "key")
