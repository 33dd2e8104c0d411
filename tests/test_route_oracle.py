"""CPU: the oracle of hvws_route / hvws_fanout_routed (tests/wsroute.py) against
a second, independent statement of the command header's grammar -- a compiled
regular expression plus an integer compare -- over an exhaustive set of short
headers and random longer ones, the boundary values as literal cases, the
rule's invariants over random turns, and its equivalence with the unrouted
contract of tests/wsfan.py when every message of a connection names one topic."""
from __future__ import annotations

import itertools
import random
import re

import pytest

import wsfan as W
import wsharness as H
import wsmsg as M
import wsrfc as R
import wsroute as T
import wssend as S

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
POLICY = S.R_SERVER | S.R_ECHO
B = H.build_frames_ref

# the header as the issue states it; \Z and not $: "$" would let a final LF pass
_HEADER = re.compile(rb"\A([PSU])(0|[1-9][0-9]{0,9})\n", re.S)


def parse2(msg: bytes, ntopics: int):
    m = _HEADER.match(msg)
    if not m or int(m.group(2)) >= ntopics:
        return T.RK_BAD, T.FAN_NONE, 0
    verb, h = m.group(1), m.end()
    if verb != b"P" and len(msg) != h:
        return T.RK_BAD, T.FAN_NONE, 0
    return {b"P": T.RK_PUB, b"S": T.RK_SUB, b"U": T.RK_UNSUB}[verb], int(m.group(2)), h


ALPHABET = [b"P", b"S", b"U", b"p", b"0", b"1", b"9", b"\n", b"\r", b" "]


def test_every_header_of_up_to_four_bytes():
    n = 0
    for ln in range(5):
        for tup in itertools.product(ALPHABET, repeat=ln):
            msg = b"".join(tup)
            for nt in (0, 1, 2, 10, 100):
                assert T.parse(msg, nt) == parse2(msg, nt), (msg, nt)
            n += 1
    assert n == sum(10 ** k for k in range(5))
    # the header is at most 12 bytes whatever follows it
    assert all(T.parse(m, 1 << 32)[2] <= T.HDR_MAX for m in (b"P4294967295\n", b"P4294967295\nbody", b"P1\n" + b"x" * 40))


def test_random_longer_headers():
    rng = random.Random(5)
    kinds = set()
    for _ in range(20000):
        ln = rng.randint(5, 16)
        # mostly digits, so that long ids, eleventh digits and late LFs occur
        msg = rng.choice((b"P", b"S", b"U", b"p")) + bytes(
            rng.choice(b"0123456789") if rng.random() < 0.85 else rng.choice(b"\n\r PSU") for _ in range(ln - 1))
        if rng.random() < 0.5:
            cut = rng.randint(1, ln)
            msg = msg[:cut] + b"\n" + (msg[cut:] if rng.random() < 0.5 else b"")
        nt = rng.choice((1, 7, 1000, (1 << 32) - 1))
        got = T.parse(msg, nt)
        assert got == parse2(msg, nt), (msg, nt)
        kinds.add(got[0])
    assert kinds == {T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD}


BOUNDARY = T.BOUNDARY


@pytest.mark.parametrize("msg,nt,want", BOUNDARY)
def test_boundary_values(msg, nt, want):
    assert T.parse(msg, nt) == want == parse2(msg, nt)


def reply_table(row):
    """A turn's reply table from the RFC form's oracle: (out, replies, sender)."""
    n = len(row)
    data, segs, _, _, _ = R.Chain(n).inputs(row)
    res = R.rfc_batch(data, segs)
    rep = R.replies_of(res[1], n, POLICY)
    return res[0], rep[0], W.senders(res[1], rep[1])


def test_invariants_over_random_turns():
    rng = random.Random(99)
    seen = {k: 0 for k in (T.RK_OTHER, T.RK_PUB, T.RK_SUB, T.RK_UNSUB, T.RK_BAD, T.RK_STOPPED)}
    for _ in range(300):
        row, nt, dest_of, ndest = T.random_turn(rng)
        out, replies, sender = reply_table(row)
        rows, topics, kinds, events, flags, bad, totals = T.route(replies, sender, out, nt, dest_of)
        assert len(rows) == len(topics) == len(kinds) == len(replies)
        want_events = []
        for i, (r, q, t, k, s) in enumerate(zip(replies, rows, topics, kinds, sender)):
            seen[k] += 1
            data = r[2] & 0xF in (1, 2)
            assert (k == T.RK_OTHER) == (not data)
            # the STOPPED rule: exactly the data replies behind the segment's first BAD one
            assert (k == T.RK_STOPPED) == (data and bad[s] != T.ROUTE_NONE and i > bad[s])
            assert (k == T.RK_BAD) <= (bad[s] <= i)
            msg = out[r[0]:r[0] + r[1]]
            if k == T.RK_PUB:
                kk, tt, h = T.parse(msg, nt)
                assert kk == k and t == tt < nt and q == (r[0] + h, r[1] - h, r[2], r[3])
                assert out[q[0]:q[0] + q[1]] == msg[h:]
            else:
                assert q == tuple(r) and t == T.FAN_NONE
            if k in (T.RK_SUB, T.RK_UNSUB):
                want_events.append((T.JOIN if k == T.RK_SUB else T.LEAVE, T.parse(msg, nt)[1], dest_of[s]))
        assert events == want_events
        for s in range(len(dest_of)):
            mine = [i for i, (k, ss) in enumerate(zip(kinds, sender)) if ss == s and k == T.RK_BAD]
            assert bad[s] == (mine[0] if mine else T.ROUTE_NONE) and len(mine) <= 1
            assert flags[s] == (T.RT_BAD if mine else 0)
        assert sum(totals) == sum(1 for r in replies if r[2] & 0xF in (1, 2))
        assert totals[1] + totals[2] == len(events)
    # the generator's cases contain every kind
    assert all(v > 0 for v in seen.values()), seen


def test_equivalence_with_the_unrouted_contract():
    """Every message of segment s is P<pub[s]>\\n + body: the routed fan-out gives
    wsfan.fanout's deliveries over the bare bodies, row for row, apart from off."""
    rng = random.Random(7)
    body = lambda: bytes(rng.randrange(256) for _ in range(rng.randint(0, 20)))
    deliveries = 0
    for _ in range(150):
        nconn = rng.randint(1, 6)
        ndest = rng.randint(nconn, 30)
        dest_of = rng.sample(range(ndest), nconn)
        nt = rng.randint(1, 5)
        topics = [[rng.choice(dest_of if rng.random() < 0.5 else range(ndest)) for _ in range(rng.choice((0, 1, 2, 5, 12)))]
                  for _ in range(nt)]
        pub = [rng.randrange(nt) for _ in range(nconn)]
        flags = rng.choice((0, W.FAN_SELF))
        bare, routed = [], []
        for s in range(nconn):
            fb, fr = [], []      # the same frames; the routed ones with the header on each message's first fragment
            hdr = T.header("P", pub[s])
            for _ in range(rng.randint(0, 6)):
                k = rng.random()
                if k < 0.45:
                    op, b = rng.choice((1, 2)), body()
                    fb.append((op | FIN | MASK, b, KEY))
                    fr.append((op | FIN | MASK, hdr + b, KEY))
                elif k < 0.65:
                    op, b1, b2 = rng.choice((1, 2)), body(), body()
                    ping = [(9 | FIN | MASK, b"mid", KEY)] if rng.random() < 0.5 else []
                    fb += [(op | MASK, b1, KEY)] + ping + [(0 | FIN | MASK, b2, KEY)]
                    fr += [(op | MASK, hdr + b1, KEY)] + ping + [(0 | FIN | MASK, b2, KEY)]
                elif k < 0.85:
                    fb.append((rng.choice((9, 10)) | FIN | MASK, body(), KEY))
                    fr.append(fb[-1])
                else:
                    fb.append((8 | FIN | MASK, b"\x03\xe8", KEY))
                    fr.append(fb[-1])
            bare.append(B(fb) if fb else b"")
            routed.append(B(fr) if fr else b"")
        out0, rep0, snd0 = reply_table(bare)
        out1, rep1, snd1 = reply_table(routed)
        assert snd0 == snd1
        want = W.fanout(rep0, snd0, topics, ndest, pub, dest_of, flags)
        rows, tps, kinds, events, rflags, bad, totals = T.route(rep1, snd1, out1, nt, dest_of)
        assert not events and not any(rflags) and totals[1:] == (0, 0, 0)
        got = T.fanout_routed(rows, tps, snd1, topics, ndest, dest_of, flags)
        assert got[1:] == want[1:]
        assert [(r[1], r[2], r[3]) for r in got[0]] == [(r[1], r[2], r[3]) for r in want[0]]
        assert [out1[o:o + n] for o, n, _, _ in got[0]] == [out0[o:o + n] for o, n, _, _ in want[0]]
        deliveries += len(got[0])
    assert deliveries > 1000
