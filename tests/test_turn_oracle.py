"""CPU: the merged event array of hvws_subs_update_routed (tests/wsturn.py
`merged`) run through hvws_subs_update's sequential rule (tests/wssubs.py)
against a sequential pub/sub server (tests/wsturn.py `Server`) that never sees
an event array: random turns of tests/wsroute.py with the host events of
tests/wssubs.py and random write limits, and the cases the contract names."""
from __future__ import annotations

import random

import wsbudget as G
import wsfan as W
import wsharness as H
import wsmsg as M
import wsrfc as R
import wsroute as T
import wssend as S
import wssubs as U
import wsturn as N

FIN, MASK = M.FIN, M.MASK
KEY = bytes([0x37, 0xFA, 0x21, 0x3D])
POLICY = S.R_SERVER | S.R_ECHO
B = H.build_frames_ref
CLOSE = (8 | FIN | MASK, b"\x03\xe8", KEY)


def text(body: bytes):
    return (1 | FIN | MASK, body, KEY)


def routed(row, topics, ntopics, ndest, dest_of, fan_flags=0):
    """The turn through the oracles of the passes: (output bytes, reply flags, the
    route's result, the routed fan-out's)."""
    n = len(row)
    data, segs, _, _, _ = R.Chain(n).inputs(row)
    res = R.rfc_batch(data, segs)
    rep = R.replies_of(res[1], n, POLICY)
    sender = W.senders(res[1], rep[1])
    r = T.route(rep[0], sender, res[0], ntopics, dest_of)
    return res[0], rep[3], r, T.fanout_routed(r[0], r[1], sender, topics, ndest, dest_of, fan_flags)


def both(row, topics, ntopics, ndest, dest_of, host=(), budgets=None, flags=0, fan_flags=0):
    """-> (the table of the merged events, the server's table, the merged events,
    the server's writes per destination, the budget oracle's)."""
    out, rflags, r, fan = routed(row, topics, ntopics, ndest, dest_of, fan_flags)
    cut = G.budget(fan, budgets)
    ev, rtflags, over = r[3], r[4], cut[5]
    sent = {}
    for d in range(ndest):
        rows = cut[0][cut[2][d]:cut[2][d] + cut[3][d]]
        if rows:
            sent[d] = [(fl & 0xF, out[o:o + ln]) for o, ln, fl, _ in rows]
    m = N.merged(ev, rflags, rtflags, dest_of, over, host, flags)
    nd = sum(1 for s in range(len(dest_of)) if rflags[s] & 1 or rtflags[s] & 1)
    no = sum(1 for f in over if f) if flags & N.OVER else 0
    assert N.parts(ev, rflags, rtflags, dest_of, over, host, flags) == (len(ev), nd, no, len(host))
    assert len(m) == len(ev) + nd + no + len(host)
    srv = N.Server(ntopics, topics, bool(flags & N.UNIQUE), bool(fan_flags & W.FAN_SELF))
    box, closed = srv.turn([(dest_of[c], N.messages_of_read(row[c])) for c in range(len(row))], host,
                           budgets if flags & N.OVER else None)
    if flags & N.OVER:
        assert closed == [d for d, f in enumerate(over) if f]
    return U.sequential(topics, (), m, flags & N.UNIQUE), srv.rows(), m, box, sent


def test_random_turns_against_the_sequential_server():
    rng = random.Random(415)
    seen = {"closed": 0, "bad": 0, "over": 0, "rejoin": 0, "writes": 0}
    for k in range(3000):
        row, nt, dest_of, ndest = T.random_turn(rng)
        pool = sorted(set(dest_of))
        topics = [[rng.choice(pool) if rng.random() < 0.7 else rng.randrange(ndest) for _ in range(rng.choice((0, 1, 2, 5)))]
                  for _ in range(nt)]
        host = U.random_events(rng, nt, ndest, pool, rng.choice((0, 0, 1, 3, 8)))
        flags = rng.choice((0, N.UNIQUE, N.OVER, N.UNIQUE | N.OVER))
        fan_flags = rng.choice((0, W.FAN_SELF))
        budgets = None
        if flags & N.OVER:
            budgets = G.random_budgets(rng, routed(row, topics, nt, ndest, dest_of, fan_flags)[3])
        got, want, m, box, sent = both(row, topics, nt, ndest, dest_of, host, budgets, flags, fan_flags)
        assert got == want, (k, row, topics, host, flags)
        drops = [e for e in m[:len(m) - len(host)] if e[0] == N.DROP]
        seen["closed"] += bool(drops)
        seen["bad"] += any(op in (1, 2) and T.parse(b, nt)[0] == T.RK_BAD for c in row for op, b in N.messages_of_read(c))
        seen["over"] += bool(flags & N.OVER and any(b < G.UNLIMITED for b in budgets) and len(drops) > sum(
            1 for e in drops if e[2] in dest_of))
        seen["rejoin"] += any(e[0] == N.JOIN and any(d[2] == e[2] for d in drops) for e in host)
        # the writes too, where the reply table's order is the stream's: no control frame but a CLOSE
        if all(op in (1, 2, 8) for c in row for op, _ in N.messages_of_read(c)):
            seen["writes"] += 1
            assert box == sent, (k, row, topics)
    assert all(v > 50 for v in seen.values()), seen


def test_random_cases_of_the_update_oracle_as_host_events():
    """wssubs.random_case: unrouted traffic (every data message is malformed or a
    stray), so the turn is its connection drops and the host's events."""
    rng = random.Random(9)
    for k in range(1500):
        reads, topics, ndest, _, dest_of, _, events, flags = U.random_case(rng)
        nt = len(topics)
        # the plain oracle parses what the frames hold; a read with a stray continuation is not a turn of messages
        try:
            msgs = [N.messages_of_read(r) for r in reads]
        except (TypeError, AssertionError):
            continue
        _, rflags, r, _ = routed(reads, topics, nt, ndest, dest_of)
        m = N.merged(r[3], rflags, r[4], dest_of, None, events, flags)
        srv = N.Server(nt, topics, bool(flags & N.UNIQUE))
        srv.turn(list(zip(dest_of, msgs)), events)
        assert U.sequential(topics, (), m, flags) == srv.rows(), (k, reads, topics, events)


# ---- the cases the contract names ------------------------------------------------------------------

def test_join_then_close_in_one_read_ends_up_unlisted():
    row = [B([text(b"S1\n"), CLOSE]), B([text(b"S1\n")])]
    got, want, m, _, _ = both(row, [[], [9]], 2, 10, [4, 5])
    assert m == [(N.JOIN, 1, 4), (N.JOIN, 1, 5), (N.DROP, 0, 4)]
    assert got == want == [[], [9, 5]]
    # what the hand-made flow gives without a DROP behind the route's events: listed for good
    assert U.sequential([[], [9]], [4], m[:2]) == [[], [9, 4, 5]]


def test_a_bad_connections_earlier_subscribe_is_annulled():
    row = [B([text(b"S0\n"), text(b"junk"), text(b"S1\n")]), B([text(b"U1\n")])]
    got, want, m, _, _ = both(row, [[7], [4, 5]], 2, 10, [4, 5])
    assert m == [(N.JOIN, 0, 4), (N.LEAVE, 1, 5), (N.DROP, 0, 4)]
    assert got == want == [[7], []]


def test_a_host_join_of_a_dropped_id_stands():
    row = [B([text(b"S0\n"), CLOSE])]
    got, want, m, _, _ = both(row, [[4, 7], [4]], 2, 10, [4], host=[(N.JOIN, 1, 4)])
    assert m[-2:] == [(N.DROP, 0, 4), (N.JOIN, 1, 4)]
    assert got == want == [[7], [4]]


def test_an_over_destinations_own_subscribe_is_annulled():
    row = [B([text(b"P0\n" + b"x" * 100)]), B([text(b"S1\n")])]
    budgets = [1 << 40] * 10
    budgets[5] = 50
    got, want, m, box, sent = both(row, [[5], []], 2, 10, [4, 5], budgets=budgets, flags=N.OVER)
    assert m == [(N.JOIN, 1, 5), (N.DROP, 0, 5)]
    assert got == want == [[], []] and box == sent == {}
    # without HVWS_SUBS_OVER the budget's verdict is the host's to pass on
    assert both(row, [[5], []], 2, 10, [4, 5], budgets=budgets)[0] == [[5], [5]]


def test_unique_with_a_join_of_an_id_listed_before_and_dropped_in_the_same_turn():
    row = [B([text(b"S0\n"), CLOSE]), B([text(b"S0\n"), text(b"S0\n")])]
    got, want, m, _, _ = both(row, [[4, 5, 6]], 1, 10, [4, 5], host=[(N.JOIN, 0, 4), (N.JOIN, 0, 4)], flags=N.UNIQUE)
    assert m == [(N.JOIN, 0, 4), (N.JOIN, 0, 5), (N.JOIN, 0, 5), (N.DROP, 0, 4), (N.JOIN, 0, 4), (N.JOIN, 0, 4)]
    # 5 was listed and stays once; 4's old listing and its JOIN die with the DROP, the host's first JOIN stands
    assert got == want == [[5, 6, 4]]
