"""CPU: the two forms of hvws_envelope's contract in tests/wsenvelope.py agree --
the sequential server and the closed form over lengths and a prefix sum -- on
random turns routed by tests/wsroute.py's oracle; every envelope parses back to
its topic and sender with the client's parser and what follows is the body; the
capacity formula holds on every turn.  The generator counts the cases the
contract names and the test asserts each occurred, so that random inputs cannot
hide one."""
from __future__ import annotations

import collections
import random

import wsenvelope as E
import wsroute as T

FIN = 0x10
NT = (1 << 32) - 1
TOPICS = (0, 0, 7, 9, 10, 42, 99999, 1234567890, 4294967294)     # 1 .. 10 digits
DESTS = (0, 9, 10, 123, 99999, 2147483646)                       # ndest <= 2^31 - 1


def message(rng) -> bytes:
    k = rng.random()
    t = rng.choice(TOPICS)
    if k < 0.6:
        n = rng.choice((0, 0, 1, 2, 5, 11, 12, 13, 14, 15, 16, 17, 28, 29, 30, rng.randint(0, 40)))
        return T.header("P", t) + bytes(rng.randrange(256) for _ in range(n))
    if k < 0.75:
        return T.header(rng.choice("SU"), t)
    if k < 0.9:
        return T.random_message(rng, 5)
    return rng.choice([b"", b"P01\n", b"X1\n", b"P1", b"P4294967295\n"])


def turn(rng, max_conn: int = 5):
    """(replies, sender, out, dest_of, reply capacity): connections each sending a
    few routed messages, a PONG or a CLOSE now and then, their bytes laid out as
    a message call leaves them (gaps between messages, replies ordered by segment)."""
    nconn = rng.randint(1, max_conn)
    dest_of = rng.sample(DESTS, nconn)
    out, replies, sender = bytearray(), [], []
    for s in range(nconn):
        for _ in range(rng.randint(0, 6)):
            out += bytes(rng.randrange(256) for _ in range(rng.randint(0, 3)))
            k = rng.random()
            if k < 0.08:
                msg, fl = bytes(rng.randrange(256) for _ in range(rng.choice((0, 4, 16, 17, 125)))), 10 | FIN
            elif k < 0.12:
                msg, fl = b"\x03\xe8" + b"bye" * rng.randint(0, 5), 8 | FIN
            else:
                msg, fl = message(rng), rng.choice((1, 2)) | FIN
            replies.append((len(out), len(msg), fl, rng.randrange(1 << 32)))
            sender.append(s)
            out += msg
    return replies, sender, bytes(out), dest_of, len(replies) + rng.randint(0, 3)


CASES = ("empty body", "topic 0", "1-digit topic", "10-digit topic", "1-digit sender", "10-digit sender", "sender on",
         "sender off", "PONG verbatim", "CLOSE verbatim", "BAD", "STOPPED", "16k bytes", "16k+1 bytes", "16k-1 bytes",
         "SUB or UNSUB", "header of 3", "header of 23")


def test_the_two_forms_agree_on_3000_random_turns():
    rng = random.Random(417)
    seen = collections.Counter()
    for n in range(3000):
        replies, sender, out, dest_of, cap = turn(rng)
        rows, topics, kinds = T.route(replies, sender, out, NT, dest_of)[:3]
        flags = n & 1
        got = E.sequential(rows, topics, kinds, sender, dest_of, out, flags)
        assert got == E.closed_form(rows, topics, kinds, sender, dest_of, out, flags)
        rows2, env, placed, totals = got
        seen["sender on" if flags else "sender off"] += 1
        at = 0
        for i, ((e, ln, fl, key), r, t, k, s) in enumerate(zip(rows2, rows, topics, kinds, sender)):
            assert e == at and e % 16 == 0 and (fl, key) == (r[2], r[3])
            at += E.up16(ln)
            got_bytes = bytes(env[e:e + ln])
            body = out[r[0]:r[0] + r[1]]
            assert not any(env[e + ln:at])                       # the pad is nobody's
            if k == T.RK_PUB:
                d = dest_of[s]
                assert E.parse(got_bytes) == (t, d if flags else None, body)
                h = ln - len(body)
                assert 3 <= h <= E.HDR_MAX
                seen["empty body"] += not body
                seen["topic 0"] += t == 0
                seen["1-digit topic"] += t < 10
                seen["10-digit topic"] += t >= 10 ** 9
                seen["1-digit sender"] += bool(flags) and d < 10
                seen["10-digit sender"] += bool(flags) and d >= 10 ** 9
                seen["header of 3"] += h == 3
                seen["header of 23"] += h == 23
            elif k == T.RK_OTHER:
                assert got_bytes == body
                seen["PONG verbatim"] += r[2] & 0xF == 10 and ln > 0
                seen["CLOSE verbatim"] += r[2] & 0xF == 8
            else:
                assert ln == 0
                seen["BAD"] += k == T.RK_BAD
                seen["STOPPED"] += k == T.RK_STOPPED
                seen["SUB or UNSUB"] += k in (T.RK_SUB, T.RK_UNSUB)
            if ln:
                seen["16k bytes"] += ln % 16 == 0
                seen["16k+1 bytes"] += ln % 16 == 1
                seen["16k-1 bytes"] += ln % 16 == 15
        assert totals == (kinds.count(T.RK_PUB), kinds.count(T.RK_OTHER), sum(r[1] for r in rows2), at) and at == len(env)
        assert [(a, b) for a, b in placed] == [(e, bytes(env[e:e + ln])) for e, ln, _, _ in rows2 if ln]
        # the capacity: replies answer disjoint pieces of out
        assert at <= E.bound(len(out), cap)
        assert sum(r[1] for r in replies) <= len(out)
    for c in CASES:
        assert seen[c] > 0, c


def test_the_client_parser_is_the_grammar():
    assert E.parse(b"M0\n") == (0, None, b"")
    assert E.parse(b"M7 12\nbody\n") == (7, 12, b"body\n")
    assert E.parse(b"M4294967294 2147483646\n") == (4294967294, 2147483646, b"")
    assert len(E.line(4294967294, 2147483646, E.ENV_SENDER)) == E.HDR_MAX == 23
    assert E.line(3, 5, 0) == b"M3\n" and E.line(3, 5, 1) == b"M3 5\n"
    for bad in (b"", b"M\n", b"M01\n", b"M1 \n", b"M1 02\n", b"m1\n", b"M1", b"M12345678901\n", b"M1  2\n", b"P1\n"):
        assert E.parse(bad) is None, bad


def test_the_retain_rows_call_an_empty_body_empty():
    out = b"P3\nP4\nx"
    rows, topics, kinds = T.route([(0, 3, 1 | FIN, 0), (3, 4, 1 | FIN, 0)], [0, 0], out, 9, [6])[:3]
    rows2 = E.sequential(rows, topics, kinds, [0, 0], [6], out, E.ENV_SENDER)[0]
    assert rows2 == [(0, 5, 1 | FIN, 0), (16, 6, 1 | FIN, 0)]
    assert E.retain_rows(rows2, rows, kinds) == [(0, 0, 1 | FIN, 0), (16, 6, 1 | FIN, 0)]


def test_the_constants_are_the_binding_s():
    import libhv_amd

    assert libhv_amd.ENV_SENDER == E.ENV_SENDER == 1 and libhv_amd.ENV_HDR_MAX == E.HDR_MAX == 23
    for m in ("envelope_bound", "envelope", "envelope_table", "envelope_totals", "fanout_enveloped", "retain_enveloped"):
        assert callable(getattr(libhv_amd.Engine, m))
