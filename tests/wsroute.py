"""Oracle for hvws_route and hvws_fanout_routed (include/hvws.h): the contract
in plain Python -- the command header's grammar, the rule over a reply table
(kinds, trimmed rows, topic per reply, the STOPPED rule, the dense event list,
per-segment flags, totals) and the fan-out with the topic per reply.  Reply
tables are those tests/wsfan.py takes: replies [(off, len, flags, key)] and the
segment that sent each.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Sequence, Tuple

from wsfan import FAN_NONE, FAN_SELF, destination_frames, flatten  # noqa: F401  (re-exported)

HDR_MAX = 12
RK_OTHER, RK_PUB, RK_SUB, RK_UNSUB, RK_BAD, RK_STOPPED = 0, 1, 2, 3, 4, 5
RT_BAD = 1
ROUTE_NONE = (1 << 64) - 1
JOIN, LEAVE = 1, 2

_VERB = {0x50: RK_PUB, 0x53: RK_SUB, 0x55: RK_UNSUB}


def parse(msg: bytes, ntopics: int) -> Tuple[int, int, int]:
    """-> (kind, topic, h): RK_PUB / RK_SUB / RK_UNSUB with the topic id and the
    header length, or (RK_BAD, FAN_NONE, 0)."""
    bad = (RK_BAD, FAN_NONE, 0)
    head = msg[:HDR_MAX]                   # the LF must lie within the first 12 bytes, and in the message
    if not head or head[0] not in _VERB:
        return bad
    lf = head.find(b"\n")
    if lf < 0:
        return bad
    digits = head[1:lf]
    if not digits or len(digits) > 10 or any(not 0x30 <= c <= 0x39 for c in digits):
        return bad
    if len(digits) > 1 and digits[0] == 0x30:
        return bad
    topic = int(digits)
    if topic >= ntopics:
        return bad
    kind, h = _VERB[head[0]], lf + 1
    if kind != RK_PUB and len(msg) != h:
        return bad
    return kind, topic, h


def route(replies, sender: Sequence[int], out: bytes, ntopics: int, dest_of: Sequence[int]):
    """-> (rows [(off, len, flags, key)], topics, kinds, events [(op, topic,
    dest)], flags [nseg], bad_reply [nseg], totals (publications, subscribes,
    unsubscribes, bad + stopped))."""
    nseg = len(dest_of)
    rows, topics, kinds, events = [], [], [], []
    bad_reply = [ROUTE_NONE] * nseg
    for i, (r, s) in enumerate(zip(replies, sender)):
        off, ln, fl, key = (int(x) for x in r)
        kind, topic = RK_OTHER, FAN_NONE
        if fl & 0xF in (1, 2):
            if bad_reply[s] != ROUTE_NONE:
                kind = RK_STOPPED
            else:
                kind, t, h = parse(bytes(out[off:off + ln]), ntopics)
                if kind == RK_PUB:
                    off, ln, topic = off + h, ln - h, t
                elif kind == RK_SUB:
                    events.append((JOIN, t, int(dest_of[s])))
                elif kind == RK_UNSUB:
                    events.append((LEAVE, t, int(dest_of[s])))
                else:
                    bad_reply[s] = i
        rows.append((off, ln, fl, key))
        topics.append(topic)
        kinds.append(kind)
    flags = [RT_BAD if b != ROUTE_NONE else 0 for b in bad_reply]
    totals = (kinds.count(RK_PUB), kinds.count(RK_SUB), kinds.count(RK_UNSUB),
              kinds.count(RK_BAD) + kinds.count(RK_STOPPED))
    return rows, topics, kinds, events, flags, bad_reply, totals


def edges(rows, topics: Sequence[int], sender: Sequence[int], subs: Sequence[Sequence[int]],
          dest_of: Sequence[int], flags: int = 0) -> List[Tuple[int, int, int, int]]:
    """[(destination, opcode == 8, reply i, listing j)] in (i, j) order."""
    out = []
    for i, (r, t, s) in enumerate(zip(rows, topics, sender)):
        op = r[2] & 0xF
        if op in (1, 2):
            if t == FAN_NONE:          # SUB, UNSUB, BAD, STOPPED
                continue
            for j, d in enumerate(subs[t]):
                if d == dest_of[s] and not flags & FAN_SELF:
                    continue
                out.append((int(d), 0, i, j))
        else:
            out.append((int(dest_of[s]), 1 if op == 8 else 0, i, 0))
    return out


def fanout_routed(rows, topics: Sequence[int], sender: Sequence[int], subs: Sequence[Sequence[int]], ndest: int,
                  dest_of: Sequence[int], flags: int = 0):
    """-> (deliveries [(off, len, flags, key)], reply of each delivery, first
    [ndest], count [ndest]): wsfan.fanout with the topic per reply and the
    routed rows."""
    es = sorted(edges(rows, topics, sender, subs, dest_of, flags))
    table = [tuple(int(x) for x in rows[i]) for _, _, i, _ in es]
    reply = [i for _, _, i, _ in es]
    count = [0] * ndest
    for d, _, _, _ in es:
        count[d] += 1
    first, at = [0] * ndest, 0
    for d in range(ndest):
        first[d] = at
        at += count[d]
    return table, reply, first, count


NT = (1 << 32) - 1
BAD = (RK_BAD, FAN_NONE, 0)
# The boundary values as literal cases, (message, ntopics, expected parse): tests/test_route_oracle.py holds the
# oracle to them, tests/test_gpu_route.py the device.
BOUNDARY = [
    (b"P0\n", NT, (RK_PUB, 0, 3)),
    (b"S4294967294\n", NT, (RK_SUB, NT - 1, 12)),              # ntopics - 1
    (b"P4294967295\n", NT, BAD),                                  # ntopics
    (b"U4294967294\n", NT, (RK_UNSUB, 4294967294, 12)),
    (b"P4294967295\nx", NT, BAD),
    (b"P4294967296\n", NT, BAD),                                  # past 2^32: compared in 64 bits
    (b"P9999999999\n", NT, BAD),
    (b"P00\n", NT, BAD),
    (b"P01\n", NT, BAD),
    (b"P12345678901\n", NT, BAD),                                 # an eleventh digit
    (b"P1234567890\nbody", NT, (RK_PUB, 1234567890, 12)),       # the LF at byte 12
    (b"P12345678901\nbody", NT, BAD),                             # ... and at byte 13
    (b"S3\nx", NT, BAD),
    (b"S3\n", NT, (RK_SUB, 3, 3)),
    (b"P3\n", NT, (RK_PUB, 3, 3)),                              # an empty body
    (b"", NT, BAD),
    (b"P1\r\n", NT, BAD),
    (b"p1\n", NT, BAD),
    (b"P\n", NT, BAD),
    (b"P1", NT, BAD),
    (b"P7\n", 7, BAD),
    (b"P6\n", 7, (RK_PUB, 6, 3)),
]


def header(verb: str, topic: int) -> bytes:
    return b"%s%d\n" % (verb.encode(), topic)


def random_message(rng, ntopics: int) -> bytes:
    """A message of a random kind: a publication with a body of 0 .. 20 bytes, a
    subscribe, an unsubscribe, or one of the malformed shapes."""
    body = bytes(rng.randrange(256) for _ in range(rng.randint(0, 20)))
    k = rng.random()
    t = rng.randrange(ntopics) if ntopics else 0
    if k < 0.5:
        return header("P", t) + body
    if k < 0.65:
        return header("S", t)
    if k < 0.8:
        return header("U", t)
    return rng.choice([b"", b"p1\n", b"P\n", b"P01\n", b"P%d\n" % ntopics, b"P1\r\n", b"S1\nx", b"X1\n", b"P12345678901\n",
                       b"P1", b"U", body])


def random_turn(rng, max_conn: int = 6, ntopics: int = 5):
    """(reads [one bytes per connection], ntopics, dest_of, ndest): connections
    sending a few routed messages (mostly well-formed), PINGs and now and then a
    CLOSE."""
    import wsharness as H

    FIN, MASK = 0x10, 0x20
    key = lambda: bytes(rng.randrange(256) for _ in range(4))
    nconn = rng.randint(1, max_conn)
    ndest = rng.randint(nconn, 3 * max_conn)
    dest_of = rng.sample(range(ndest), nconn)
    reads = []
    for _ in range(nconn):
        frames = []
        for _ in range(rng.randint(0, 6)):
            k = rng.random()
            if k < 0.8:
                frames.append((rng.choice((1, 2)) | FIN | MASK, random_message(rng, ntopics), key()))
            elif k < 0.93:
                frames.append((9 | FIN | MASK, b"ping", key()))
            else:
                frames.append((8 | FIN | MASK, b"\x03\xe8", key()))
        reads.append(H.build_frames_ref(frames) if frames else b"")
    return reads, ntopics, dest_of, ndest
