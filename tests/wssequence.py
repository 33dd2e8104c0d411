"""Oracle for hvws_sequence and hvws_envelope_sequenced (include/hvws.h): the
contract in plain Python, twice.  A sequential server walks the replies with a
dict of counters and hands every publication the next number of its topic;
beside it the closed form: a stable argsort by topic and each element's rank in
its run.  The inputs are what tests/wsroute.py's route() returns for a turn
(topics and kinds per reply).  envelope_sequential() is tests/wsenvelope.py's
sequential server with the number on a publication's line, and a client's
parser for the sequenced lines stands beside it.

Counters are any mapping topic -> last number given out (a dict, a list, a
numpy array); numbers wrap at 2^64.

A helper, not a test module."""
from __future__ import annotations

import re
from typing import Dict, List, Sequence, Tuple

import numpy as np

from wsenvelope import ENV_SENDER, up16
from wsroute import RK_OTHER, RK_PUB

HDR_MAX = 45
M64 = (1 << 64) - 1

_D32 = rb"(0|[1-9][0-9]{0,9})"
_LINE = re.compile(rb"M" + _D32 + rb"(?: " + _D32 + rb")? #(0|[1-9][0-9]{0,19})\n")
_PLAIN = re.compile(rb"M" + _D32 + rb"(?: " + _D32 + rb")?\n")


def bound(out_cap: int, reply_capacity: int) -> int:
    """hvws_envelope_sequenced_bound's formula."""
    return out_cap + (HDR_MAX + 15) * reply_capacity + 16


def sequential(counters, topics: Sequence[int], kinds: Sequence[int]):
    """-> (seq per reply, {topic: counter afterwards} of the topics published to,
    totals (publications numbered, distinct topics published to))."""
    last: Dict[int, int] = {}
    seq: List[int] = []
    pubs = 0
    for t, k in zip(topics, kinds):
        if k != RK_PUB:
            seq.append(0)
            continue
        t = int(t)
        if t not in last:
            last[t] = int(counters[t])
        last[t] = (last[t] + 1) & M64
        seq.append(last[t])
        pubs += 1
    return seq, last, (pubs, len(last))


def closed_form(counters, topics: Sequence[int], kinds: Sequence[int]):
    """sequential(), without a walk: the publications sorted by topic, stable, and
    each one's position minus its run head's."""
    topics = np.asarray(topics, np.int64).reshape(-1)
    kinds = np.asarray(kinds, np.int64).reshape(-1)
    n = len(topics)
    seq = [0] * n
    idx = np.flatnonzero(kinds == RK_PUB)
    order = idx[np.argsort(topics[idx], kind="stable")]
    st = topics[order]
    pos = np.arange(len(order))
    head = np.ones(len(order), bool)
    head[1:] = st[1:] != st[:-1]
    rank = pos - np.maximum.accumulate(np.where(head, pos, 0))
    after: Dict[int, int] = {}
    for i, t, r in zip(order.tolist(), st.tolist(), rank.tolist()):
        seq[i] = (int(counters[t]) + 1 + r) & M64
        after[t] = seq[i]                      # the run's last element stands
    return seq, after, (len(order), int(head.sum()))


def line(topic: int, sender: int, seq: int, flags: int) -> bytes:
    return b"M%d %d #%d\n" % (topic, sender, seq) if flags & ENV_SENDER else b"M%d #%d\n" % (topic, seq)


def parse(msg: bytes):
    """A client's parser for hvws_envelope_sequenced's two lines: -> (topic,
    sender or None, seq, body), or None where msg does not begin with one."""
    m = _LINE.match(msg)
    if not m:
        return None
    return int(m.group(1)), (int(m.group(2)) if m.group(2) is not None else None), int(m.group(3)), msg[m.end():]


def parse_any(msg: bytes):
    """The same for a client that is served either envelope: hvws_envelope's own
    lines give seq None."""
    got = parse(msg)
    if got is not None:
        return got
    m = _PLAIN.match(msg)
    if not m:
        return None
    return int(m.group(1)), (int(m.group(2)) if m.group(2) is not None else None), None, msg[m.end():]


def reply_bytes(row, topic: int, kind: int, sender_dest: int, seq: int, out: bytes, flags: int) -> bytes:
    off, ln = int(row[0]), int(row[1])
    if kind == RK_PUB:
        return line(topic, sender_dest, seq, flags) + bytes(out[off:off + ln])
    if kind == RK_OTHER:
        return bytes(out[off:off + ln])
    return b""


def envelope_sequential(rows, topics, kinds, sender, dest_of, out: bytes, seq: Sequence[int], flags: int = 0):
    """tests/wsenvelope.py's sequential() with reply i's number seq[i] on its line:
    -> (rows' [(e, bytes, flags, key)], env bytearray of the spanned size with 0
    in the pads, placed [(offset, bytes)], totals (enveloped publications,
    verbatim replies, bytes written, bytes spanned))."""
    env = bytearray()
    rows2, placed = [], []
    pubs = verb = written = 0
    for r, t, k, s, q in zip(rows, topics, kinds, sender, seq):
        env += bytes(up16(len(env)) - len(env))
        b = reply_bytes(r, t, k, int(dest_of[s]), int(q), out, flags)
        rows2.append((len(env), len(b), int(r[2]), int(r[3])))
        if b:
            placed.append((len(env), b))
        env += b
        pubs, verb, written = pubs + (k == RK_PUB), verb + (k == RK_OTHER), written + len(b)
    env += bytes(up16(len(env)) - len(env))
    return rows2, env, placed, (pubs, verb, written, len(env))


def envelope_closed_form(rows, topics, kinds, sender, dest_of, out: bytes, seq: Sequence[int], flags: int = 0):
    """envelope_sequential()'s rows and totals from the lengths alone: h' by digit count, e by prefix sum."""
    digits = lambda v: len(str(int(v)))
    rows2, at, written = [], 0, 0
    for r, t, k, s, q in zip(rows, topics, kinds, sender, seq):
        h = 4 + digits(t) + digits(q) + ((1 + digits(dest_of[s])) if flags & ENV_SENDER else 0) if k == RK_PUB else 0
        n = h + int(r[1]) if k in (RK_PUB, RK_OTHER) else 0
        rows2.append((at, n, int(r[2]), int(r[3])))
        at, written = at + up16(n), written + n
    return rows2, (sum(k == RK_PUB for k in kinds), sum(k == RK_OTHER for k in kinds), written, at)
