"""Oracle for hvws_envelope (include/hvws.h): the contract in plain Python,
twice.  A sequential server walks the replies and appends each one's bytes --
a publication's as b"M%d %d\\n" % (topic, sender) + body -- to a bytearray at
the next multiple of 16; beside it the closed form: lengths, a cumulative sum of
the lengths rounded up to 16, one placement.  The inputs are what
tests/wsroute.py's route() returns for a turn (the routed rows, topics and
kinds) with the segment that sent each reply.  A client's parser for the
envelope line stands beside them.

d_env is modelled sparsely: `placed` lists (offset, bytes) per reply that wrote
some; bytes between them (the pads) and behind the spanned size belong to the
caller.

A helper, not a test module."""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

from wsroute import RK_OTHER, RK_PUB

ENV_SENDER = 1
HDR_MAX = 23
NO_SENDER = (1 << 32) - 1

_LINE = re.compile(rb"M(0|[1-9][0-9]{0,9})(?: (0|[1-9][0-9]{0,9}))?\n")


def up16(n: int) -> int:
    return (n + 15) // 16 * 16


def bound(out_cap: int, reply_capacity: int) -> int:
    """hvws_envelope_bound's formula."""
    return out_cap + (HDR_MAX + 15) * reply_capacity + 16


def line(topic: int, sender: int, flags: int) -> bytes:
    return b"M%d %d\n" % (topic, sender) if flags & ENV_SENDER else b"M%d\n" % topic


def parse(msg: bytes):
    """A client's parser: -> (topic, sender or None, body), or None where msg does not begin with an envelope line."""
    m = _LINE.match(msg)
    if not m:
        return None
    return int(m.group(1)), (int(m.group(2)) if m.group(2) is not None else None), msg[m.end():]


def reply_bytes(row, topic: int, kind: int, sender_dest: int, out: bytes, flags: int) -> bytes:
    off, ln = int(row[0]), int(row[1])
    if kind == RK_PUB:
        return line(topic, sender_dest, flags) + bytes(out[off:off + ln])
    if kind == RK_OTHER:
        return bytes(out[off:off + ln])
    return b""


def sequential(rows, topics: Sequence[int], kinds: Sequence[int], sender: Sequence[int], dest_of: Sequence[int],
               out: bytes, flags: int = 0):
    """-> (rows' [(e, bytes, flags, key)], env bytearray of the spanned size with
    0 in the pads, placed [(offset, bytes)], totals (enveloped publications,
    verbatim replies, bytes written, bytes spanned))."""
    env = bytearray()
    rows2, placed = [], []
    pubs = verb = written = 0
    for r, t, k, s in zip(rows, topics, kinds, sender):
        env += bytes(up16(len(env)) - len(env))        # the next multiple of 16
        b = reply_bytes(r, t, k, int(dest_of[s]), out, flags)
        rows2.append((len(env), len(b), int(r[2]), int(r[3])))
        if b:
            placed.append((len(env), b))
        env += b
        pubs, verb, written = pubs + (k == RK_PUB), verb + (k == RK_OTHER), written + len(b)
    env += bytes(up16(len(env)) - len(env))
    return rows2, env, placed, (pubs, verb, written, len(env))


def closed_form(rows, topics, kinds, sender, dest_of, out: bytes, flags: int = 0):
    """sequential(), from the lengths alone: h' by digit count, e by prefix sum."""
    digits = lambda v: len(str(v))
    lens = []
    for r, t, k, s in zip(rows, topics, kinds, sender):
        h = (2 + digits(t) + ((1 + digits(int(dest_of[s]))) if flags & ENV_SENDER else 0)) if k == RK_PUB else 0
        lens.append(h + int(r[1]) if k in (RK_PUB, RK_OTHER) else 0)
    e, at = [], 0
    for n in lens:
        e.append(at)
        at += up16(n)
    env = bytearray(at)
    placed = []
    for r, t, k, s, n, a in zip(rows, topics, kinds, sender, lens, e):
        if n:
            b = reply_bytes(r, t, k, int(dest_of[s]), out, flags)
            assert len(b) == n
            env[a:a + n] = b
            placed.append((a, b))
    rows2 = [(a, n, int(r[2]), int(r[3])) for r, n, a in zip(rows, lens, e)]
    totals = (sum(k == RK_PUB for k in kinds), sum(k == RK_OTHER for k in kinds), sum(lens), at)
    return rows2, env, placed, totals


def retain_rows(rows2, routed_rows, kinds) -> List[Tuple[int, int, int, int]]:
    """The rows hvws_retain_enveloped's rule reads: R', with length 0 where a
    publication's body is empty ("empty" means an empty body)."""
    return [(e, 0 if k == RK_PUB and int(r[1]) == 0 else n, fl, key)
            for (e, n, fl, key), r, k in zip(rows2, routed_rows, kinds)]
