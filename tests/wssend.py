"""Send-side oracle for hvws_send_messages and hvws_replies (include/hvws.h):
the reference's fragment plan (WebSocketChannel::send, reference
http/WebSocketChannel.cpp:24-48), hvws_frag_key, and the server's reply rule
(http/server/HttpHandler.cpp:174-200) restated on the CPU.  Expected bytes are
wsharness.build_frames_ref over the planned fragments: the reference's own
websocket_build_frame when oracle/_ref is built.

A helper, not a test module."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

FIN, MASK = 0x10, 0x20
M_END = 1 << 4
R_PONG, R_CLOSE, R_ECHO = 1, 2, 4
R_SERVER = R_PONG | R_CLOSE
RF_CLOSED, RF_DEFERRED = 1, 2
DEFAULT_FRAGMENT = 0xFFFF   # WebSocketChannel.cpp:6


def frag_key(k: int, j: int) -> int:
    """hvws_frag_key: the key of fragment j of a message with key k."""
    j &= 0xFFFFFFFF
    if j == 0:
        return k & 0xFFFFFFFF
    x = (k + j * 0x9E3779B9) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def plan(length: int, flags: int, fragment: int = 0) -> List[Tuple[int, int, int]]:
    """[(payload offset within the message, payload bytes, flags)] of one
    message: send(buf, len, fragment, opcode) of WebSocketChannel.cpp:24-48,
    and the single-frame send of lines 5-12 (which alone honours `fin`)."""
    fragment = fragment or DEFAULT_FRAGMENT
    op = flags & 0xF
    if length <= fragment:
        return [(0, length, flags & 0x1F)]            # sendFrame(buf, len, opcode, fin)
    out = [(0, fragment, op)]                         # first fragment: opcode, no FIN
    p, remain = fragment, length - fragment
    while remain > fragment:
        out.append((p, fragment, 0))                  # CONTINUE, no FIN
        p += fragment
        remain -= fragment
    out.append((p, remain, FIN))                      # last fragment: CONTINUE + FIN
    return out


def hdr_len(n: int, masked: bool) -> int:
    """websocket_calc_frame_size minus the payload (http/websocket_parser.c:189-205)."""
    return 2 + (0 if n < 126 else (2 if n <= 0xFFFF else 8)) + (4 if masked else 0)


def closed_form(length: int, fragment: int, masked: bool) -> Tuple[int, int]:
    """(frames, output bytes) of one message without walking its fragments."""
    fragment = fragment or DEFAULT_FRAGMENT
    if length <= fragment:
        return 1, hdr_len(length, masked) + length
    fr = -(-length // fragment)
    last = length - (fr - 1) * fragment
    return fr, (fr - 1) * (hdr_len(fragment, masked) + fragment) + hdr_len(last, masked) + last


def planned_frames(msgs: Sequence[Tuple[int, bytes, int]], fragment: int = 0,
                   masked: bool = False) -> List[List[Tuple[int, bytes, Optional[bytes]]]]:
    """Per message (flags, bytes, key): its frames as build_frames_ref takes them."""
    out = []
    for flags, data, key in msgs:
        frames = []
        for j, (o, n, fl) in enumerate(plan(len(data), flags, fragment)):
            k = frag_key(key, j).to_bytes(4, "little") if masked else None
            frames.append((fl | (MASK if masked else 0), data[o:o + n], k))
        out.append(frames)
    return out


def expected(msgs: Sequence[Tuple[int, bytes, int]], fragment: int = 0, masked: bool = False):
    """(output bytes, msg_off [len(msgs) + 1], frames) a send of msgs must give."""
    import wsharness as H

    out = bytearray()
    offs, nfr = [0], 0
    for frames in planned_frames(msgs, fragment, masked):
        out += H.build_frames_ref(frames)
        offs.append(len(out))
        nfr += len(frames)
    return bytes(out), offs, nfr


def reply_op(op: int, policy: int) -> int:
    """The reply opcode to a complete message with opcode `op` (0: none)."""
    if op == 9 and policy & R_PONG:
        return 10
    if op == 8 and policy & R_CLOSE:
        return 8
    if op in (1, 2) and policy & R_ECHO:
        return op
    return 0


def replies_of_messages(msgs: Sequence[Tuple[int, bytes]], policy: int, closed: bool = False):
    """The reply rule over one connection's onMessage log [(opcode, bytes)]:
    -> ([(reply flags, bytes)], closed afterwards)."""
    out = []
    for op, data in msgs:
        if closed:
            break
        r = reply_op(op, policy)
        if r:
            out.append((r | FIN, data))
        if r == 8:
            closed = True
    return out, closed


def replies_of_pieces(pieces, nseg: int, policy: int, closed_in=None):
    """The reply rule over a piece table (MSG_DTYPE, ordered by segment):
    -> (replies [(off, len, flags, key)], the piece each answers,
        (first, count) per segment, flags per segment)."""
    replies, answered = [], []
    first, count, flags = [0] * nseg, [0] * nseg, [0] * nseg
    closed = [bool(closed_in[s]) if closed_in is not None else False for s in range(nseg)]
    seen = [False] * nseg
    for s in range(nseg):
        if closed[s]:
            flags[s] |= RF_CLOSED
    cur = 0
    for p, m in enumerate(pieces):
        s = int(m["seg"])
        while cur <= s:                 # segments without pieces included
            first[cur] = len(replies)
            cur += 1
        is_first, seen[s] = not seen[s], True
        info = int(m["info"])
        r = reply_op(info & 0xF, policy) if info & M_END else 0
        if not r or closed[s]:
            continue
        if int(m["total"]) != int(m["len"]):
            assert is_first
            flags[s] |= RF_DEFERRED     # the host answers this one from its own copy
        else:
            replies.append((int(m["off"]), int(m["len"]), r | FIN, 0))
            answered.append(p)
            count[s] += 1
        if r == 8:
            closed[s] = True
            flags[s] |= RF_CLOSED
    while cur < nseg:
        first[cur] = len(replies)
        cur += 1
    return replies, answered, (first, count), flags
