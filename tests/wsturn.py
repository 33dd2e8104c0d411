"""Oracle for hvws_subs_update_routed (include/hvws.h): the merged event array
in plain Python (`merged`), and a sequential pub/sub server (`Server`) that
keeps a dict of room -> list and handles a turn connection by connection and
message by message, as a service written against the reference's onmessage
would.  tests/test_turn_oracle.py holds the two against each other: the table
tests/wssubs.py `sequential` gives for the merged events is the server's.

The server is written from the contract's prose, not from wssubs.closed_form:
  - a message is a command header (verb, decimal room, LF) and, for 'P', a body;
  - 'S' lists the sender in the room (under UNIQUE only if it is not listed at
    that moment), 'U' removes every listing of it from the room, 'P' goes to the
    room as it stood when the turn began: a subscription takes effect in the
    next turn;
  - a malformed message, a CLOSE or a protocol failure closes the connection:
    nothing it sent behind that point counts, and it leaves every room (behind
    a malformed message its PINGs and its CLOSE are still answered: they are
    the reply rule's business);
  - a destination whose writes go over its limit is closed: the write that does
    not fit and everything behind it are not sent, and it leaves every room.
    What its own connection sent in this read was taken already and still goes
    out, but its subscriptions of this turn go with it;
  - the service's own events apply last, so the JOIN of a new connection that
    took a closed id over stands.

A helper, not a test module."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import wsbudget as G
import wsroute as T

JOIN, LEAVE, DROP = 1, 2, 3
UNIQUE, OVER = 1, 2
RF_CLOSED, RT_BAD, BF_OVER = 1, 1, 1
FAIL = -1   # a pseudo opcode in a connection's messages: the protocol check failed it here


def merged(route_events, reply_flags: Sequence[int], route_flags: Sequence[int], dest_of: Sequence[int],
           over_flags: Optional[Sequence[int]], host_events, flags: int = 0) -> List[Tuple[int, int, int]]:
    """The array M of hvws_subs_update_routed: the route's events, a DROP per
    closed or malformed segment, with OVER a DROP per destination over its
    budget, the host's events."""
    m = [tuple(int(x) for x in e) for e in route_events]
    m += [(DROP, 0, int(dest_of[s])) for s in range(len(dest_of)) if reply_flags[s] & RF_CLOSED or route_flags[s] & RT_BAD]
    if flags & OVER:
        m += [(DROP, 0, d) for d, f in enumerate(over_flags) if f & BF_OVER]
    return m + [tuple(int(x) for x in e) for e in host_events]


def parts(route_events, reply_flags, route_flags, dest_of, over_flags, host_events, flags: int = 0):
    """hvws_get_subs_merged: (route events, connection drops, OVER drops, host events)."""
    a = len(merged(route_events, reply_flags, route_flags, dest_of, None, (), 0)) - len(route_events)
    b = sum(1 for f in over_flags if f & BF_OVER) if flags & OVER else 0
    return len(route_events), a, b, len(host_events)


def messages_of_read(read: bytes) -> List[Tuple[int, bytes]]:
    """The whole messages of one read of complete client frames, in stream order:
    [(opcode, payload)], control frames where they stand."""
    out, at, cur = [], 0, None
    while at < len(read):
        b0, b1 = read[at], read[at + 1]
        n, at = b1 & 0x7F, at + 2
        if n == 126:
            n, at = int.from_bytes(read[at:at + 2], "big"), at + 2
        elif n == 127:
            n, at = int.from_bytes(read[at:at + 8], "big"), at + 8
        key = b"\0\0\0\0"
        if b1 & 0x80:
            key, at = read[at:at + 4], at + 4
        body = bytes(c ^ key[i & 3] for i, c in enumerate(read[at:at + n]))
        at += n
        op, fin = b0 & 0xF, b0 & 0x80
        if op >= 8:
            out.append((op, body))
        else:
            cur = (op, body) if op else (cur[0], cur[1] + body)
            if fin:
                out.append(cur)
                cur = None
    assert cur is None and at == len(read)
    return out


class Server:
    """rooms: {room: [[destination, joined]]}; joined is None for a listing that
    stood when the turn began, else the order of its join within the turn."""

    def __init__(self, ntopics: int, topics: Optional[Sequence[Sequence[int]]] = None, unique: bool = False,
                 self_too: bool = False):
        self.ntopics, self.unique, self.self_too = ntopics, unique, self_too
        self.rooms: Dict[int, list] = {t: [[int(d), None] for d in (topics[t] if topics else [])] for t in range(ntopics)}
        self.joins = 0

    def rows(self) -> List[List[int]]:
        """The rooms in the table's order: the listings that stood before in their
        order, then the joined ones by destination, then by join."""
        out = []
        for t in range(self.ntopics):
            old = [d for d, j in self.rooms[t] if j is None]
            new = sorted((d, j) for d, j in self.rooms[t] if j is not None)
            out.append(old + [d for d, _ in new])
        return out

    def _join(self, t: int, d: int) -> None:
        if not self.unique or all(x != d for x, _ in self.rooms[t]):
            self.rooms[t].append([d, self.joins])
            self.joins += 1

    def _leave(self, t: int, d: int) -> None:
        self.rooms[t] = [e for e in self.rooms[t] if e[0] != d]

    def _close(self, d: int) -> None:
        for t in self.rooms:
            self._leave(t, d)

    def turn(self, conns: Sequence[Tuple[int, Sequence[Tuple[int, bytes]]]], host_events=(),
             budgets: Optional[Sequence[int]] = None, fragment: int = 0, masked: bool = False):
        """conns: [(destination id, [(opcode, payload)])] -> ({destination: [(opcode,
        body)] written to it, in order}, the destinations closed as over the limit)."""
        self.rooms = {t: [[d, None] for d in row] for t, row in enumerate(self.rows())}
        before = {t: [d for d, _ in row] for t, row in self.rooms.items()}
        box: Dict[int, list] = {}
        queued: Dict[int, int] = {}
        over = set()

        def write(d: int, op: int, body: bytes) -> None:
            if d in over:
                return
            n = G.wire(len(body), fragment, masked)
            if budgets is not None and queued.get(d, 0) + n > budgets[d]:
                over.add(d)
                self._close(d)
                return
            queued[d] = queued.get(d, 0) + n
            box.setdefault(d, []).append((op, body))

        closing = []   # a connection's CLOSE reply goes out behind everything else it gets
        for me, msgs in conns:
            stopped = False   # behind a malformed message: only its PINGs and its CLOSE are still answered
            for op, body in msgs:
                if op == 9:
                    write(me, 10, body)
                elif op == 8:
                    closing.append((me, body))
                    self._close(me)
                    break
                elif op == FAIL:
                    self._close(me)
                    break
                elif op in (1, 2) and not stopped:
                    kind, room, h = T.parse(body, self.ntopics)
                    if kind == T.RK_PUB:
                        for d in before[room]:
                            if d != me or self.self_too:
                                write(d, op, body[h:])
                    elif kind == T.RK_SUB:
                        self._join(room, me)
                    elif kind == T.RK_UNSUB:
                        self._leave(room, me)
                    else:
                        self._close(me)
                        stopped = True
        for me, body in sorted(closing):
            write(me, 8, body)
        # an over destination whose connection came later in the turn may have joined since
        for d in over:
            self._close(d)
        for op, t, d in host_events:
            if op == JOIN:
                self._join(t, d)
            elif op == LEAVE:
                self._leave(t, d)
            else:
                self._close(d)
        return box, sorted(over)
