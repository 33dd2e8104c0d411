"""GPU: a destroyed context holds nothing.  hvws_debug_dump's first line ends
with the device and pinned bytes the library holds through its grow-only
buffers, process-wide (include/hvws.h); a cycle -- create a context, run the
scan paths, every table pass with its per-connection input, the transmit side,
both host entry paths and the readback, destroy the context -- must leave both
figures where they were, and must have moved them on the way.

The batch: three connections, a few dozen frames of at most 200 bytes, in two
reads each.  Connection 0's text message arrives in two fragments, one per
read, with a PING between them; connection 1 has unmasked frames among masked
ones.  The RFC pass of each read is compared with tests/wsrfc.py, so the cycle
is known to have run what it claims."""
from __future__ import annotations

import os
import random
import re

import numpy as np
import pytest

import libhv_amd
import wsharness as H
import wsmsg as M
import wsrfc as R
import wssend as S

pytestmark = pytest.mark.gpu

FIN, MASK = M.FIN, M.MASK
KEY = b"\x11\x22\x33\x44"
CAP = 8192
POLICY = S.R_SERVER | S.R_ECHO


def held():
    """(device bytes, pinned bytes) from the first line of hvws_debug_dump."""
    r, w = os.pipe()
    try:
        libhv_amd.lib().hvws_debug_dump(w)
    finally:
        os.close(w)
    with os.fdopen(r) as f:
        first = f.readline()
    m = re.search(r"holding (\d+) device bytes, (\d+) pinned bytes", first)
    assert m, first
    return int(m.group(1)), int(m.group(2))


def reads():
    """Two reads of three connections: [[bytes per connection], [...]]."""
    rng = random.Random(5)
    body = lambda: rng.randbytes(rng.randint(0, 200))
    c0 = [H.build_frames_ref([(1 | MASK, b"caf\xc3", KEY), (9 | FIN | MASK, b"ping", KEY)]),
          H.build_frames_ref([(0 | FIN | MASK, b"\xa9 au lait", KEY)] + [(2 | FIN | MASK, body(), KEY) for _ in range(8)])]
    c1 = [H.build_frames_ref([(2 | FIN, body(), None), (1 | FIN | MASK, b"text", KEY)] * 6),
          H.build_frames_ref([(1 | FIN, b"plain", None), (8 | FIN | MASK, b"\x03\xe8bye", KEY)])]
    c2 = [H.build_frames_ref([(2 | FIN | MASK, body(), KEY) for _ in range(12)]),
          H.build_frames_ref([(2 | MASK, body(), KEY), (0 | FIN | MASK, body(), KEY)])]
    return [[c0[0], c1[0], c2[0]], [c0[1], c1[1], c2[1]]]


def cycle():
    """One context from creation to destruction; returns held() just before the destruction."""
    L = libhv_amd.lib()
    chain = R.Chain(3)
    with libhv_amd.Engine(0) as eng:
        outs = [eng.alloc(CAP + 64), eng.alloc(CAP + 64)]
        plain, wire = eng.alloc(CAP + 64), eng.alloc(2 * CAP)
        u8 = np.zeros(3, np.uint32)
        ck = np.zeros(3, np.uint32)
        closed = np.zeros(3, np.uint8)
        prev_len = 0
        for k, row in enumerate(reads()):
            data, segs, _, carries, st = chain.inputs(row)
            want = chain.oracle(row)
            nrec = sum(len(H.scan_segment(r, c)[0]) for r, c in zip(row, carries))
            host = np.frombuffer(data, np.uint8)
            rx = eng.to_device(host)
            cur, old = outs[k % 2], outs[(k + 1) % 2]
            # the scan alone, then the three message forms, the check and the server's turn
            eng.scan(rx, len(data), segs, carries)
            eng.utf8(rx, len(data), True, u8)
            eng.messages(rx, len(data), True, plain, CAP, np.zeros(3, libhv_amd.MSG_STATE_DTYPE))
            eng.messages_joined(rx, len(data), True, plain, CAP, np.zeros(3, libhv_amd.MSG_STATE_DTYPE), None, 0,
                                np.zeros(3, np.uint64))
            eng.msg_carry(3)
            eng.messages_rfc(rx, len(data), True, cur, CAP, st, old if k else None, prev_len)
            assert eng.message_table().tolist() == want[1].tolist(), k
            assert bytes(cur.download(len(want[0]))) == want[0], k
            eng.check(libhv_amd.C_ALL, 0, ck)
            eng.replies_checked(POLICY, closed)
            table, d_n, n = eng.replies_device()
            eng.send_messages(wire, 2 * CAP, cur, CAP, table, n, d_n)
            eng.reply_table(), eng.segment_replies(3), eng.segment_messages(3)
            closed_out = (eng.reply_flags(3) & S.RF_CLOSED).astype(np.uint8)
            u8_out, ck_out = eng.utf8_result(3)[0], eng.check_result(3)[0]
            # the same read through both steps (they unmask in place), the passes behind each
            for step in (eng.step, eng.step_resident):
                rx.upload(host)
                step(rx, len(data), segs, carries)
                assert len(eng.frames()) == nrec, k
                eng.utf8(rx, len(data), False, u8)
                eng.messages_rfc(rx, len(data), False, plain, CAP, st, old if k else None, prev_len)
                assert eng.message_table().tolist() == want[1].tolist(), k
                eng.check(libhv_amd.C_ALL, 0, ck)
            eng.sync()
            rx.free()
            chain.take(want, row)
            prev_len, u8, ck, closed = len(want[0]), u8_out, ck_out, closed_out
        assert (1, b"caf\xc3\xa9 au lait") in chain.merged[0] and (9, b"ping") in chain.merged[0]
        # the transmit side on its own
        tx = libhv_amd.TxPlan(eng, [0, 5], [5, 3], [1 | FIN, 2 | FIN | MASK], [0, 0x44332211])
        pay = eng.to_device(np.arange(16, dtype=np.uint8))
        assert eng.build_frames(wire, 2 * CAP, pay, 16, tx) == (2 + 5) + (6 + 3)
        eng.sync()
        tx.free()
        pay.free()
        # host memory: the small path, then the staged path with its readback
        data, segs, _, _, _ = R.Chain(3).inputs(reads()[0])
        nrec = sum(len(H.scan_segment(r)[0]) for r in reads()[0])
        for limit in (0, (1 << 64) - 1):   # the default limit, then no small path at all
            L.hvws_set_small_batch_limit(eng.ctx, limit)
            eng.rx_batch(np.frombuffer(data, np.uint8).copy(), segs)
            assert len(eng.frames()) == nrec
        for b in outs + [plain, wire]:
            b.free()
        return held()


def test_a_destroyed_context_holds_nothing():
    cycle()   # what the process creates once and keeps exists from here on
    before = held()
    inside = cycle()
    after = held()
    print(f"(device, pinned) bytes held: before {before}, inside the cycle {inside}, after {after}")
    assert after == before, (before, inside, after)
    assert inside[0] > before[0] and inside[1] > before[1], (before, inside)
