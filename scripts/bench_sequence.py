#!/usr/bin/env python3
"""hvws_sequence and hvws_envelope_sequenced measurement, everything in one loop
on one tree, the two sides of each comparison alternating in order:

  * hvws_sequence's device time beside hvws_route's on the same batch, per
    reply, and the sort's share of it: the same call behind a route with
    ntopics = 0 runs no sort pass (fan_key_passes(0) == 0) and the same pair,
    scan, number and counter kernels;
  * hvws_envelope_sequenced's device time beside hvws_envelope's on the same
    batch, each with its table part alone (behind the ntopics = 0 route every
    message is BAD or STOPPED, nothing is copied) and the copy as the
    difference;
  * the whole turn: sequence + sequenced envelope + enveloped fan-out + send
    beside envelope + enveloped fan-out + send.

The shapes are scripts/bench_envelope.py's: one card, device resident, 4096
connections (one segment each) of masked FIN binary frames in rooms of 16
(256 topics: two sort passes), HVWS_FAN_SELF set;
  * "c3": 64 KiB frames (FRAMES_C3 of them);
  * "c2": 1 KiB frames (FRAMES_C2 of them).
Every message is "P<room>\\n" + body; the envelope names topic and sender
(HVWS_ENV_SENDER).  Run one process per shape (FRAMES_C2=0 or FRAMES_C3=0).
Checks, in the same run: the numbers, the totals and the counters against numpy
on the host, before the loop and after it; the sequenced rows and totals
against numpy; the bytes of SAMPLE replies spread over the batch (line, body,
and the pad behind them untouched).

Not measured: skewed topics (one hot topic), ntopics above 65 536 (a third
sort pass), turns without the sender.

REPS sets the repetitions.  Prints JSON lines.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]

import libhv_amd  # noqa: E402
from libhv_amd import synth  # noqa: E402
from bench_fanout import FIN, FRAGMENT, NSEG, ROOM, span  # noqa: E402

SAMPLE = 1024
SEED = 0xA5
START = 10 ** 10 - 3            # the counters' seed: numbers of 10 and 11 digits


def digits(v: np.ndarray) -> np.ndarray:
    v = np.asarray(v, np.int64)
    return 1 + sum((v >= 10 ** k).astype(np.int64) for k in range(1, 19))


def shape(eng, name, frames, payload, reps):
    L = libhv_amd.lib()
    p = synth.uniform_plan(frames, payload, 1).split(NSEG)
    nseg = len(p.segments)
    assert nseg % ROOM == 0 and nseg <= 10000
    dp = libhv_amd.DevicePlan(eng, p)
    rx = eng.alloc(p.total + 64)
    msg = eng.alloc(p.total + 64)
    eng.synth(rx, p.total, p.seed, dp, 0)
    op = int(p.flags[0]) & 0xF
    assert op in (1, 2) and bool((p.flags & FIN).all()), "the shapes are FIN data frames"
    policy = libhv_amd.R_SERVER | libhv_amd.R_ECHO
    old_run = L.hvws_set_run(eng.ctx, 0)
    eng.scan(rx, p.total, p.segments)
    eng.messages(rx, p.total, True, msg, p.total)
    eng.replies(policy)
    assert L.hvws_reply_count(eng.ctx) == p.n, "one echo per frame"
    nbytes = eng.msg_bytes()
    rep_table, _ = eng.reply_table()
    rfirst, rcount = eng.segment_replies(nseg)
    sender = np.repeat(np.arange(nseg, dtype=np.int64), rcount.astype(np.int64))
    room = sender // ROOM
    # "P<room>\n" over the first bytes of every message, in the message call's output
    host = msg.download(nbytes)
    off = rep_table["off"].astype(np.int64)
    assert int(rep_table["len"].min()) >= 8
    for r in range(nseg // ROOM):
        h = np.frombuffer(b"P%d\n" % r, np.uint8)
        at = off[room == r]
        for k in range(len(h)):
            host[at + k] = h[k]
    libhv_amd._check(L.hvws_h2d(eng.ctx, msg.ptr, host.ctypes.data, nbytes), "hvws_h2d")
    eng.sync()
    ntopics = nseg // ROOM
    topic_first = np.arange(ntopics + 1, dtype=np.uint64) * ROOM
    member = np.arange(nseg, dtype=np.uint32)
    d_first, d_member = eng.to_device(topic_first), eng.to_device(member)
    dest_of = np.arange(nseg, dtype=np.uint32)
    ctr = eng.to_device(np.full(ntopics, START, np.uint64))

    eng.route(ntopics, nseg, dest_of)
    env_cap = eng.envelope_sequenced_bound()
    assert env_cap == p.total + 60 * int(L.hvws_reply_capacity(eng.ctx)) + 16 >= eng.envelope_bound()
    env = eng.alloc(env_cap + 64)
    libhv_amd._check(L.hvws_memset(eng.ctx, env.ptr, SEED, env_cap + 64), "hvws_memset")

    # the numbering against numpy: a stable sort by topic and each element's rank in its run
    rows, topic, kind = eng.route_table()
    assert bool((kind == libhv_amd.RK_PUB).all()) and np.array_equal(topic.astype(np.int64), room)
    order = np.argsort(room, kind="stable")
    st = room[order]
    pos = np.arange(p.n, dtype=np.int64)
    head = np.ones(p.n, bool)
    head[1:] = st[1:] != st[:-1]
    rank = np.zeros(p.n, np.int64)
    rank[order] = pos - np.maximum.accumulate(np.where(head, pos, 0))
    per_topic = np.bincount(room, minlength=ntopics).astype(np.int64)
    eng.sequence(ctr)
    seq = eng.sequence_table().astype(np.int64)
    assert np.array_equal(seq, START + 1 + rank)
    assert eng.sequence_totals() == (p.n, int((per_topic > 0).sum()))
    assert np.array_equal(ctr.download(8 * ntopics).view(np.uint64).astype(np.int64), START + per_topic)

    # the sequenced envelope against numpy
    eng.envelope_sequenced(env, env_cap, libhv_amd.ENV_SENDER)
    blen = rows["len"].astype(np.int64)
    src = rows["off"].astype(np.int64)
    eh = 5 + digits(room) + digits(sender) + digits(seq)         # 'M' topic ' ' sender ' ' '#' seq LF
    size = eh + blen
    e = np.concatenate(([0], np.cumsum((size + 15) // 16 * 16)))
    got = eng.envelope_table()
    assert np.array_equal(got["off"].astype(np.int64), e[:-1]) and np.array_equal(got["len"].astype(np.int64), size)
    assert np.array_equal(got["flags"], rows["flags"]) and np.array_equal(got["key"], rows["key"])
    written, spanned = int(size.sum()), int(e[-1])
    assert eng.envelope_totals() == (p.n, 0, written, spanned), eng.envelope_totals()
    for i in np.unique(np.linspace(0, p.n - 1, SAMPLE).astype(np.int64)):
        padded = int(e[i + 1] - e[i])
        mine = np.zeros(padded, np.uint8)
        libhv_amd._check(L.hvws_d2h(eng.ctx, mine.ctypes.data, env.ptr + int(e[i]), padded), "hvws_d2h")
        eng.sync()
        want = b"M%d %d #%d\n" % (room[i], sender[i], seq[i]) + host[src[i]:src[i] + blen[i]].tobytes()
        assert mine[:len(want)].tobytes() == want, f"reply {i}"
        assert bool((mine[len(want):] == SEED).all()), f"reply {i}: pad bytes written"
    del host

    def wire(lens):
        perd = np.maximum(1, -(-lens // FRAGMENT))
        nfr = int(perd.sum())
        j = np.arange(nfr, dtype=np.int64) - np.repeat(np.cumsum(perd) - perd, perd)
        pr = np.repeat(perd, perd)
        length = np.where(j + 1 < pr, FRAGMENT, np.repeat(lens - (perd - 1) * FRAGMENT, perd))
        return int((np.where(length < 126, 2, np.where(length <= 0xFFFF, 4, 10)) + length).sum()), nfr

    nfrag = -(-(payload + 64) // FRAGMENT)                 # frames per delivery, at most 10 bytes of header each
    out_cap = spanned * ROOM + 10 * nfrag * p.n * ROOM + 64
    out = eng.alloc(out_cap)

    def send():
        t, d_n, n = eng.fanout_device()
        return eng.send_messages(out, out_cap, env, env_cap, t, n, d_n, 0, False)

    def fan():
        return eng.fanout_enveloped(d_first, d_member, nseg, libhv_amd.FAN_SELF)

    plain = lambda: eng.envelope(env, env_cap, libhv_amd.ENV_SENDER)
    numbered = lambda: eng.envelope_sequenced(env, env_cap, libhv_amd.ENV_SENDER)
    ms = eng.last_kernel_ms
    M = {k: [] for k in ("route", "route_bad", "seq", "seq_span", "seq_nosort", "env", "envs", "env_tab", "envs_tab",
                         "turn_plain", "turn_seq", "send_plain", "send_seq", "fan_plain", "fan_seq")}
    sizes = {}
    for k in range(reps + 1):
        # the table parts: every message BAD or STOPPED, no sort pass, an empty copy
        eng.route(0, nseg, dest_of)
        M["route_bad"].append(ms())
        eng.sequence(None)
        M["seq_nosort"].append(ms())
        assert eng.sequence_totals() == (0, 0)
        for which in ((0, 1) if k % 2 else (1, 0)):
            (numbered if which else plain)()
            M["envs_tab" if which else "env_tab"].append(ms())
            assert eng.envelope_totals() == (0, 0, 0, 0)
        eng.route(ntopics, nseg, dest_of)
        M["route"].append(ms())
        M["seq_span"].append(span(eng, lambda: eng.sequence(ctr)))
        M["seq"].append(ms())
        for which in ((0, 1) if k % 2 else (1, 0)):
            (numbered if which else plain)()
            a = ms()
            M["envs" if which else "env"].append(a)
            b = span(eng, fan)
            M["fan_seq" if which else "fan_plain"].append(b)
            sent = send()
            c = ms()
            M["send_seq" if which else "send_plain"].append(c)
            M["turn_seq" if which else "turn_plain"].append(a + b + c + (M["seq"][-1] if which else 0.0))
            if k == 0:
                t, _ = eng.fanout_table()
                assert sent == wire(t["len"].astype(np.int64))
                sizes[which] = sent[0]
            else:
                assert sent[0] == sizes[which] or which       # the numbers' digits may grow from turn to turn
    # the counters moved on once per numbered turn
    assert np.array_equal(ctr.download(8 * ntopics).view(np.uint64).astype(np.int64), START + (reps + 2) * per_topic)
    L.hvws_set_run(eng.ctx, old_run)
    med = lambda v: float(np.median(v[1:]))
    rng = lambda v: [round(min(v[1:]), 4), round(max(v[1:]), 4)]
    row = {"bench": "sequence", "shape": name, "messages": p.n, "payload": payload, "connections": nseg, "room": ROOM,
           "topics": ntopics, "sort_passes": 2, "bytes_written": written, "bytes_spanned": spanned, "env_cap": env_cap,
           "reps": reps}
    for key, v in M.items():
        row[key + "_ms"] = round(med(v), 4)
        row[key + "_range"] = rng(v)
    copy_plain = [a - b for a, b in zip(M["env"], M["env_tab"])]
    copy_seq = [a - b for a, b in zip(M["envs"], M["envs_tab"])]
    row.update({
        "ratio_sequence_to_route": round(med(M["seq"]) / med(M["route"]), 4),
        "sequence_ns_per_reply": round(med(M["seq"]) * 1e6 / p.n, 3),
        "route_ns_per_reply": round(med(M["route"]) * 1e6 / p.n, 3),
        "sort_share_of_sequence": round(1.0 - med(M["seq_nosort"]) / med(M["seq"]), 4),
        "copy_plain_ms": round(med(copy_plain), 4), "copy_plain_range": rng(copy_plain),
        "copy_seq_ms": round(med(copy_seq), 4), "copy_seq_range": rng(copy_seq),
        "ratio_envelope_sequenced_to_envelope": round(med(M["envs"]) / med(M["env"]), 4),
        "ratio_table_part": round(med(M["envs_tab"]) / med(M["env_tab"]), 4),
        "ratio_copy_part": round(med(copy_seq) / med(copy_plain), 4),
        "ratio_turn": round(med(M["turn_seq"]) / med(M["turn_plain"]), 4),
        "out_bytes_plain": sizes[0], "out_bytes_sequenced": sizes[1],
        "checked": "numbers, totals and counters of hvws_sequence against numpy before the loop, the counters after it; "
                   "rows and totals of hvws_envelope_sequenced against numpy; line, body and pad of %d replies byte for "
                   "byte; the send's bytes and frames against the delivery table's lengths" % SAMPLE,
    })
    print(json.dumps(row), flush=True)
    for b in (rx, msg, env, out, d_first, d_member, ctr):
        b.free()
    dp.free()


def main():
    reps = int(os.environ.get("REPS", "5"))
    n3 = int(os.environ.get("FRAMES_C3", str(1 << 15)))
    n2 = int(os.environ.get("FRAMES_C2", str(1 << 20)))
    eng = libhv_amd.Engine(int(os.environ.get("HVWS_BENCH_DEVICE", "0")))
    if n3:
        shape(eng, "c3", n3, 65536, reps)
    if n2:
        shape(eng, "c2", n2, 1024, reps)
    eng.close()


if __name__ == "__main__":
    main()
