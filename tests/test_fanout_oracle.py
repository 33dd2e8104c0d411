"""CPU: the invariants of the hvws_fanout model (tests/wsfan.py) that the GPU
test then holds the device to, over reply tables made by the reply oracles of
tests/wsrfc.py from random small turns:

  - a destination's deliveries are in reply order, its own CLOSE last;
  - with every topic equal to {its sender} and HVWS_FAN_SELF, the output is a
    permutation of the reply table grouped by dest_of;
  - the delivery count is the sum of the list sizes reached minus the self edges;

and the binding declares what the model speaks of."""
from __future__ import annotations

import ctypes
import random

import pytest

import libhv_amd
import wsfan as W
import wsrfc as R
import wssend as S

POLICY = S.R_SERVER | S.R_ECHO


@pytest.fixture(autouse=True)
def _bound():
    """The entry points exist, with the constants the model uses."""
    assert (W.FAN_NONE, W.FAN_SELF) == (libhv_amd.FAN_NONE, libhv_amd.FAN_SELF)
    L = libhv_amd.lib()
    for name in ("hvws_fanout", "hvws_fanout_device", "hvws_fanout_count_device", "hvws_fanout_count",
                 "hvws_get_fanout", "hvws_get_dest_fanout"):
        assert hasattr(L, name) and name in libhv_amd._SIGS, name
    assert len(libhv_amd._SIGS["hvws_fanout"][1]) == 11
    assert libhv_amd._SIGS["hvws_fanout"][1][10] == ctypes.POINTER(ctypes.c_uint64)


def turns(seed: int, n: int):
    """n random turns: (replies, senders, topics, ndest, pub, dest_of, flags)."""
    rng = random.Random(seed)
    for _ in range(n):
        reads, topics, ndest, pub, dest_of, flags = W.random_case(rng)
        data, segs, _, _, _ = R.Chain(len(reads)).inputs(reads)
        pieces = R.rfc_batch(data, segs)[1]
        rep, answered, _, _ = R.replies_of(pieces, len(reads), POLICY)
        yield rep, W.senders(pieces, answered), topics, ndest, pub, dest_of, flags


def test_the_cases_cover_the_ground():
    ops, selfs, twice, empty = set(), 0, 0, 0
    for rep, snd, topics, ndest, pub, dest_of, flags in turns(2024, 200):
        ops |= {r[2] & 0xF for r in rep}
        es = W.edges(rep, snd, topics, pub, dest_of, W.FAN_SELF)
        selfs += sum(1 for d, _, i, _ in es if rep[i][2] & 0xF in (1, 2) and d == dest_of[snd[i]])
        twice += sum(1 for t in topics if len(set(t)) < len(t))
        empty += 0 if es else 1
    assert ops == {1, 2, 8, 10} and selfs and twice and empty


def test_per_destination_order_is_reply_order_with_close_last():
    for rep, snd, topics, ndest, pub, dest_of, flags in turns(1, 300):
        table, reply, first, count = W.fanout(rep, snd, topics, ndest, pub, dest_of, flags)
        assert sum(count) == len(table) == len(reply)
        assert all(first[d + 1] == first[d] + count[d] for d in range(ndest - 1)) and (not ndest or first[0] == 0)
        for d in range(ndest):
            mine = reply[first[d]: first[d] + count[d]]
            assert [tuple(rep[i]) for i in mine] == table[first[d]: first[d] + count[d]]
            closes = [i for i in mine if rep[i][2] & 0xF == 8]
            rest = [i for i in mine if rep[i][2] & 0xF != 8]
            assert mine == rest + closes and rest == sorted(rest)
            # "close is final" is the reply pass's: at most one CLOSE, the destination's own
            assert len(closes) <= 1 and all(dest_of[snd[i]] == d for i in closes)


def test_singleton_topics_with_self_give_the_reply_table_grouped_by_destination():
    for rep, snd, topics, ndest, pub, dest_of, flags in turns(2, 300):
        nconn = len(dest_of)
        own = [[dest_of[s]] for s in range(nconn)]
        table, reply, first, count = W.fanout(rep, snd, own, ndest, list(range(nconn)), dest_of, W.FAN_SELF)
        assert sorted(reply) == list(range(len(rep)))
        for d in range(ndest):
            mine = reply[first[d]: first[d] + count[d]]
            assert all(dest_of[snd[i]] == d for i in mine)
        # and without HVWS_FAN_SELF only the control replies are left
        table, reply, _, _ = W.fanout(rep, snd, own, ndest, list(range(nconn)), dest_of, 0)
        assert sorted(reply) == [i for i, r in enumerate(rep) if r[2] & 0xF not in (1, 2)]


def test_delivery_counts_are_list_sizes_minus_self_edges():
    for rep, snd, topics, ndest, pub, dest_of, flags in turns(3, 300):
        want = 0
        for r, s in zip(rep, snd):
            if r[2] & 0xF not in (1, 2):
                want += 1
            elif pub[s] != W.FAN_NONE:
                lst = topics[pub[s]]
                want += len(lst) - (0 if flags & W.FAN_SELF else lst.count(dest_of[s]))
        table, _, _, count = W.fanout(rep, snd, topics, ndest, pub, dest_of, flags)
        assert len(table) == want == sum(count)
        # a destination listed twice is delivered twice
        for d in range(ndest):
            got = count[d]
            exp = sum(1 for e in W.edges(rep, snd, topics, pub, dest_of, flags) if e[0] == d)
            assert got == exp


def test_flatten_is_the_subscription_table_layout():
    first, member = W.flatten([[3, 1], [], [2, 2, 0]])
    assert first.tolist() == [0, 2, 2, 5] and member.tolist() == [3, 1, 2, 2, 0]
    assert first.dtype.itemsize == 8 and member.dtype.itemsize == 4
