"""tests/ranks.py without a device: the real callbacks and the real runner on real threads, with the view of a raw pointer taken
over host memory and a synchronisation that does nothing.  What the GPU tests of every scheme's sharded run lean on -- the sum
a rank receives, the order of a gather, the blocks of an all-to-all-v, which error the caller sees -- is pinned here."""
import ctypes
import threading

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import ranks

WORLD = 3
WHOLE = random_corpus(7, 30, 9, seed=1)


def host_view(ptr, n, typestr):
    import torch
    dt = np.dtype(typestr)
    return torch.from_numpy(np.frombuffer((ctypes.c_byte * (n * dt.itemsize)).from_address(ptr), dt))


class Handle:
    """the six methods run_ranks calls"""

    def __init__(self, log=None):
        self.closed, self.mode, self.log = threading.Event(), None, log if log is not None else []

    def attach_exchange(self, rank, world, *callbacks):
        self.rank, self.world, self.callbacks = rank, world, callbacks
        self.log.append("attach")

    def set_count_exchange(self, mode):
        self.mode = mode
        self.log.append("mode")

    def set_corpus(self, doc_ptr, tokens, doc_base, tok_base):
        self.corpus = (len(doc_ptr) - 1, len(tokens), doc_base, tok_base)
        self.log.append("corpus")

    def set_global_token_count(self, n):
        self.global_tokens = n
        self.log.append("global")

    def count_exchange(self):
        return {"sparse": self.mode == "sparse"}

    def close(self):
        self.closed.set()


def run(body, handles=None, **kw):
    handles = handles if handles is not None else [Handle() for _ in range(WORLD)]
    return ranks.run_ranks(WORLD, WHOLE, lambda rank: handles[rank], body, view=host_view, sync=lambda: None, **kw)


def ptr(a):
    return a.ctypes.data


def test_reduce_scatter_sums_the_ranks_own_slices():
    count = 5
    send = [(np.arange(WORLD * count) * 7 + 1000 * (r + 1) ** 2).astype(np.int32) for r in range(WORLD)]

    def body(h, rank, sub, tok_base):
        recv = np.full(count + 2, -1, np.int32)                     # two guard elements behind
        assert h.callbacks[0](ptr(send[rank]), ptr(recv), count, None) == 0
        return recv

    handles = [Handle() for _ in range(WORLD)]
    out, counters = run(body, handles, counters=True)
    for r in range(WORLD):
        want = sum(send[s][r * count:(r + 1) * count].astype(np.int64) for s in range(WORLD))
        assert np.array_equal(out[r][:count], want) and (out[r][count:] == -1).all(), r
        assert counters[r] == dict(dense_calls=1, sparse_calls=0, pairs_sent=0)
        # what the runner did around the body: no mode given, so no set_count_exchange; the shard and its bases; four callbacks
        h = handles[r]
        assert h.log == ["attach", "corpus", "global"] and len(h.callbacks) == 4 and (h.rank, h.world) == (r, WORLD)
        sub, doc_base, tok_base = ranks.shard_of(WHOLE, r, WORLD)
        assert h.corpus == (sub.num_docs, sub.num_tokens, doc_base, tok_base) and h.global_tokens == WHOLE.num_tokens
        assert h.closed.is_set()
    assert sum(h.corpus[0] for h in handles) == WHOLE.num_docs


@pytest.mark.parametrize("typestr,which", [("<f8", 1), ("<i4", 2)], ids=["f8", "i4"])
def test_all_gather_concatenates_in_rank_order(typestr, which):
    count = 4
    if typestr == "<f8":
        nan = np.array([0x7ff8000000000123], np.uint64).view(np.float64)[0]
        send = [np.array([1.5, -0.0, 0.0, 3.25]), np.array([nan, 2.0, -7.0, 5e-324]), np.array([-0.0, np.nan, 9.0, 1e308])]
    else:
        send = [np.array([1, -2, 3, 2**31 - 1], np.int32), np.array([5, 6, -2**31, 8], np.int32), np.array([9, 10, 11, -12], np.int32)]

    def body(h, rank, sub, tok_base):
        recv = np.zeros(count * WORLD, np.dtype(typestr))
        assert h.callbacks[which](ptr(send[rank]), ptr(recv), count, None) == 0
        return recv

    # cuts in place of the even split, one shard empty; three callbacks; a mode that is set and then checked
    handles = [Handle() for _ in range(WORLD)]
    out = run(body, handles, cuts=[0, 5, 5, 7], all_to_all=False, mode="dense")
    want = np.concatenate(send)
    for r in range(WORLD):
        assert out[r].tobytes() == want.tobytes(), r
        ranks.assert_bit_equal(out[r], want, "rank %d" % r)
        assert len(handles[r].callbacks) == 3 and handles[r].log == ["attach", "mode", "corpus", "global"]
    assert [h.corpus[0] for h in handles] == [5, 0, 2] and [h.corpus[2] for h in handles] == [0, 5, 5]


# CNT[s][d]: what rank s addresses to rank d -- an empty block (0 -> 1), a rank that sends nothing (2)
CNT = [[2, 0, 4], [6, 2, 2], [0, 0, 0]]


def all_to_all_case(rcnt_of):
    base = [np.arange(32, dtype=np.int32) + 100 * (s + 1) for s in range(WORLD)]

    def body(h, rank, sub, tok_base):
        soff, roff = [7 * d + rank for d in range(WORLD)], [8 * s + rank for s in range(WORLD)]     # gaps between the blocks, none aligned
        recv = np.full(32, -1, np.int32)
        assert h.callbacks[3](ptr(base[rank]), soff, CNT[rank], ptr(recv), roff, rcnt_of(rank), None) == 0
        return recv

    out, counters = run(body, mode="sparse", counters=True)
    return base, out, counters


def test_all_to_all_v_moves_every_block_to_its_offset():
    base, out, counters = all_to_all_case(lambda rank: [CNT[s][rank] for s in range(WORLD)])
    for r in range(WORLD):
        want = np.full(32, -1, np.int32)
        for s in range(WORLD):
            want[8 * s + r:8 * s + r + CNT[s][r]] = base[s][7 * r + s:7 * r + s + CNT[s][r]]
        assert np.array_equal(out[r], want), r
        assert counters[r] == dict(dense_calls=0, sparse_calls=1, pairs_sent=sum(CNT[r]) // 2)
    assert [c["pairs_sent"] for c in counters] == [3, 5, 0]


def test_all_to_all_v_refuses_a_block_of_another_size():
    """rank 1 announces one element from rank 0, which sends it none"""
    with pytest.raises(AssertionError, match="rank 1 expected 1 elements from rank 0, got 0"):
        all_to_all_case(lambda rank: [CNT[s][rank] + (rank == 1 and s == 0) for s in range(WORLD)])


def gather(h, rank):
    recv = np.zeros(WORLD, np.int32)
    return h.callbacks[2](ptr(np.array([rank], np.int32)), ptr(recv), 1, None)


def test_the_caller_sees_the_error_not_the_broken_barrier():
    handles = [Handle() for _ in range(WORLD)]

    def body(h, rank, sub, tok_base):
        if rank == 1:
            raise ValueError("rank 1")
        return gather(h, rank)                                      # waits for rank 1, which never comes

    with pytest.raises(ValueError, match="rank 1"):
        run(body, handles)
    assert all(h.closed.is_set() for h in handles)

    # the barrier error of a rank that gave up is in the list BEFORE the error of the rank it was waiting for
    handles = [Handle() for _ in range(WORLD)]

    def late(h, rank, sub, tok_base):
        if rank == 0:
            raise threading.BrokenBarrierError
        if rank == 1:
            assert handles[0].closed.wait(60)                       # set behind rank 0's entry in the list
            raise ValueError("late")
        return gather(h, rank)

    with pytest.raises(ValueError, match="late"):
        run(late, handles)
    assert all(h.closed.is_set() for h in handles)

    # nothing but barrier errors: the first of them
    def only_barriers(h, rank, sub, tok_base):
        if rank == 2:
            raise threading.BrokenBarrierError
        return gather(h, rank)

    with pytest.raises(threading.BrokenBarrierError):
        run(only_barriers)

    # the form that was asked for is checked after the body
    def switches(h, rank, sub, tok_base):
        h.set_count_exchange("dense")

    with pytest.raises(AssertionError):
        run(switches, mode="sparse")
    assert run(switches, mode="auto") == [None] * WORLD


def test_assert_bit_equal_rejects_what_differs():
    nan = np.array([0x7ff8000000000001, 0x7ff8000000000002], np.uint64).view(np.float64)
    ranks.assert_bit_equal([0.0, -0.0, nan[0]], [0.0, -0.0, nan[0]], "equal doubles")
    ranks.assert_bit_equal(np.arange(4, dtype=np.int32), np.arange(4, dtype=np.int64), "equal integers")
    ranks.assert_bit_equal(np.float32([1.5, -0.0]), np.float64([1.5, -0.0]), "float32 against its double")
    ranks.assert_bit_equal(3, 3, "scalars")
    for a, b, message in (([1.0, 0.0], [1.0, -0.0], r"1 of 2 differ, first at \[1\]: \S*\b0\.0\S* vs \S*-0\.0"),
                          (nan[:1], nan[1:], "1 of 1 differ"),
                          (np.zeros((2, 3)), np.zeros((3, 2)), r"shapes \(2, 3\) and \(3, 2\)"),
                          (np.zeros(3, np.int32), np.zeros(4, np.int32), r"shapes \(3,\) and \(4,\)"),
                          (np.int32([1, 2, 3, 4]), np.int32([1, 5, 3, 6]), r"2 of 4 differ, first at \[1\]: \S*\b2\S* vs \S*\b5"),
                          (np.float32([0.0]), np.float32([-0.0]), "1 of 1 differ"),
                          ([1.0, 2.0], [1, 2], "float64 against int64"),
                          ([1, 2], [1.0, 2.0], "int64 against float64"),
                          (1.0, 2.0, "1 of 1 differ")):
        with pytest.raises(AssertionError, match=message):
            ranks.assert_bit_equal(a, b, "x")
