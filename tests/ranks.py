"""A world of ranks in one process: `world` handles driven by threads and joined by attach_exchange callbacks over an in-memory
barrier transport (host staging).  The one copy of what every scheme's sharded test needs -- the transport, the callbacks, the
shard of a rank, the runner that starts, joins and reports the ranks -- with assert_bit_equal and the two one-line helpers the
forced-form tests share.  The collective logic is pinned without a device by tests/test_ranks_model.py."""
import threading

import numpy as np

from ldagroupedgibbssampler_amd.corpus import even_split


def assert_bit_equal(a, b, what):
    """Equal shapes; floating point against floating point only, as bit patterns (-0.0 is not 0.0, a NaN equals only the NaN
    with its payload); everything else by value."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, "%s: shapes %s and %s" % (what, a.shape, b.shape)
    assert (a.dtype.kind == "f") == (b.dtype.kind == "f"), "%s: %s against %s" % (what, a.dtype, b.dtype)
    if a.dtype.kind == "f":
        bad = np.ascontiguousarray(a, np.float64).view(np.int64) != np.ascontiguousarray(b, np.float64).view(np.int64)
    else:
        bad = np.asarray(a != b)
    if bad.any():
        first = np.unravel_index(np.flatnonzero(bad)[0], a.shape)
        raise AssertionError("%s: %d of %d differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, [int(i) for i in first], a[first], b[first]))


def force_form(monkeypatch, margin):
    monkeypatch.setenv("GGS_DEBUG", "1")
    if margin is None:
        monkeypatch.delenv("GGS_DEBUG_MARGIN", raising=False)
    else:
        monkeypatch.setenv("GGS_DEBUG_MARGIN", margin)


def z_kernel(g):
    return g.launch_info()["z_kernel"]


class Transport:
    """In-memory collectives between handles driven by threads of one process."""

    def __init__(self, n):
        self.n, self.bar, self.box = n, threading.Barrier(n, timeout=300), [None] * n

    def exchange(self, rank, payload):
        self.box[rank] = payload
        self.bar.wait()
        got = list(self.box)
        self.bar.wait()
        return got


def device_view():
    """n elements at a raw device pointer as a tensor on cuda:0"""
    import torch
    from ldagroupedgibbssampler_amd.sharded import _DevPtr
    dev = torch.device("cuda", 0)

    def view(ptr, n, typestr):
        return torch.as_tensor(_DevPtr(ptr, n, typestr), device=dev)
    return view


def exchange_callbacks(tr, rank, world, all_to_all=True, counters=None, view=None, sync=None):
    """(reduce_scatter_i32, all_gather_f64, all_gather_i32[, all_to_all_v_i32]) over a Transport, through host staging.
    counters: the rank's dict, in which dense_calls (reduce-scatters), sparse_calls (all-to-all-vs) and pairs_sent (the
    (cell, count) pairs this rank addressed to anybody) are kept.  view / sync: what touches the device (device_view(),
    torch.cuda.synchronize)."""
    import torch
    view = view or device_view()
    sync = sync or torch.cuda.synchronize
    counters = counters if counters is not None else new_counters()

    def reduce_scatter_i32(send, recv, count, stream):
        sync()
        parts = tr.exchange(rank, view(send, count * world, "<i4").cpu().numpy().reshape(world, count))
        view(recv, count, "<i4").copy_(torch.from_numpy(np.sum([p[rank] for p in parts], axis=0, dtype=np.int32)))
        sync()
        counters["dense_calls"] += 1
        return 0

    def all_gather(typestr):
        def cb(send, recv, count, stream):
            sync()
            parts = tr.exchange(rank, view(send, count, typestr).cpu().numpy())
            view(recv, count * world, typestr).copy_(torch.from_numpy(np.concatenate(parts)))
            sync()
            return 0
        return cb

    def all_to_all_v(send, soff, scnt, recv, roff, rcnt, stream):
        sync()
        total = max(soff[i] + scnt[i] for i in range(world))
        mine = view(send, max(total, 1), "<i4").cpu().numpy()
        everyone = tr.exchange(rank, [mine[soff[d]:soff[d] + scnt[d]].copy() for d in range(world)])   # everyone[s][d]: what rank s addresses to rank d
        for s_ in range(world):
            got = everyone[s_][rank]
            assert got.size == rcnt[s_], "rank %d expected %d elements from rank %d, got %d" % (rank, rcnt[s_], s_, got.size)
            if got.size:
                view(recv + 4 * roff[s_], got.size, "<i4").copy_(torch.from_numpy(got))
        sync()
        counters["sparse_calls"] += 1
        counters["pairs_sent"] += sum(scnt[d] for d in range(world)) // 2
        return 0

    return (reduce_scatter_i32, all_gather("<f8"), all_gather("<i4")) + ((all_to_all_v,) if all_to_all else ())


def new_counters():
    return dict(dense_calls=0, sparse_calls=0, pairs_sent=0)


def shard_of(whole, rank, world, doc_off=0, tok_off=0, cuts=None):
    """(sub-corpus, doc_base, tok_base) of a rank: documents split evenly and contiguously, or at `cuts` (world + 1 document
    boundaries).  doc_off / tok_off: the global indices of the first document / token of `whole` itself (a corpus that is a
    part of a larger one)."""
    bounds = even_split(whole.num_docs, world) if cuts is None else cuts
    assert len(bounds) == world + 1
    sub, doc_base, tok_base = whole.shard(bounds[rank], bounds[rank + 1])
    return sub, doc_base + doc_off, tok_base + tok_off


def run_ranks(world, whole, make_handle, body, mode=None, all_to_all=True, cuts=None, doc_off=0, tok_off=0, counters=False, through=None,
              view=None, sync=None):
    """`world` threads, each with one handle from make_handle(rank) (called in the rank's thread) joined to the others, its shard
    of `whole` (shard_of) set as corpus; body(h, rank, sub, tok_base) runs on each and the return values come back in rank order
    -- with counters=True as (results, the ranks' counters of exchange_callbacks).  Every collective call of body must be made by
    every rank in the same order.

    mode: the form of the count exchange ("auto", "dense", "sparse"), set before the corpus; None: ggs_set_count_exchange is not
    called.  After the body a "dense" or "sparse" must be the form that ran.  all_to_all=False attaches three callbacks, no
    all_to_all_v_i32.  With doc_off / tok_off the handles' bases are offset; body's tok_base stays the shard's first token WITHIN
    `whole` (what slices a z of the whole corpus).  through(h, attach, rank): takes the place of set_corpus and
    set_global_token_count for a caller whose own object shards and attaches (ShardedGGS); attach(engine) is attach_exchange and
    set_count_exchange on the engine it is handed.

    A rank that raises aborts the barrier; the caller gets the first exception that is not the BrokenBarrierError of a rank
    that was merely waiting.  Every handle is closed."""
    tr, out, errs, counts = Transport(world), [None] * world, [], [new_counters() for _ in range(world)]

    def rank_main(rank):
        h = None
        try:
            sub, doc_base, tok_base = shard_of(whole, rank, world, doc_off, tok_off, cuts)
            h = make_handle(rank)

            def attach(engine):
                engine.attach_exchange(rank, world, *exchange_callbacks(tr, rank, world, all_to_all, counts[rank], view, sync))
                if mode is not None:
                    engine.set_count_exchange(mode)

            if through is None:
                attach(h)
                h.set_corpus(sub.doc_ptr, sub.tokens, doc_base, tok_base)
                h.set_global_token_count(whole.num_tokens)
            else:
                through(h, attach, rank)
            out[rank] = body(h, rank, sub, tok_base - tok_off)
            if mode in ("dense", "sparse"):
                assert h.count_exchange()["sparse"] == (mode == "sparse")
        except BaseException as e:                      # noqa: BLE001 -- re-raised by the caller
            errs.append(e)
            tr.bar.abort()
        finally:
            if h is not None:
                h.close()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise ([e for e in errs if not isinstance(e, threading.BrokenBarrierError)] or errs)[0]
    return (out, counts) if counters else out
