"""scheme=adlda on the device (GGS_FLAG_ADLDA): whole sweeps bit for bit against the CPU restatement
(tests/adlda_restatement.py) -- z, n_wk, n_k, the words' lists and the four bucket counters; runs behind an exchange against
one handle; the persistent grid on one CU; the interface; the held-out likelihood against scheme=collapsed's parallel
schedule; the driver and the host mirrors.

adlda_wave_kernel proposes by wave scans and replays the undecided tokens exactly (ggs_z_adlda.hpp); the smoothing bucket is
always replayed.  test_debug_margin_sends_every_token_through_the_replay runs with the margins scaled so that nothing is
decided by a scan: the same bits.  The knife-edge rows (sample == Q, sample - Q == R, a walk's rest of exactly 0.0, the
63 / 64 seam of each walk, the entries next to a zero score) are tests/adlda_knife_edge.py's: tests/test_adlda_knife_edge_gpu.py
puts them through the device, tests/test_adlda_knife_edge_model.py shows what they tell; tests/test_adlda_model.py has the
restatement's own edges on the CPU."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import adlda_restatement as R
from tests import persistent_grid as PG
from tests.diagnostics_cases import asymmetric_alpha
from tests.ranks import assert_bit_equal, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777
KERNEL = "adlda_wave_kernel"


def lds_bytes(K, longest):
    """adlda_lds_bytes (ggs_z_adlda.hpp): den0 and alpha fp64 [K], 64 fp64 terms, counts int32 [K], back-map u16 [K], list u16 [cap]"""
    cap = max(1, min(K, longest))
    return 16 * K + 512 + 4 * K + 2 * K + 2 * ((cap + 3) & ~3)


def assert_state_equal(g, m, what=""):
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z " + what)
    assert_bit_equal(g.sparse_stats(), m.stats, "bucket counters " + what)
    assert_bit_equal(g.get_type_topic_counts(), m.counts(), "n_wk " + what)
    assert_bit_equal(g.get_topic_totals(), m.topic_totals(), "n_k " + what)
    nw, lists = m.lists()
    gnw, glists = g.word_topic_lists()
    assert_bit_equal(gnw, nw, "nw " + what)
    assert_bit_equal(glists, lists, "lists " + what)


def run_pair(native, c, K, alpha, beta, sweeps, z0=None, zseed=5):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_ADLDA | native.FLAG_PARANOID)
    g.set_corpus(c.doc_ptr, c.tokens)
    if z0 is None:
        g.init_z_java_lcg(zseed)
        z0 = g.get_z()
        assert_bit_equal(z0, java_lcg_initial_z(c.num_tokens, K, zseed), "initial z")
        g.init_phi()
    else:
        g.set_z(z0, redraw_phi=True)
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0)
    assert_state_equal(g, m, "before the first sweep")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_state_equal(g, m, "after sweep %d" % (s + 1))
    assert g.launch_info()["z_kernel"].startswith(KERNEL)
    assert_bit_equal(g.get_phi(), m.phi(), "the point estimate")
    assert int(m.stats[:3].sum()) == sweeps * c.num_tokens
    return g, m


# ---- whole runs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 20, 100])
@pytest.mark.parametrize("alpha,beta", [(5.0, 7.0), (0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, K, alpha, beta):
    g, m = run_pair(native, cats, K, alpha, beta, 2)
    print("K = %d alpha = %g beta = %g: tokens from Q, R, S %s; mean candidates %.1f" % (K, alpha, beta, m.stats[:3].tolist(), m.stats[3] / m.stats[:3].sum()))
    assert m.stats[0] > 0
    if alpha == 5.0:                                                # large priors: all three buckets are drawn from (at 0.1 / 0.01 the word's takes nearly all)
        assert (m.stats[:3] >= 200).all()
    g.close()


def test_cats_with_asymmetric_alpha(native, oracle, cats):
    g, m = run_pair(native, cats, 20, asymmetric_alpha(20), 0.01, 2)
    print("tokens from Q, R, S: %s" % m.stats[:3].tolist())
    assert m.stats[0] > 0 and m.stats[1] > 0
    g.close()


def test_ragged_corpus(native, oracle):
    """Documents of 0, 1, 2, 63, 64, 65 and 129 tokens (the chunk boundaries and the look-ahead past them) between empty ones,
    V = 7 of which one word has no token, K = 5."""
    rng = np.random.default_rng(3)
    lens = np.array([63, 0, 1, 64, 0, 129, 65, 1, 0, 2, 0], np.int64)
    tokens = rng.integers(0, 6, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 7)
    g, m = run_pair(native, c, 5, 1.5, 0.5, 3)
    nw, _ = g.word_topic_lists()
    assert nw[6] == 0 and (nw[:6] > 0).all()                        # the unused word has an empty list
    print("tokens from Q, R, S: %s" % m.stats[:3].tolist())
    assert m.stats[0] > 0 and m.stats[1] + m.stats[2] > 0
    g.close()


@pytest.mark.parametrize("K", [64, 65, 130])
def test_word_lists_across_the_64_topic_seam(native, oracle, K):
    """V = 3 and 20 documents of 150 tokens: 1 000 tokens per word keep every list long -- more than 60 entries, and past 64
    (a second block of terms, gathered without the look-ahead) at K = 65 and 130; asserted from the restatement."""
    rng = np.random.default_rng(K)
    lens = np.full(20, 150, np.int64)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), rng.integers(0, 3, lens.sum()).astype(np.int32), 3)
    g, m = run_pair(native, c, K, 0.1, 0.01, 2)
    nw, _ = m.lists()
    print("K = %d: list lengths %s" % (K, nw.tolist()))
    assert (nw > 60).all() and (K == 64 or (nw > 64).all())
    g.close()


def test_a_document_list_of_more_than_64_entries(native, oracle):
    """K = 130; one document of 400 tokens that ggs_set_z spreads over 110 topics (and four short ones): its list is walked in
    two blocks for both R's sum and R's walk.  The length is counted from the restatement's state."""
    rng = np.random.default_rng(11)
    lens = np.array([30, 400, 5, 70, 1], np.int64)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), rng.integers(0, 40, lens.sum()).astype(np.int32), 40)
    K = 130
    z0 = rng.integers(0, K, c.num_tokens).astype(np.int32)
    z0[30:430] = rng.permutation(K)[:110][np.arange(400) % 110]
    assert np.unique(z0[30:430]).size == 110
    g, m = run_pair(native, c, K, 0.5, 0.1, 3, z0=z0)
    assert np.unique(m.z[30:430]).size > 64                         # still more than one block after three sweeps
    assert m.stats[1] > 0
    g.close()


def test_one_document_of_33000_tokens(native, oracle):
    rng = np.random.default_rng(8)
    lens = np.array([5, 33000, 70], np.int64)
    tokens = rng.integers(0, 50, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 50)
    g, m = run_pair(native, c, 8, 0.1, 0.01, 2)
    n_d = g.get_doc_topic_counts(1, 2)
    assert n_d.sum() == 33000 > 32767 and n_d.max() > 2000          # past the lane kernels' int16 counts
    g.close()


@pytest.mark.parametrize("K,alpha,beta", [(20, 0.1, 0.01), (100, 5.0, 7.0)])
def test_debug_margin_sends_every_token_through_the_replay(native, oracle, cats, monkeypatch, K, alpha, beta):
    """GGS_DEBUG_MARGIN = 1e30 scales delta past every sum: no bucket is proven, every token takes the exact chains.  The run
    has the default's bits and the restatement's (run_pair compares every sweep)."""
    g0, _ = run_pair(native, cats, K, alpha, beta, 2)
    monkeypatch.setenv("GGS_DEBUG_MARGIN", "1e30")
    g1, _ = run_pair(native, cats, K, alpha, beta, 2)
    assert_bit_equal(g1.get_z(), g0.get_z(), "z under GGS_DEBUG_MARGIN")
    assert_bit_equal(g1.sparse_stats(), g0.sparse_stats(), "counters under GGS_DEBUG_MARGIN")
    g0.close()
    g1.close()


def test_one_cu_takes_every_workgroup_through_three_items(native, oracle, monkeypatch):
    """GGS_DEBUG_NUM_CUS=1 over 200 documents of 0 to 5 tokens at K = 8: the grid is at most 32 single-wave workgroups, so some
    workgroup takes at least 3 documents -- asserted from the launch info before anything is compared."""
    c = PG.short_corpus(200, 30, 77)
    monkeypatch.setenv(PG.KNOB, "1")
    g = native.GGSHandle(8, 30, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA | native.FLAG_PARANOID)
    g.set_corpus(c.doc_ptr, c.tokens)
    info = g.launch_info()
    assert info["z_kernel"].startswith(KERNEL) and info["num_chunks"] == c.num_docs == 200
    assert info["lds_bytes_z"] == lds_bytes(8, int(np.diff(c.doc_ptr).max()))
    PG.assert_trips(info["num_chunks"], 1, PG.CAP_WAVE, "adlda_wave_kernel")
    g.close()
    g, m = run_pair(native, c, 8, 0.1, 0.01, 3)
    g.close()


# ---- behind an exchange: bit-identical to one handle ----------------------------------------------------------------------
def shard_corpus_for(K):
    return random_corpus(120, 40, 50, seed=K, empty_every=7)


def reference_state(c, K, sweeps):
    m = R.Model(K, c.num_types, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, java_lcg_initial_z(c.num_tokens, K, 17))
    m.sweep(sweeps)
    return m


@pytest.mark.parametrize("K", [5, 65])
def test_null_exchange_of_one_rank_equals_one_handle(native, oracle, K):
    """ggs_attach_null_exchange(0, 1): every collective of the sweep runs (the count reduce-scatter, the gather of the count
    slices) and, with one rank, moves exactly what a real transport would."""
    c = shard_corpus_for(K)
    h = native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA)
    h.attach_null_exchange(0, 1)
    h.set_corpus(c.doc_ptr, c.tokens)
    h.set_global_token_count(c.num_tokens)
    h.set_z(java_lcg_initial_z(c.num_tokens, K, 17), redraw_phi=True)
    h.sweep(3)
    h.check_invariants()
    assert_state_equal(h, reference_state(c, K, 3), "behind the null exchange")
    h.close()


def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA)

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), lists=h.word_topic_lists(),
                    kernel=h.launch_info()["z_kernel"], stats=h.sparse_stats())
    return make_handle, body


@pytest.mark.parametrize("world,mode,K", [(2, "dense", 5), (3, "sparse", 65)])
def test_sharded_runs_equal_one_handle_and_the_restatement(native, oracle, world, mode, K):
    """Ranks as threads over the callback exchange, as tests/test_lightcollapsed_gpu.py shards.  (Either case takes 0.05 to
    0.2 s.  Whichever test of the session first uses torch on the device pays torch's start-up on top: 2 s in a fresh process,
    12 s measured behind this file's earlier tests -- start-up that the first torch user of another file paid before.)"""
    whole = shard_corpus_for(K)
    sweeps = 3
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    m = reference_state(whole, K, sweeps)
    assert_state_equal(h, m, "one handle")
    assert_bit_equal(np.concatenate([out[r]["z"] for r in range(world)]), h.get_z(), "z")
    assert_bit_equal(np.sum([out[r]["stats"] for r in range(world)], axis=0), h.sparse_stats(), "summed bucket counters")
    nw, lists = h.word_topic_lists()
    for r in range(world):
        assert out[r]["kernel"].startswith(KERNEL)
        assert_bit_equal(out[r]["nwk"], h.get_type_topic_counts(), "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], h.get_topic_totals(), "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], h.get_phi(), "the point estimate rank %d" % r)
        assert_bit_equal(out[r]["lists"][0], nw, "nw rank %d" % r)
        assert_bit_equal(out[r]["lists"][1], lists, "lists rank %d" % r)
    h.close()


def _gloo_rank(rank, world, port, out_dir, K, sweeps):
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as dist
    from ldagroupedgibbssampler_amd import native
    from ldagroupedgibbssampler_amd.sharded import ShardedGGS, gloo_callback_exchange
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    whole = shard_corpus_for(K)
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, device_id=0, flags=native.FLAG_ADLDA)
    sh = ShardedGGS(h, gloo_callback_exchange(rank, world), whole, rank, world)
    sh.set_z_global(java_lcg_initial_z(whole.num_tokens, K, 17))
    sh.sweep(sweeps)
    h.check_invariants()
    nw, lists = h.word_topic_lists()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), nw=nw, lists=lists,
             stats=h.sparse_stats())
    h.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("K", [5, 65])
def test_one_process_gloo_group_equals_the_restatement(oracle, tmp_path, K):
    """A real process group of one rank over gloo behind the callback exchange, in a child process of its own."""
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_gloo_rank, args=(1, port, str(tmp_path), K, 3), nprocs=1, join=True)
    p = np.load(os.path.join(str(tmp_path), "rank0.npz"))
    m = reference_state(shard_corpus_for(K), K, 3)
    nw, lists = m.lists()
    assert_bit_equal(p["z"], m.z.astype(np.int32), "z")
    assert_bit_equal(p["nwk"], m.counts(), "n_wk")
    assert_bit_equal(p["nk"], m.topic_totals(), "n_k")
    assert_bit_equal(p["nw"], nw, "nw")
    assert_bit_equal(p["lists"], lists, "lists")
    assert_bit_equal(p["stats"], m.stats, "bucket counters")


def test_one_process_device_group_equals_the_restatement(native, oracle):
    """ggs_group_create / ggs_group_set_z / ggs_group_sweep with the one device there is: the merge is the grouped gather of the
    count slices, as for scheme=collapsed."""
    K = 65
    c = shard_corpus_for(K)
    z0 = java_lcg_initial_z(c.num_tokens, K, 17)
    g = native.GGSGroup(K, c.num_types, 0.1, 0.01, SEED, device_ids=[0], flags=native.FLAG_ADLDA)
    h = g.handles[0]
    h.set_corpus(c.doc_ptr, c.tokens)
    g.set_z([z0], redraw_phi=True)
    g.sweep(3)
    g.gather_counts()
    assert_state_equal(h, reference_state(c, K, 3), "after the group's 3 sweeps")
    g.close()


# ---- statistics -----------------------------------------------------------------------------------------------------------
def heldout_after(native, flags, c, K, sweeps):
    h = native.GGSHandle(K, c.num_types, 0.1, 0.01, 4711, flags=flags)
    h.set_corpus(c.doc_ptr, c.tokens)
    h.init_z_java_lcg(4711)
    h.init_phi()
    h.sweep(sweeps)
    h.set_test_corpus(c.doc_ptr, c.tokens)
    v = h.heldout_log_likelihood(100)[0]
    h.close()
    return v


def test_heldout_likelihood_against_the_collapsed_parallel_schedule(native, cats):
    """After the same 200 sweeps on cats the left-to-right estimate lies within the project's 1 % of
    scheme=collapsed's parallel schedule.  The two chains have the same law (tests/test_adlda_model.py); they consume their
    uniforms differently, so this is a guard, not a measurement."""
    K = 20
    co = heldout_after(native, native.FLAG_COLLAPSED, cats, K, 200)
    ad = heldout_after(native, native.FLAG_ADLDA, cats, K, 200)
    gap = abs(ad - co) / abs(co)
    print("held-out log likelihood after 200 sweeps: collapsed (parallel schedule) %.2f, adlda %.2f, gap %.4f" % (co, ad, gap))
    assert gap < 0.01


# ---- the interface --------------------------------------------------------------------------------------------------------
def test_launch_info_z_form_and_sparse_stats(native, cats):
    import ctypes as C
    g = native.GGSHandle(20, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    assert (g.sparse_stats() == 0).all()
    zk, zf, zc = C.c_int32(), C.c_int32(), C.c_int32()
    assert g._L.ggs_get_z_form(g._h, C.byref(zk), C.byref(zf), C.byref(zc)) == 0
    assert zk.value == 11 and zf.value == 0
    info = g.launch_info()
    assert info["z_kernel"] == "adlda_wave_kernel (wave per document)" and info["num_chunks"] == cats.num_docs
    assert info["lds_bytes_z"] == lds_bytes(20, int(np.diff(cats.doc_ptr).max()))
    g.init_z_java_lcg(1)
    g.init_phi()
    g.reset_timings()
    g.sweep(3)
    s = g.sparse_stats()
    assert s.dtype == np.int64 and s[:3].sum() == 3 * cats.num_tokens and (s[:3] > 0).all()
    assert 3 * cats.num_tokens <= s[3] <= 3 * cats.num_tokens * 2 * 20   # 1 <= nnz_w, and nnz_w + nnz_d <= 2 K
    t = g.get_timings()
    assert t["sweeps"] == 3 and t["z_ms"] > 0
    g.set_corpus(cats.doc_ptr, cats.tokens)                         # cumulative since set_corpus
    assert (g.sparse_stats() == 0).all()
    g.close()


def test_paranoid_sweeps_the_split_sweep_and_the_diagnostics_as_collapsed(native, cats):
    """Paranoid whole sweeps and the two halves of a split one give the same z; the model log likelihood and the point estimate
    are those of a scheme=collapsed handle given the same z, bit for bit; the log posterior is refused by both, as
    scheme=collapsed refuses it; the held-out estimate runs."""
    K = 20
    g = native.GGSHandle(K, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA | native.FLAG_PARANOID)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    g.init_z_java_lcg(1)
    g.init_phi()
    g.sweep(2)
    g.check_invariants()
    g.sweep_begin()                                                 # the two halves are one sweep
    g.sweep_end()
    h = native.GGSHandle(K, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_ADLDA)
    h.set_corpus(cats.doc_ptr, cats.tokens)
    h.init_z_java_lcg(1)
    h.init_phi()
    h.sweep(3)
    assert_bit_equal(g.get_z(), h.get_z(), "z after 2 + 1 sweeps")
    co = native.GGSHandle(K, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_COLLAPSED)
    co.set_corpus(cats.doc_ptr, cats.tokens)
    co.set_z(g.get_z(), redraw_phi=True)
    assert g.model_log_likelihood() == co.model_log_likelihood()
    assert_bit_equal(g.get_phi(), co.get_phi(), "the point estimate")
    assert_bit_equal(g.get_type_topic_counts(), co.get_type_topic_counts(), "n_wk")
    for x in (g, h):                                                # the estimator's particles are drawn per iteration: the two handles at iteration 3
        x.set_test_corpus(cats.doc_ptr, cats.tokens)
    tg, dg = g.heldout_log_likelihood(10)
    th, dh = h.heldout_log_likelihood(10)
    assert tg == th and np.isfinite(tg) and tg < 0 and dg.size == cats.num_docs
    assert_bit_equal(dg, dh, "held-out per document")
    for x in (g, co):
        with pytest.raises(native.GGSError) as e:
            x.log_posterior()
        assert e.value.code == native.ERR_UNSUPPORTED
    for x in (g, h, co):
        x.close()


def test_unsupported_calls_and_misuse(native, cats):
    with pytest.raises(native.GGSError) as e:
        native.GGSHandle(4097, 10, 0.1, 0.01, 1, flags=native.FLAG_ADLDA)
    assert e.value.code == native.ERR_UNSUPPORTED
    g = native.GGSHandle(5, cats.num_types, 0.1, 0.01, 1, flags=native.FLAG_ADLDA)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    g.init_z_java_lcg(1)
    g.init_phi()
    for call, code in ((g.alias_tables, native.ERR_UNSUPPORTED), (g.mh_stats, native.ERR_UNSUPPORTED),
                       (lambda: g.sample_z_given_phi(1), native.ERR_UNSUPPORTED), (lambda: g.collapsed_serial_sweep(1, 1), native.ERR_STATE),
                       (lambda: g.set_phi(np.full((5, cats.num_types), 1.0 / cats.num_types)), native.ERR_UNSUPPORTED),
                       (g.get_theta, native.ERR_UNSUPPORTED)):
        with pytest.raises(native.GGSError) as e:
            call()
        assert e.value.code == code
    g.sweep(1)                                                      # the refusals left the handle usable
    assert g.sparse_stats()[:3].sum() == cats.num_tokens
    g.close()
    for flags in (native.FLAG_PCGS, native.FLAG_COLLAPSED):         # and the counters stay refused to the schemes without them
        h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=flags)
        with pytest.raises(native.GGSError) as e:
            h.sparse_stats()
        assert e.value.code == native.ERR_STATE
        h.close()


# ---- the host mirrors and the driver --------------------------------------------------------------------------------------
def test_host_mirror_end_to_end(native, cats):
    from ldagroupedgibbssampler_amd import sampler
    cfg = sampler.SimpleLDAConfiguration(scheme="adlda", topics=20, alpha=0.1, beta=0.01, iterations=5, seed=42, exec_time=None)
    m = sampler.ADLDA(cfg)
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(cats)
    m.sample(5)
    assert m.getCurrentIteration() == 5
    phi = np.asarray(m.getPhi())
    assert phi.shape == (20, cats.num_types) and not np.isnan(phi).any()
    assert np.allclose(phi.sum(axis=1), 1.0)
    n_wk = np.asarray(m.getTypeTopicMatrix())
    assert n_wk.sum() == cats.num_tokens
    assert m.getSparseStats()[:3].sum() == 5 * cats.num_tokens
    nw, lists = m.getWordTopicLists()
    _, _, want_nw, want_lists = R.head(n_wk, n_wk.sum(axis=0), 0.1, 0.01)
    assert_bit_equal(nw, want_nw, "nw of the model's counts")
    assert_bit_equal(lists, want_lists, "lists of the model's counts")
    with pytest.raises(NotImplementedError):
        m.getTheta()
    with pytest.raises(NotImplementedError):
        m.sampleZGivenPhi(1)


def test_cpp_mirror_end_to_end(native, tmp_path):
    """include/ggs_sampler.hpp with config_.adlda: the C++ mirror's z and topic totals are the handle's."""
    exe = os.path.join(ROOT, "examples", "ggs_host_demo")
    if not os.path.exists(exe):
        pytest.fail("examples/ggs_host_demo is not built: run __graft_entry__.build()")
    c = random_corpus(60, 90, 70, seed=12, empty_every=8)
    path = os.path.join(str(tmp_path), "corpus.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (c.num_docs, c.num_types))
        for d in range(c.num_docs):
            t = c.tokens[c.doc_ptr[d]:c.doc_ptr[d + 1]]
            f.write(" ".join([str(len(t))] + [str(int(x)) for x in t]) + "\n")
    K, alpha, beta, seed, its = 6, 0.5, 0.1, 99, 3
    logs = tmp_path / "logs"
    logs.mkdir()
    out = subprocess.run([exe, path, str(K), str(alpha), str(beta), str(seed), str(its), str(logs), "adlda"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    g = native.GGSHandle(K, c.num_types, alpha, beta, seed, flags=native.FLAG_ADLDA)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(seed)
    g.init_phi()
    g.sweep(its)
    assert lines["iteration"] == "%d hooks %d %d" % (its, its, its)
    assert np.array_equal(np.array(lines["z"].split(), np.int32), g.get_z())
    assert np.array_equal(np.array(lines["nk"].split(), np.int32), g.get_topic_totals())
    assert "logposterior" not in lines
    assert "z_3.csv" in os.listdir(logs)
    g.close()


def test_run_dataset_writes_the_driver_files(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--scheme", "adlda", "--topics", "5",
                        "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files
