"""scheme=polyaurn on the device (GGS_FLAG_POLYAURN): the Poisson layer, whole sweeps, the two uniform-draw rules and
sharded runs bit for bit against the CPU restatement (tests/polyaurn_restatement.py) or one handle; the held-out
likelihood against pcgs; the host mirror end to end; misuse."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, even_split, random_corpus, synthetic_lda_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import polyaurn_restatement as R
from tests.ranks import assert_bit_equal, run_ranks, z_kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777


@pytest.mark.parametrize("L", [1, 7, 100, 512])
@pytest.mark.parametrize("beta", [0.01, 0.5, 7.0])
def test_debug_poisson_equals_the_restatement(native, oracle, L, beta):
    rng = np.random.default_rng(L)
    counts = np.concatenate([np.repeat(np.arange(L), 40), np.full(200, L), rng.integers(L, 10 ** 6, 300), np.zeros(3000, np.int64)])
    for purpose, it, elem0 in ((R.PURPOSE_PHI, 3, 0), (R.PURPOSE_INIT_PHI, 0, 12345678901)):
        got = native.debug_poisson(counts, beta, L, SEED, it, purpose, elem0)
        want = R.poisson_draw(counts, beta, L, SEED, it, purpose, elem0)
        assert_bit_equal(got.astype(np.int64), want, "X (L=%d, beta=%g)" % (L, beta))


def run_pair(native, oracle, c, K, alpha, beta, sweeps, zseed=5, flags=0, burn_in=0, thin=1, L=0):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_POLYAURN | native.FLAG_PARANOID | flags,
                         phi_burn_in=burn_in, phi_mean_thin=thin, alias_poisson_threshold=L)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, L=L, save_phi_mean=bool(flags & native.FLAG_SAVE_PHI_MEAN),
                phi_burn_in=burn_in, phi_thin=thin)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
    n_kw = m.counts()
    assert_bit_equal(g.get_type_topic_counts(), n_kw.T.astype(np.int32), "n_wk")
    assert_bit_equal(g.get_topic_totals(), n_kw.sum(axis=1).astype(np.int32), "n_k")
    assert_bit_equal(g.get_phi(), m.phi, "phi")
    return g, m


@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, K, alpha, beta):
    g, m = run_pair(native, oracle, cats, K, alpha, beta, 4)
    assert z_kernel(g).startswith("pcgs_sliced")                                    # the lane-per-document kernel
    g.close()


def test_phi_mean_with_burn_in_and_thin(native, oracle, cats):
    g, m = run_pair(native, oracle, cats, 20, 0.1, 0.01, 6, flags=native.FLAG_SAVE_PHI_MEAN, burn_in=2, thin=2)
    mean, n = g.get_phi_mean()
    assert n == m.n_sampled == 2
    assert_bit_equal(mean, m.phi_mean(), "phi mean")
    g.close()


def test_sliced_kernel_with_empty_and_one_token_documents(native, oracle):
    c = random_corpus(300, 700, 60, seed=9, empty_every=7)
    lens = np.diff(c.doc_ptr)
    assert (lens == 0).any() and (lens == 1).any()
    g, m = run_pair(native, oracle, c, 100, 0.1, 0.01, 3, L=7)
    assert z_kernel(g).startswith("pcgs_sliced")
    g.close()


def test_wave_kernel_by_topics(native, oracle):
    c = random_corpus(150, 500, 50, seed=13, empty_every=5)
    g, m = run_pair(native, oracle, c, 200, 0.1, 0.01, 2)
    assert z_kernel(g).startswith("pcgs_wave")
    g.close()


def test_wave_kernel_by_document_length(native, oracle):
    rng = np.random.default_rng(3)
    lens = np.array([33000, 1, 40, 0, 7], np.int64)
    tokens = rng.integers(0, 300, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 300)
    g, m = run_pair(native, oracle, c, 30, 0.1, 0.01, 2)
    assert z_kernel(g).startswith("pcgs_wave")
    g.close()


def test_one_token_documents_draw_floor_u_k(native, oracle):
    K = 9
    c = Corpus(np.arange(41, dtype=np.int64), (np.arange(40) % 6).astype(np.int32), 6)   # 40 documents of one token
    g = native.GGSHandle(K, 6, 0.5, 0.1, SEED, flags=native.FLAG_POLYAURN)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(1)
    g.init_phi()
    g.sweep(1)
    U = oracle.uniforms(SEED, 1, R.PURPOSE_Z, 0, 40)
    assert_bit_equal(g.get_z(), np.minimum((U * K).astype(np.int32), K - 1), "z of one-token documents")
    g.close()


def test_zeroed_column_draws_floor_u_k_given_phi(native, oracle):
    c = random_corpus(80, 50, 30, seed=4)
    K = 12
    g = native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(2)
    g.init_phi()
    phi = g.get_phi()
    phi[:, 3] = 0.0                                               # word 3: an all-zero column
    phi[:, 5] = 0.0
    g.set_phi(phi)
    z = g.get_z().astype(np.int64)
    g.sample_z_given_phi(1)
    it = 1
    n = R.z_step(c.doc_ptr, c.tokens, z, phi, 0.1, SEED, it)
    assert n > 0
    assert_bit_equal(g.get_z(), z.astype(np.int32), "z given a phi with zero columns")
    U = oracle.uniforms(SEED, it, R.PURPOSE_Z, 0, c.num_tokens)
    hit = np.flatnonzero(np.isin(c.tokens, [3, 5]))
    assert hit.size and (g.get_z()[hit] == np.minimum((U[hit] * K).astype(np.int32), K - 1)).all()
    g.close()


def test_topic_without_tokens_gives_a_zero_row(native, oracle):
    c = random_corpus(60, 40, 20, seed=8)
    K = 6
    g = native.GGSHandle(K, c.num_types, 0.1, 1e-9, SEED, flags=native.FLAG_POLYAURN | native.FLAG_PARANOID)
    g.set_corpus(c.doc_ptr, c.tokens)
    z = np.zeros(c.num_tokens, np.int32)
    z[::2] = 1                                                    # topics 2..5 have no tokens
    g.set_z(z, redraw_phi=True)
    phi = g.get_phi()
    assert not np.isnan(phi).any()
    assert (phi[2:] == 0).all()
    g.check_invariants()
    g.sweep(2)
    assert not np.isnan(g.get_phi()).any()
    g.close()


# ---- sharded: bit-identical to one handle -------------------------------------------------------------------------
def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN | native.FLAG_SAVE_PHI_MEAN, phi_burn_in=1,
                                phi_mean_thin=2, alias_poisson_threshold=20)

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(),
                    how=h.count_exchange())
    return make_handle, body


def one_handle(native, whole, K, sweeps):
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN | native.FLAG_SAVE_PHI_MEAN, phi_burn_in=1, phi_mean_thin=2,
                         alias_poisson_threshold=20)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    r = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean())
    h.close()
    return r


@pytest.mark.parametrize("world,mode,K,V", [(2, "dense", 40, 900), (3, "dense", 100, 2100), (3, "sparse", 100, 900), (2, "sparse", 7, 1500)])
def test_sharded_runs_equal_one_handle(native, oracle, world, mode, K, V):
    whole = random_corpus(310, V, 90, seed=K + V, empty_every=9)
    sweeps = 5
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    ref = one_handle(native, whole, K, sweeps)
    bounds = even_split(whole.num_docs, world)
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert z.size == whole.num_tokens
    assert_bit_equal(z, ref["z"], "z")
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], ref["nk"], "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
    del bounds


def test_one_rank_through_rccl(native, oracle):
    whole = random_corpus(200, 600, 60, seed=31, empty_every=6)
    K = 24
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN | native.FLAG_SAVE_PHI_MEAN, phi_burn_in=1, phi_mean_thin=2,
                         alias_poisson_threshold=20)
    h.attach_rccl(0, 1, native.rccl_unique_id())
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(3)
    got = dict(z=h.get_z(), phi=h.get_phi(), nwk=h.get_type_topic_counts())
    h.close()
    ref = one_handle(native, whole, K, 3)
    for k in got:
        assert_bit_equal(got[k], ref[k], k)


# ---- statistics ---------------------------------------------------------------------------------------------------
def heldout_after(native, flags, train, test, K, sweeps):
    h = native.GGSHandle(K, train.num_types, 0.1, 0.01, 4711, flags=flags)
    h.set_corpus(train.doc_ptr, train.tokens)
    h.init_z_java_lcg(4711)
    h.init_phi()
    h.sweep(sweeps)
    h.set_test_corpus(test.doc_ptr, test.tokens)
    ll, _ = h.heldout_log_likelihood(100)
    r = dict(ll=ll, phi=h.get_phi(), nwk=h.get_type_topic_counts())
    h.close()
    return r


def test_heldout_likelihood_matches_pcgs_and_phi_has_the_expected_zeros(native):
    full = synthetic_lda_corpus(2200, 2000, 60, true_topics=20, seed=99)
    train, _, _ = full.shard(0, 2000)
    test, _, _ = full.shard(2000, 2200)
    K, sweeps = 20, 300
    pa = heldout_after(native, native.FLAG_POLYAURN, train, test, K, sweeps)
    pc = heldout_after(native, native.FLAG_PCGS, train, test, K, sweeps)
    gap = abs(pa["ll"] - pc["ll"]) / abs(pc["ll"])
    print("held-out log likelihood after %d sweeps: polyaurn %.2f, pcgs %.2f, gap %.4f" % (sweeps, pa["ll"], pc["ll"], gap))
    assert gap < 0.01
    # the zeros of the last Phi draw: P(Poisson(beta + n) = 0) = exp(-(beta + n)) per cell, on the counts it was drawn from
    lam = 0.01 + pa["nwk"].T.astype(np.float64)
    p0 = np.exp(-lam)
    want, sd = p0.sum(), np.sqrt((p0 * (1 - p0)).sum())
    got = float((pa["phi"] == 0).sum())
    print("exact zeros in phi: %d, expected %.1f +- %.1f" % (got, want, sd))
    assert abs(got - want) < 5 * sd + 1


# ---- the host mirror ----------------------------------------------------------------------------------------------
def test_host_mirror_end_to_end(native, cats):
    from ldagroupedgibbssampler_amd import sampler
    cfg = sampler.SimpleLDAConfiguration(scheme="polyaurn", topics=20, alpha=0.1, beta=0.01, iterations=5, seed=42, exec_time=None,
                                         alias_poisson_threshold=50)
    m = sampler.create_model(cfg)
    assert type(m) is sampler.PolyaUrnSpaliasLDA
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(cats)
    m.sample(5)
    assert m.getCurrentIteration() == 5
    phi = np.asarray(m.getPhi())
    assert phi.shape == (20, cats.num_types) and not np.isnan(phi).any()
    sums = phi.sum(axis=1)
    assert np.allclose(sums[sums > 0], 1.0)
    n_wk = np.asarray(m.getTypeTopicMatrix())
    assert n_wk.sum() == cats.num_tokens
    est = np.asarray(m.getThetaEstimate())
    assert est.shape == (cats.num_docs, 20)
    with pytest.raises(NotImplementedError):
        m.getTheta()


def test_run_dataset_writes_the_driver_files(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--scheme", "polyaurn", "--topics", "5",
                        "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files


# ---- misuse -------------------------------------------------------------------------------------------------------
def test_misuse_is_rejected(native):
    with pytest.raises(native.GGSError) as e:
        native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN | native.FLAG_COLLAPSED)
    assert e.value.code == native.ERR_BAD_ARG
    for bad in (513, -1):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN, alias_poisson_threshold=bad)
        assert e.value.code == native.ERR_BAD_ARG
    # 0 means 100; without the flag the field is not read
    native.GGSHandle(5, 10, 0.1, 0.01, 1, alias_poisson_threshold=513).close()
    counts = np.arange(0, 130, dtype=np.int32)
    assert_bit_equal(native.debug_poisson(counts, 0.5, 0, SEED, 1, R.PURPOSE_PHI, 0), native.debug_poisson(counts, 0.5, 100, SEED, 1, R.PURPOSE_PHI, 0),
                     "threshold 0 == 100")
    c = random_corpus(40, 30, 10, seed=1)
    hs = []
    for L in (0, 100):
        h = native.GGSHandle(6, c.num_types, 0.1, 0.01, 3, flags=native.FLAG_POLYAURN, alias_poisson_threshold=L)
        h.set_corpus(c.doc_ptr, c.tokens)
        h.init_z_java_lcg(3)
        h.init_phi()
        h.sweep(2)
        hs.append(h.get_phi())
        h.close()
    assert_bit_equal(hs[0], hs[1], "phi with threshold 0 and 100")
    with pytest.raises(native.GGSError):
        native.debug_poisson(np.array([-1], np.int32), 0.5, 10, SEED, 1, R.PURPOSE_PHI, 0)
