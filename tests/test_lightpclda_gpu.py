"""scheme=lightpclda on the device (GGS_FLAG_LIGHTPCLDA): whole sweeps, the z step on edge rows of Phi, sharded runs and
the posterior fixture bit for bit against the CPU restatement (tests/lightpclda_restatement.py) or one handle -- z, n_wk,
n_k, phi and the three Metropolis-Hastings counters; the held-out likelihood against pcgs; the driver and the host
mirrors end to end.

There is one z kernel, lightpc_wave_kernel (a wave per document), with one way through it: no margins, no replay."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus, synthetic_lda_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import lda_posterior as LP
from tests import lightpclda_knife_edge as KE
from tests import lightpclda_restatement as R
from tests.ranks import assert_bit_equal, run_ranks, z_kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777
KERNEL = "lightpc_wave_kernel"


def assert_state_equal(g, m, what=""):
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z " + what)
    assert_bit_equal(g.mh_stats(), m.stats, "MH counters " + what)


# ---- whole runs ---------------------------------------------------------------------------------------------------
def run_pair(native, c, K, alpha, beta, sweeps, zseed=5, flags=0, burn_in=0, thin=1):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_LIGHTPCLDA | native.FLAG_PARANOID | flags, phi_burn_in=burn_in,
                         phi_mean_thin=thin)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, save_phi_mean=bool(flags & native.FLAG_SAVE_PHI_MEAN),
                phi_burn_in=burn_in, phi_thin=thin)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_state_equal(g, m, "after sweep %d" % (s + 1))
    assert z_kernel(g).startswith(KERNEL)
    assert_bit_equal(g.get_type_topic_counts(), m.counts(), "n_wk")
    assert_bit_equal(g.get_topic_totals(), m.topic_totals(), "n_k")
    assert_bit_equal(g.get_phi(), m.phi, "phi")
    ps, a, tn = g.alias_tables()
    assert_bit_equal(tn, m.tables[2], "typeNorm after the last sweep")
    assert_bit_equal(a, m.tables[1], "a after the last sweep")
    assert_bit_equal(ps, m.tables[0], "ps after the last sweep")
    assert int(m.stats.sum()) == sweeps * c.num_tokens
    return g, m


@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, K, alpha, beta):
    g, m = run_pair(native, cats, K, alpha, beta, 5)
    assert (m.stats > 0).all()                                      # all three outcomes occur
    g.close()


def test_cats_with_asymmetric_alpha(native, oracle, cats):
    alpha = 0.02 + 0.07 * np.arange(20)                             # alpha[s] stands where alpha[t] belongs: a wrong index shows
    g, m = run_pair(native, cats, 20, alpha, 0.01, 5)
    g.close()


def test_phi_mean_with_burn_in_and_thin(native, oracle, cats):
    g, m = run_pair(native, cats, 20, 0.1, 0.01, 6, flags=native.FLAG_SAVE_PHI_MEAN, burn_in=2, thin=2)
    mean, n = g.get_phi_mean()
    wmean, wn = m.phi_mean()
    assert n == wn == 2
    assert_bit_equal(mean, wmean, "phi mean")
    g.close()


def test_ragged_corpus(native, oracle):
    """Documents of 0 and 1 tokens (the one-token document: (int)ui can only be 0 or the alpha branch), 63, 64 and 65 (chunk
    boundaries), 130, and 700 tokens over V = 5, where most (int)ui land inside the current chunk, in an earlier chunk or
    on the token itself -- counted: over the sweeps at least 20 tokens draw their document proposal from each of the
    token's own position, a later one, an earlier one of the same 64-token chunk, an earlier chunk and the alpha branch,
    both after an accepted word proposal and without (12 sweeps: the own position without an accepted word proposal, one
    token in about len + alphaSum of those, is what needs them)."""
    doc_ptr, tokens = KE.ragged_corpus()
    c = Corpus(doc_ptr, tokens, KE.RAGGED["V"])
    q = KE.RAGGED
    assert SEED == q["seed"]
    g, m = run_pair(native, c, q["K"], q["alpha"], q["beta"], q["sweeps"], zseed=q["zseed"])
    assert (m.stats > 0).all()
    g.close()
    walk = KE.ragged_model(java_lcg_initial_z(c.num_tokens, q["K"], q["zseed"]))
    counts = {}
    for _ in range(q["sweeps"]):
        z = KE.count_dt_sources(walk, counts)
        walk.sweep(1)
        assert (z == walk.z).all()
    assert (walk.z == m.z).all()                                    # the walk counted the chain the device was compared with
    print("document proposals by (source, after an accepted word proposal): %s" % sorted(counts.items()))
    for src in KE.RAGGED_SOURCES:
        for after in (False, True):
            assert counts.get((src, after), 0) >= 20, (src, after, counts)


@pytest.mark.parametrize("K", [1024, 4096])
def test_wide_topic_rows_on_a_small_vocabulary(native, oracle, K):
    c = random_corpus(40, 200, 150, seed=K, empty_every=11)
    g, m = run_pair(native, c, K, 0.05, 0.01, 2)
    g.close()


def test_one_document_of_33000_tokens(native, oracle):
    rng = np.random.default_rng(8)
    lens = np.array([5, 33000, 70], np.int64)
    tokens = rng.integers(0, 50, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 50)
    g, m = run_pair(native, c, 40, 0.1, 0.01, 2)
    g.close()


# ---- edges of the ratio -------------------------------------------------------------------------------------------
def test_ratio_edges_through_set_phi(native, oracle):
    """Phi set by hand, then z steps given it.  Constant columns: the ratios are exact rationals -- word ratios equal to
    1.0 wherever ni[t] == ni[s] (`pi_w > 1` is false there and U2 < 1 accepts), document ratios (alpha + n[s]) /
    (alpha + n[s] - 1), always above 1.  A column with phi[k][w] == 0 for half the topics: document ratios of 0, +inf and
    NaN.  A column that is 0 everywhere: the identity table (typeNorm == 0), every document ratio NaN."""
    K, V = 8, 6
    rng = np.random.default_rng(11)
    c = random_corpus(120, V, 40, seed=21, empty_every=13)
    phi = np.empty((K, V))
    phi[:, 0] = 0.25
    phi[:, 1] = 0.125
    phi[:, 2] = np.where(np.arange(K) % 2 == 0, 0.0, 0.25)
    phi[:, 3] = 0.0
    phi[:, 4] = np.where(np.arange(K) < 4, 0.0, rng.random(K))
    phi[:, 5] = rng.random(K)
    alpha = 0.5                                                     # 0.5 + n is exact: equal ratios are exactly 1.0
    g = native.GGSHandle(K, V, alpha, 0.1, SEED, flags=native.FLAG_LIGHTPCLDA)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(3)
    z0 = g.get_z()
    m = R.Model(K, V, alpha, 0.1, SEED, c.doc_ptr, c.tokens, z0)
    g.set_phi(phi)
    m.set_phi(phi)
    ps, a, tn = g.alias_tables()
    assert tn[3] == 0.0 and (a[3] == np.arange(K)).all() and (ps[3] == 1.0).all()
    assert_bit_equal(ps, m.tables[0], "ps")
    met = dict(word_one=0, doc_nan=0, doc_inf=0, doc_zero=0)
    for it in range(4):
        zb = m.z.copy()
        g.sample_z_given_phi(1)
        m.sample_z_given_phi(1)
        assert_state_equal(g, m, "after z step %d" % (it + 1))
        # how many ratios of this step were exactly 1.0, NaN, +inf or 0: the edges are really met
        for d in range(c.num_docs):
            b, e = int(c.doc_ptr[d]), int(c.doc_ptr[d + 1])
            zdoc, n = [int(k) for k in zb[b:e]], np.bincount(zb[b:e], minlength=K).tolist()
            for pos in range(e - b):
                det = {}
                w = int(c.tokens[b + pos])
                R.token_step(n, zdoc, pos, phi[:, w], np.full(K, alpha), R.alpha_sum(alpha, K), m.tables[0][w], m.tables[1][w],
                             R.token_uniforms(SEED, it + 1, b + pos), det)
                r = det.get("ratio")
                met["word_one"] += det.get("pi_w") == 1.0
                if r is not None:
                    met["doc_nan"] += bool(np.isnan(r))
                    met["doc_inf"] += bool(np.isinf(r))
                    met["doc_zero"] += r == 0.0
            assert zdoc == m.z[b:e].tolist()
    assert min(met.values()) >= 20, met
    assert z_kernel(g).startswith(KERNEL)
    g.close()


# ---- sharded: bit-identical to one handle -------------------------------------------------------------------------
FLAGS_SHARDED = dict(phi_burn_in=1, phi_mean_thin=2)


def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_LIGHTPCLDA | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(),
                    how=h.count_exchange(), tables=h.alias_tables(), kernel=z_kernel(h), mh=h.mh_stats())
    return make_handle, body


def one_handle(native, whole, K, sweeps):
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_LIGHTPCLDA | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    r = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), tables=h.alias_tables(),
             mh=h.mh_stats())
    h.close()
    return r


@pytest.mark.parametrize("world,mode,K,V", [(2, "dense", 40, 900), (3, "dense", 100, 2100), (3, "sparse", 100, 900), (2, "sparse", 7, 1500)])
def test_sharded_runs_equal_one_handle(native, oracle, world, mode, K, V):
    whole = random_corpus(310, V, 90, seed=K + V, empty_every=9)
    sweeps = 5
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    ref = one_handle(native, whole, K, sweeps)
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert z.size == whole.num_tokens
    assert_bit_equal(z, ref["z"], "z")
    assert_bit_equal(np.sum([out[r]["mh"] for r in range(world)], axis=0), ref["mh"], "summed MH counters")
    assert int(ref["mh"].sum()) == sweeps * whole.num_tokens
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        assert out[r]["kernel"].startswith(KERNEL)
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], ref["nk"], "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))


# ---- the posterior fixture ----------------------------------------------------------------------------------------
N_SAMPLES, THIN = 4000, 8


def test_posterior_fixture_a_equals_the_restatement(native, oracle):
    """Fixture A, K = 3, n = 4000, thin 8: the histogram of visited states is the restatement's from the same seed (the
    chain is approximate by design: no p-value, tests/test_lightpclda_model.py prints its distance)."""
    from oracle import oracle as O
    fx = LP.FIXTURE_A
    g = native.GGSHandle(fx.K, fx.V, np.asarray(fx.alpha), fx.beta, SEED, flags=native.FLAG_LIGHTPCLDA)
    g.set_corpus(np.asarray(fx.doc_ptr, np.int64), np.asarray(fx.tokens, np.int32))
    g.init_z_java_lcg(SEED)
    g.init_phi()
    got = LP.run_chain(g.sweep, g.get_z, fx.K, N_SAMPLES, THIN, LP.BURN_IN, max_topic=fx.K - 1)
    m = R.Model(fx.K, fx.V, np.asarray(fx.alpha), fx.beta, SEED, fx.doc_ptr, fx.tokens, O.jrandom_ints(SEED, fx.K, len(fx.tokens)))
    m.init_phi()
    want = LP.run_chain(m.sweep, lambda: m.z, fx.K, N_SAMPLES, THIN, LP.BURN_IN, max_topic=fx.K - 1)
    assert z_kernel(g).startswith(KERNEL)
    assert_bit_equal(g.mh_stats(), m.stats, "MH counters")
    g.close()
    assert (LP.histogram(got, 729) == LP.histogram(want, 729)).all()
    assert (got == want).all()


def test_posterior_fixture_b_at_1024_topics_equals_the_restatement(native, oracle):
    """Fixture B: the same corpus padded to K = 1024 by alpha = 1e-12, n = 4000, thin 8.  The CPU side is the restatement's
    z step over the Phi and the tables read from the device before every sweep (both are pinned to the oracle and to the
    spalias restatement by their own tests; the CPU Phi draw at K = 1024 alone needs a minute for this chain), compared
    after EVERY sweep; the visited states, as indices in base 1024, and hence their histogram, are identical.

    NOT asserted for this scheme: "a padded topic is never the final z".  The alpha branch proposes (int)(... * K), uniform
    over all 1024 topics, and the ratio carries alpha[s], never alpha[t]: for an empty padded topic t it is
    phi[t][w] / phi[s][w] * (alpha[s] + n[s]) / (alpha[s] + ni[s]), which does not see alpha[t] = 1e-12 at all, so padded
    topics are accepted (the count below shows how often).  This is the reference's asymmetric-alpha approximation."""
    fx = LP.fixture_b(1024)
    K = fx.K
    alpha = np.asarray(fx.alpha)
    doc_ptr, tokens = np.asarray(fx.doc_ptr, np.int64), np.asarray(fx.tokens, np.int32)
    g = native.GGSHandle(K, fx.V, alpha, fx.beta, SEED, flags=native.FLAG_LIGHTPCLDA)
    g.set_corpus(doc_ptr, tokens)
    g.init_z_java_lcg(SEED)
    g.init_phi()
    z = g.get_z().astype(np.int64)
    stats = np.zeros(3, np.int64)
    it = [0]

    def step(n):
        for _ in range(n):
            it[0] += 1
            stats[:] += R.z_step(doc_ptr, tokens, z, g.get_phi(), alpha, g.alias_tables(), SEED, it[0])
            g.sweep(1)
            assert (g.get_z() == z).all(), "z after sweep %d" % it[0]

    got = LP.run_chain(step, lambda: z, K, N_SAMPLES, THIN, LP.BURN_IN)
    assert z_kernel(g).startswith(KERNEL)
    assert_bit_equal(g.mh_stats(), stats, "MH counters")
    g.close()
    padded = int((got % K > 2).sum())                               # samples whose last token sits on a padded topic
    print("fixture B at K = 1024: %d of %d samples end on a padded topic; MH counters %s" % (padded, N_SAMPLES, stats.tolist()))
    assert got.min() >= 0


# ---- statistics ---------------------------------------------------------------------------------------------------
def heldout_after(native, flags, train, test, K, sweeps):
    h = native.GGSHandle(K, train.num_types, 0.1, 0.01, 4711, flags=flags)
    h.set_corpus(train.doc_ptr, train.tokens)
    h.init_z_java_lcg(4711)
    h.init_phi()
    out = []
    done = 0
    for s in sweeps:
        h.sweep(s - done)
        done = s
        h.set_test_corpus(test.doc_ptr, test.tokens)
        out.append(h.heldout_log_likelihood(100)[0])
    h.close()
    return out


def test_heldout_likelihood_against_pcgs(native):
    """The recipe of test_spalias_gpu.py::test_heldout_likelihood_matches_pcgs: pcgs after its 300 sweeps, lightpclda after
    S sweeps within the project's 1 %.  An MH chain moves less per sweep, so the gaps at S = 300, 600 and
    1200 are printed (they belong in DESIGN.md 6d, which names them as not yet measured) and the bar is asserted at
    S = 1200, the largest of the three."""
    full = synthetic_lda_corpus(2200, 2000, 60, true_topics=20, seed=99)
    train, _, _ = full.shard(0, 2000)
    test, _, _ = full.shard(2000, 2200)
    K = 20
    pc = heldout_after(native, native.FLAG_PCGS, train, test, K, [300])[0]
    lp = heldout_after(native, native.FLAG_LIGHTPCLDA, train, test, K, [300, 600, 1200])
    gaps = [abs(v - pc) / abs(pc) for v in lp]
    print("held-out log likelihood: pcgs after 300 sweeps %.2f; lightpclda after 300 / 600 / 1200 sweeps %s, gaps %s"
          % (pc, ["%.2f" % v for v in lp], ["%.4f" % x for x in gaps]))
    assert gaps[-1] < 0.01


# ---- the interface ------------------------------------------------------------------------------------------------
def test_launch_info_z_form_and_mh_stats(native, cats):
    import ctypes as C
    g = native.GGSHandle(20, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_LIGHTPCLDA)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    assert (g.mh_stats() == 0).all()
    zk, zf, zc = C.c_int32(), C.c_int32(), C.c_int32()
    assert g._L.ggs_get_z_form(g._h, C.byref(zk), C.byref(zf), C.byref(zc)) == 0
    assert zk.value == 7 and zf.value == 0
    assert g.launch_info()["z_kernel"] == "lightpc_wave_kernel (wave per document)"
    g.init_z_java_lcg(1)
    g.init_phi()
    g.sweep(3)
    s = g.mh_stats()
    assert s.dtype == np.int64 and s.sum() == 3 * cats.num_tokens and (s > 0).all()
    g.set_corpus(cats.doc_ptr, cats.tokens)                         # cumulative since set_corpus
    assert (g.mh_stats() == 0).all()
    g.close()


def test_misuse_is_rejected(native):
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_LIGHTPCLDA | other)
        assert e.value.code == native.ERR_BAD_ARG
    for flags in (native.FLAG_PCGS, native.FLAG_SPALIAS):
        h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=flags)
        with pytest.raises(native.GGSError) as e:
            h.mh_stats()
        assert e.value.code == native.ERR_STATE
        h.close()


# ---- the host mirrors and the driver ------------------------------------------------------------------------------
def test_host_mirror_end_to_end(native, cats):
    from ldagroupedgibbssampler_amd import sampler
    from tests import spalias_restatement as SR
    cfg = sampler.SimpleLDAConfiguration(scheme="lightpclda", topics=20, alpha=0.1, beta=0.01, iterations=5, seed=42, exec_time=None)
    m = sampler.create_model(cfg, "lightpclda")
    assert type(m) is sampler.LightPCLDA
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(cats)
    m.sample(5)
    assert m.getCurrentIteration() == 5
    phi = np.asarray(m.getPhi())
    assert phi.shape == (20, cats.num_types) and not np.isnan(phi).any()
    assert np.allclose(phi.sum(axis=1), 1.0)
    assert np.asarray(m.getTypeTopicMatrix()).sum() == cats.num_tokens
    assert m.getMHStats().sum() == 5 * cats.num_tokens
    ps, a, tn = m.getAliasTables()
    assert_bit_equal(tn, SR.alias_tables(phi, 0.1)[2], "typeNorm of the model's Phi")
    with pytest.raises(NotImplementedError):
        m.getTheta()


def test_cpp_mirror_end_to_end(native, tmp_path):
    """include/ggs_sampler.hpp with config_.lightpclda: the C++ mirror's z and topic totals are the handle's."""
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
    out = subprocess.run([exe, path, str(K), str(alpha), str(beta), str(seed), str(its), str(logs), "lightpclda"], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    g = native.GGSHandle(K, c.num_types, alpha, beta, seed, flags=native.FLAG_LIGHTPCLDA)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(seed)
    g.init_phi()
    g.sweep(its)
    assert lines["iteration"] == "%d hooks %d %d" % (its, its, its)
    assert np.array_equal(np.array(lines["z"].split(), np.int32), g.get_z())
    assert np.array_equal(np.array(lines["nk"].split(), np.int32), g.get_topic_totals())
    assert "z_3.csv" in os.listdir(logs)
    g.close()


def test_run_dataset_writes_the_driver_files(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--scheme", "lightpclda", "--topics", "5",
                        "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files
