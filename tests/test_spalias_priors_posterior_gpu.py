"""The device's spalias_priors chain against the scheme's enumerated stationary law (tests/lda_posterior.py, "the constrained
posterior"; the CPU side of the same check is tests/test_spalias_priors_posterior_model.py).  The recipe of every case, the
pattern of tests/test_posterior_gpu.py: a FLAG_SPALIAS | FLAG_PARANOID handle with the fixture's prior cells, started like the
parity tests start one (seeded z0, initial Phi), 50 burn-in sweeps, n = 4000 samples of the whole z vector one every 4 sweeps.
Then

  parity   the histogram of the visited states is IDENTICAL to the CPU restatement's from the same seed (K = 3 and K = 40; at
           K = 1024 the restatement is too slow);
  model    p > 0.01 against the law with the row masses m of the CPU ORACLE's unmasked initial Phi times P (the device's own
           initial Phi is asserted to be that matrix, bit for bit), p < 1e-4 for the same histogram against the law with
           m = 1, no sample off the support, no padded topic drawn, and the rows of the final Phi within LP.mass_bound of m.

Equal histograms that are rejected are a model bug shared by the restatement and the kernels; different histograms are a
parity bug.  Fixture: fixture A with the cells (topic 0, word 1) and (topic 2, word 2) masked; padded to K = 40 / 1024 by
alpha = 1e-12, a padded topic k masked at word k mod 3 (mask bits through K - 1, across the mask's 32-bit words).
"""
import functools
import time

import numpy as np
import pytest

from tests import lda_posterior as LP

pytestmark = pytest.mark.gpu

P_ACCEPT = 0.01
P_REJECT = 1e-4
Z_BAR = 4.5
A = LP.FIXTURE_A
N_SAMPLES, BURN_IN, THIN = LP.N_SAMPLES, LP.BURN_IN, LP.THIN["spalias_priors"]
SWEEPS = BURN_IN + N_SAMPLES * THIN
SPALIAS = "spalias_wave_kernel"
P3 = LP.prior_matrix(3, 3, LP.prior_cells(3))


def fixture(K):
    return A if K == A.K else LP.fixture_b(K)


@functools.lru_cache(maxsize=None)
def law(m):
    """the constrained law of fixture A under the two cells, masses m (a tuple of three, or 1.0)"""
    q = LP.enumerate_constrained_posterior(A, P3, m)
    q.p.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def reference(K, seed):
    """(m [K], phi0 * P [K][V]) of the CPU oracle: computed once per (K, seed), shared by the cases"""
    from oracle import oracle as O
    m, phi0 = LP.oracle_row_masses(O, fixture(K), LP.prior_cells(K), seed)
    m.setflags(write=False), phi0.setflags(write=False)
    return m, phi0


@functools.lru_cache(maxsize=None)
def cpu_histogram(K, seed):
    """the CPU restatement's histogram of visited states: computed once per (K, seed)"""
    from oracle import oracle as O
    idx, _ = LP.spalias_priors_chain(O, fixture(K), LP.prior_cells(K), seed, N_SAMPLES)
    h = LP.histogram(idx, 729)
    h.setflags(write=False)
    return h


def make_handle(native, monkeypatch, K, seed, margin=None, flags=0):
    fx = fixture(K)
    if margin is None:
        monkeypatch.delenv("GGS_DEBUG_MARGIN", raising=False)
    else:
        monkeypatch.setenv("GGS_DEBUG_MARGIN", margin)
    try:
        g = native.GGSHandle(fx.K, fx.V, np.asarray(fx.alpha), fx.beta, seed, flags=native.FLAG_SPALIAS | native.FLAG_PARANOID | flags,
                             phi_burn_in=BURN_IN)
    finally:
        monkeypatch.delenv("GGS_DEBUG_MARGIN", raising=False)       # ggs_create has read every knob
    g.set_corpus(fx.doc_ptr, np.asarray(fx.tokens, np.int32))
    g.set_topic_priors(*LP.prior_cells(K))
    g.init_z_java_lcg(seed)
    g.init_phi()
    m, phi0 = reference(K, seed)
    phi = g.get_phi()
    assert np.array_equal(phi.view(np.int64), phi0.view(np.int64)), "the initial Phi is not the oracle's times P, bit for bit"
    assert np.array_equal(g.get_topic_priors(), LP.prior_matrix(K, fx.V, LP.prior_cells(K)))
    assert g.launch_info()["z_kernel"].startswith(SPALIAS), g.launch_info()["z_kernel"]
    return g, m


DEVICE_HISTOGRAMS = {}                                              # (K, seed, margin) -> histogram, of the cases that have run


def device_chain(native, monkeypatch, K, seed, margin=None):
    """One whole case but the parity assertion: the chain, and every assertion against the model.  Returns the histogram."""
    g, m = make_handle(native, monkeypatch, K, seed, margin)
    t0 = time.perf_counter()
    idx = LP.run_chain(g.sweep, g.get_z, 3, N_SAMPLES, THIN, BURN_IN, max_topic=2)     # raises where a padded topic is drawn
    dt = time.perf_counter() - t0
    print("device chain: %d sweeps + %d get_z in %.2f s (%.0f us per sweep)" % (SWEEPS, N_SAMPLES, dt, 1e6 * dt / SWEEPS))
    g.check_invariants()
    phi = g.get_phi()
    g.close()
    what = "spalias_priors K=%d seed %d%s" % (K, seed, "" if margin is None else " GGS_DEBUG_MARGIN=" + margin)
    q, q1 = law(tuple(m[:3])), law(1.0)
    v, v1, off = LP.verdict(idx, q.p), LP.verdict(idx, q1.p), LP.off_support(idx, q.p)
    masked = LP.prior_matrix(K, 3, LP.prior_cells(K)) == 0.0
    drift = float((np.abs(LP.exact_row_sums(phi) - m) / m).max())
    print("%s, m = (%.3f, %.3f, %.3f): chi2 = %.1f on %d cells, p = %.3g, TV = %.4f; %d off the support; against m = 1: chi2 = %.1f, p = %.3g; "
          "rows drift by %.3g relative (bound %.3g)" % (what, m[0], m[1], m[2], v.chi2, v.cells, v.pvalue, v.tv, off, v1.chi2, v1.pvalue, drift,
                                                        LP.mass_bound(SWEEPS, A.V)))
    assert v.n == N_SAMPLES
    assert off == 0, "%s: %d samples on a masked (topic, word) cell" % (what, off)
    assert (phi[masked] == 0.0).all() and not np.signbit(phi[masked]).any()
    assert drift <= LP.mass_bound(SWEEPS, A.V), "%s: a row's mass moved by %.3g relative" % (what, drift)
    h = LP.histogram(idx, 729)
    DEVICE_HISTOGRAMS[(K, seed, margin)] = h
    assert v.pvalue > P_ACCEPT, "MODEL bug: %s is not a sampler of the constrained law (%r)" % (what, v)
    assert v1.pvalue < P_REJECT, "%s: the statistic does not tell m from 1 (%r)" % (what, v1)
    return h


def assert_parity(h, K, seed, what):
    ref = cpu_histogram(K, seed)
    same = bool(np.array_equal(h, ref))
    print("%s: histogram %s" % (what, "identical to the CPU chain's" if same else "DIFFERS from the CPU chain's"))
    assert same, "PARITY bug: %s visits other states than its CPU restatement from the same seed (%d of 729 cells differ)" % (what, int((h != ref).sum()))


@pytest.mark.parametrize("K,seed", [(3, 4), (3, 5), (40, 4)], ids=["A-seed4", "A-seed5", "B40"])
def test_chain_samples_the_constrained_law_and_equals_the_restatement(native, oracle, monkeypatch, K, seed):
    """K = 40: mask bits 3 ... 39 set, across the first 32-bit word of a word's mask row"""
    h = device_chain(native, monkeypatch, K, seed)
    assert_parity(h, K, seed, "spalias_priors K=%d seed %d" % (K, seed))


def test_every_token_replayed_gives_the_default_forms_histogram(native, oracle, monkeypatch):
    """GGS_DEBUG_MARGIN=1e30: every token goes through the z kernel's exact replay"""
    default = DEVICE_HISTOGRAMS.get((3, 4, None))
    if default is None:                                             # this test on its own
        default = device_chain(native, monkeypatch, 3, 4)
    h = device_chain(native, monkeypatch, 3, 4, margin="1e30")
    assert np.array_equal(h, default), "%d of 729 cells differ between the two forms" % int((h != default).sum())
    assert_parity(h, 3, 4, "spalias_priors K=3 seed 4, every token replayed")


def test_wide_rows_sample_the_constrained_law(native, oracle, monkeypatch):
    """K = 1024: the alias build with one chain per four words, mask rows of 32 words.  No CPU chain: the restatement needs
    minutes for it (as in test_posterior_gpu.py::test_spalias)."""
    device_chain(native, monkeypatch, 1024, 4)


def test_device_side_means_of_phi(native, oracle, monkeypatch):
    """GGS_FLAG_SAVE_PHI_MEAN under the existing gating (phi_burn_in = 50): the running mean the conditional normalise kernel
    keeps, read every 500 sweeps and differenced into 40 batch means, against the enumerated
    E[m_k (n_kv + beta) / (n_k + |A_k| beta)] over the seven allowed cells; the masked cells of the mean are +0.0 exactly."""
    batches, per = 40, 500
    g, m = make_handle(native, monkeypatch, 3, 4, flags=native.FLAG_SAVE_PHI_MEAN)
    g.sweep(BURN_IN)                                                # the phi mean starts behind phi_burn_in = BURN_IN
    assert g.get_phi_mean()[1] == 0
    bm, before = [], np.zeros((A.K, A.V))
    for b in range(batches):
        g.sweep(per)
        mean, n = g.get_phi_mean()
        assert n == (b + 1) * per
        assert (mean[P3 == 0.0] == 0.0).all() and not np.signbit(mean[P3 == 0.0]).any()
        bm.append((mean * n - before) / per)
        before = mean * n
    g.close()
    allowed = P3 != 0.0
    bm = np.asarray(bm)
    z = LP.batch_means_z(bm[:, allowed], law(tuple(m)).e_phi[allowed], batches)
    z1 = LP.batch_means_z(bm[:, allowed], law(1.0).e_phi[allowed], batches)
    print("device spalias_priors, m = %s: max |z| of the phi means %.2f; against the expectation with m = 1: %.2f" % (
        np.round(m, 3), np.abs(z).max(), np.abs(z1).max()))
    assert np.abs(z).max() < Z_BAR, z
