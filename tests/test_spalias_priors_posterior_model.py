"""Is the restatement of scheme=spalias_priors a sampler of the law it should sample?  The device is compared with
tests/spalias_priors_restatement.py bit for bit; here that restatement's chain is compared with the one reference that does not
depend on anybody's restatement: the scheme's exact stationary law on a corpus small enough to enumerate
(tests/lda_posterior.py, "the constrained posterior": fixture A, two masked cells, 144 of the 729 states in the support).

Every row of Phi keeps the mass m_k its allowed words had in the initial draw, so the law has m as a parameter; m is taken
from the CPU oracle's unmasked initial Phi (LP.oracle_row_masses), never from the chain that is judged.  The recipe is
lda_posterior.run_chain's (50 burn-in sweeps, n = 4000, thin 4, cells with an expected count below 5 pooled into one).
Acceptance: p > 0.01 against the law with the seed's own m, p < 1e-4 for the same histogram against the law with m = 1 (the
mass forgotten), no sample off the support.  The chains are deterministic: a case passes or fails for good.
"""
import functools

import numpy as np
import pytest

from tests import lda_posterior as LP

N_SAMPLES, BURN_IN, THIN = LP.N_SAMPLES, LP.BURN_IN, LP.THIN["spalias_priors"]
SWEEPS = BURN_IN + N_SAMPLES * THIN
P_ACCEPT = 0.01
P_REJECT = 1e-4
Z_BAR = 4.5
MIN_CELLS = 60
A = LP.FIXTURE_A
CELLS = LP.prior_cells(3)
P = LP.prior_matrix(3, 3, CELLS)
SAMPLER_M = (0.45, 1.0, 0.74)                                       # the NumPy sampler's masses: both masked rows far from 1, neither dead
RESTATEMENT_CASES = [(3, 4), (3, 5), (3, 6), (40, 4)]               # (K, seed): both masked rows keep a mass between 0.35 and 0.95


@functools.lru_cache(maxsize=None)
def law(m, cells=None, beta=A.beta):
    """the constrained law of fixture A (at another beta if given) under CELLS (or cells), masses m (a tuple, or 1.0)"""
    q = LP.enumerate_constrained_posterior(A._replace(beta=beta), P if cells is None else LP.prior_matrix(3, 3, cells), m)
    q.p.setflags(write=False)
    return q


# ---- the enumeration itself ---------------------------------------------------------------------------------------
def test_probabilities_sum_to_one_over_the_support():
    q = law(SAMPLER_M)
    assert q.p.shape == (729,) and abs(q.p.sum() - 1.0) < 1e-12
    on = np.array([all(P[k, w] != 0.0 for k, w in zip(z, A.tokens)) for z in q.states])
    assert on.sum() == 144 and (q.p[on] > 0).all() and (q.p[~on] == 0.0).all()
    assert (q.e_phi[P == 0.0] == 0.0).all() and np.allclose(q.e_phi.sum(axis=1), SAMPLER_M, rtol=1e-13, atol=0)
    assert np.allclose(q.e_theta.sum(axis=1), 1.0, atol=1e-12)


def test_without_a_mask_and_with_unit_masses_it_is_the_lda_posterior():
    want = LP.enumerate_posterior(A.doc_ptr, A.tokens, A.K, A.V, A.alpha, A.beta)
    got = LP.enumerate_constrained_posterior(A, np.ones((3, 3)), np.ones(3))
    assert np.abs(got.p - want.p).max() < 1e-13 and np.allclose(got.p, want.p, rtol=1e-11, atol=0)
    assert np.abs(got.e_phi - want.e_phi).max() < 1e-13 and np.abs(got.e_theta - want.e_theta).max() < 1e-13


def test_permuting_topics_with_alpha_masses_and_mask_rows_permutes_the_probabilities():
    perm = np.array([2, 0, 1])                                      # new topic j is old topic perm[j]
    old = law(SAMPLER_M)
    q = LP.enumerate_constrained_posterior(A._replace(alpha=tuple(np.asarray(A.alpha)[perm])), P[perm], np.asarray(SAMPLER_M)[perm])
    relabelled = LP.state_index(perm[q.states], A.K)                # the old-label index of every new-label state
    assert np.allclose(q.p, old.p[relabelled], rtol=1e-12, atol=0)
    assert np.allclose(q.e_theta, old.e_theta[:, perm], atol=1e-14) and np.allclose(q.e_phi, old.e_phi[perm], atol=1e-14)
    assert not np.allclose(q.p, old.p, rtol=1e-3, atol=1e-6)        # nothing here is exchangeable


def test_two_tokens_two_topics_one_masked_cell_by_hand():
    """One document, two tokens of words 0 and 1, K = 2, V = 2, alpha = (a0, a1), beta = b, the cell (topic 0, word 1) masked,
    m = (0.5, 1).  A_0 = {0}, A_1 = {0, 1}; the second token can only sit in topic 1.  Dropping what is common to all states
    (Gamma(x + 1) = x Gamma(x)), the word side of a topic relative to the empty topic is
        topic 0 holding the token of word 0:  0.5 * Gamma(1 + b) / Gamma(1 + b)                   = 0.5
        topic 1 holding one token:            b / (2b)                                            = 1 / 2
        topic 1 holding both:                 b b / ((2b) (2b + 1))
    so  z = (0, 1): a0 a1 * 0.5 * (1 / 2),   z = (1, 1): a1 (a1 + 1) * b b / ((2b) (2b + 1)),   z = (0, 0) and (1, 0): 0.
    psi_0 is the point mass on word 0, so E[phi_0] = (0.5, 0) whatever z is."""
    a0, a1, b = 0.7, 2.5, 0.3
    w = np.array([0.0, a0 * a1 * 0.5 * 0.5, 0.0, a1 * (a1 + 1) * b * b / (2 * b * (2 * b + 1))])
    fx = LP.Fixture(K=2, V=2, alpha=(a0, a1), beta=b, doc_ptr=(0, 2), tokens=(0, 1))
    got = LP.enumerate_constrained_posterior(fx, [[1, 0], [1, 1]], (0.5, 1.0))
    assert (got.states == [[0, 0], [0, 1], [1, 0], [1, 1]]).all()
    assert got.p[0] == 0.0 and got.p[2] == 0.0
    assert np.allclose(got.p, w / w.sum(), rtol=1e-13, atol=0)
    assert np.allclose(got.e_phi[0], [0.5, 0.0], rtol=1e-15, atol=0)
    p01, p11 = w[1] / w.sum(), w[3] / w.sum()
    assert np.allclose(got.e_phi[1], [p01 * b / (1 + 2 * b) + p11 * (1 + b) / (2 + 2 * b), p01 * (1 + b) / (1 + 2 * b) + p11 * (1 + b) / (2 + 2 * b)], rtol=1e-13)


def test_fixture_cells_are_a_list_the_library_accepts():
    """every topic keeps two allowed words and every word an allowed topic (what ggs_set_topic_priors checks), at every K used"""
    for K in (3, 40, 1024):
        t, w = LP.prior_cells(K)
        Pk = LP.prior_matrix(K, 3, (t, w))
        assert len(t) == K - 1 and (Pk.sum(axis=1) >= 2).all() and (Pk.sum(axis=0) >= 1).all()
        assert (Pk[:3] == P).all() and all(Pk[k, k % 3] == 0.0 for k in range(3, K))


# ---- the chains ---------------------------------------------------------------------------------------------------
def sampler_chain(seed, mutant=None):
    s = LP.ConstrainedSampler(A, P, SAMPLER_M, seed, mutant)
    return LP.run_chain(s.sweep, s.get_z, A.K, N_SAMPLES, THIN, BURN_IN)


def report(what, v, extra=""):
    print("%s: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f%s" % (what, v.chi2, v.cells, v.pvalue, v.tv, extra))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_numpy_constrained_sampler_is_accepted(seed):
    q = law(SAMPLER_M)
    idx = sampler_chain(seed)
    v = LP.verdict(idx, q.p)
    report("NumPy constrained sampler, seed %d" % seed, v)
    assert v.n == N_SAMPLES and LP.off_support(idx, q.p) == 0
    assert v.pvalue > P_ACCEPT, v


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("mutant", ["renormalised", "beta_double"])
def test_a_dropped_mass_and_a_doubled_beta_are_rejected(mutant, seed):
    v = LP.verdict(sampler_chain(seed, mutant), law(SAMPLER_M).p)
    report("NumPy constrained sampler, mutant %s, seed %d" % (mutant, seed), v)
    assert v.pvalue < P_REJECT, "the statistic does not see %s: %r" % (mutant, v)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_a_transposed_mask_leaves_the_support(seed):
    q = law(SAMPLER_M)
    idx = sampler_chain(seed, "mask_transposed")
    off = LP.off_support(idx, q.p)
    print("NumPy constrained sampler, mask transposed, seed %d: %d of %d samples off the support" % (seed, off, N_SAMPLES))
    assert off > 0


@functools.lru_cache(maxsize=None)
def restatement_case(K, seed):
    """(state indices, m [K], exact row sums of the model's Phi at the start / after the burn-in / at the end): one chain per
    case, shared by the tests below"""
    from oracle import oracle as O
    fx = A if K == A.K else LP.fixture_b(K)
    masses = []
    idx, m = LP.spalias_priors_chain(O, fx, LP.prior_cells(K), seed, N_SAMPLES, masses)
    for a in (idx, m) + tuple(masses):
        a.setflags(write=False)
    return idx, m, masses


@pytest.mark.parametrize("K,seed", RESTATEMENT_CASES)
def test_restatement_samples_the_constrained_law(oracle, K, seed):
    """run_chain raises if a padded topic is ever drawn (max_topic = 2), so at K = 40 the state is fixture A's"""
    idx, m, _ = restatement_case(K, seed)
    assert ((m[[0, 2]] > 0.35) & (m[[0, 2]] < 0.95)).all(), m[:3]   # a condition on the fixture's seeds
    q, q1 = law(tuple(m[:3])), law(1.0)
    v, v1, off = LP.verdict(idx, q.p), LP.verdict(idx, q1.p), LP.off_support(idx, q.p)
    report("spalias_priors restatement K=%d seed %d, m = (%.3f, %.3f, %.3f)" % (K, seed, m[0], m[1], m[2]), v,
           "; %d off the support; against m = 1: chi2 = %.1f, p = %.3g" % (off, v1.chi2, v1.pvalue))
    assert v.n == N_SAMPLES
    assert off == 0
    assert int((N_SAMPLES * q.p >= 5.0).sum()) >= MIN_CELLS          # a condition on the fixture: the chi-square has cells to speak with
    assert v.pvalue > P_ACCEPT, "the restatement is not a sampler of the constrained law: %r" % (v,)
    assert v1.pvalue < P_REJECT, "the statistic does not tell m from 1: %r" % (v1,)


@pytest.mark.parametrize("K,seed", RESTATEMENT_CASES)
def test_restatement_rows_keep_their_mass(oracle, K, seed):
    """m_k is a constant of the chain: the rows of Phi against the oracle's masses, relative, within LP.mass_bound
    (16 050 sweeps, V = 3: 8.9e-12; measured 2.4e-14 at most)"""
    _, m, (start, burnt, end) = restatement_case(K, seed)
    assert np.array_equal(start, m)                                 # the initial draw times P, exactly
    worst = [float((np.abs(x - m) / m).max()) for x in (burnt, end)]
    print("K=%d seed %d: rows drift by %.3g relative in %d sweeps (bound %.3g), by %.3g in %d (bound %.3g)" % (
        K, seed, worst[0], BURN_IN, LP.mass_bound(BURN_IN, A.V), worst[1], SWEEPS, LP.mass_bound(SWEEPS, A.V)))
    assert worst[0] <= LP.mass_bound(BURN_IN, A.V) and worst[1] <= LP.mass_bound(SWEEPS, A.V)


# ---- Rao-Blackwell means -------------------------------------------------------------------------------------------
BATCHES, PER_BATCH = 40, 500


def test_restatement_means_of_phi(oracle):
    """The restatement's Phi of every sweep, 40 batches of 500 sweeps, against the enumerated
    E[m_k (n_kv + beta) / (n_k + |A_k| beta)] over the allowed cells (the other mask: cells (0, 1) and (2, 0); seed 1).  Seven
    entries: |z| < 4.5 holds for a correct chain with probability 1 - 5e-5.  Against the expectation with m = 1 the same means
    are far off (measured |z| = 129)."""
    from tests import spalias_priors_restatement as PR
    cells = LP.prior_cells(3, LP.PRIOR_CELLS_RB)
    Prb = LP.prior_matrix(3, 3, cells)
    m, _ = LP.oracle_row_masses(oracle, A, cells, 1)
    mdl = PR.Model(A.K, A.V, np.asarray(A.alpha), A.beta, 1, A.doc_ptr, A.tokens, oracle.jrandom_ints(1, A.K, len(A.tokens)), cells=cells)
    mdl.init_phi()
    mdl.sweep(BURN_IN)
    phi = []
    for _ in range(BATCHES * PER_BATCH):
        mdl.sweep(1)
        phi.append(mdl.phi)
    phi = np.asarray(phi)
    assert (phi[:, Prb == 0.0] == 0.0).all()
    allowed = Prb != 0.0                                            # a masked cell is 0.0 in every sweep: no spread to score it by
    z = LP.batch_means_z(phi[:, allowed], law(tuple(m), LP.PRIOR_CELLS_RB).e_phi[allowed], BATCHES)
    z1 = LP.batch_means_z(phi[:, allowed], law(1.0, LP.PRIOR_CELLS_RB).e_phi[allowed], BATCHES)
    print("spalias_priors restatement, m = %s: max |z| of the phi means %.2f; against the expectation with m = 1: %.2f" % (
        np.round(m, 3), np.abs(z).max(), np.abs(z1).max()))
    assert np.abs(z).max() < Z_BAR, z
    assert np.abs(z1).max() > Z_BAR, z1


# ---- recorded, not asserted ----------------------------------------------------------------------------------------
def test_at_a_tiny_beta_the_clamp_moves_the_law_recorded(oracle):
    """beta = 0.001: about half of the gammas of an empty allowed cell are exactly 0 and become 1e-4 before they are summed
    (ConditionalDirichlet.java:90-92), so psi_k | z is no longer Dir(beta + n_k.) and the chain is not a sampler of the
    constrained law: approximate by design, the reference's design.  Nothing is asserted about its distribution.  Recorded
    (seed 4, n = 4000, thin 4): the figures are in DESIGN.md, section 2.  Asserted: states in range, and the same seed gives the
    same histogram."""
    fx = A._replace(beta=0.001)
    runs = [LP.spalias_priors_chain(oracle, fx, CELLS, 4) for _ in range(2)]
    (idx, m), (again, _) = runs
    q = law(tuple(m), beta=fx.beta)
    v = LP.verdict(idx, q.p)
    report("spalias_priors restatement at beta = 0.001, seed 4, m = %s" % np.round(m, 3), v, "; %d off the support" % LP.off_support(idx, q.p))
    assert idx.shape == (N_SAMPLES,) and idx.min() >= 0 and idx.max() < 729
    assert np.array_equal(LP.histogram(idx, 729), LP.histogram(again, 729))
