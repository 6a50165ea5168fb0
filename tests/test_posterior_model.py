"""Are the CPU restatements LDA?  Every GPU parity test compares the device with a restatement (oracle/ for ggs, pcgs and
collapsed, tests/spalias_restatement.py for spalias); here the restatements' chains are compared with the one reference
that does not depend on anybody's restatement: the exact posterior p(z | w) of a corpus of 3^6 = 729 states
(tests/lda_posterior.py, fixture A), which all four exact schemes leave invariant.

The recipe (lda_posterior.run_chain / verdict): 50 burn-in sweeps, n = 4000 samples of the whole z vector, one every
`thin` sweeps (thin per scheme: the lag at which the samples are as good as independent -- ggs 8, pcgs / spalias 4,
serial collapsed 2), cells with an expected count below 5 pooled into one, Pearson chi-square.  Acceptance: p > 0.01 for
each of three fixed seeds -- the chains are deterministic (Philox, java.util.Random, seeded NumPy generators), so a case
passes or fails for good.  Power: every mutant of the NumPy reference sampler, at the n and thin of the scheme it
imitates, is rejected at p < 1e-4.
"""
import numpy as np
import pytest

from tests import lda_posterior as LP

N_SAMPLES, BURN_IN, THIN = LP.N_SAMPLES, LP.BURN_IN, LP.THIN
SEEDS = [1, 2, 3]
P_ACCEPT = 0.01
P_REJECT = 1e-4
Z_BAR = 4.5
A = LP.FIXTURE_A


@pytest.fixture(scope="module")
def post():
    return LP.enumerate_posterior(A.doc_ptr, A.tokens, A.K, A.V, A.alpha, A.beta)


# ---- the enumeration itself ---------------------------------------------------------------------------------------
def test_probabilities_sum_to_one(post):
    assert post.p.shape == (729,) and (post.p > 0).all()
    assert abs(post.p.sum() - 1.0) < 1e-12
    assert np.allclose(post.e_theta.sum(axis=1), 1.0, atol=1e-12) and np.allclose(post.e_phi.sum(axis=1), 1.0, atol=1e-12)
    # the one-token document's E[theta] is (alpha + p(z_5 = .)) / (1 + sum alpha)
    pz5 = np.array([post.p[post.states[:, 5] == k].sum() for k in range(3)])
    assert np.allclose(post.e_theta[2], (np.asarray(A.alpha) + pz5) / (1.0 + sum(A.alpha)), atol=1e-14)


def test_two_tokens_two_topics_by_hand():
    """One document, two tokens of two different words, K = 2, alpha = (a0, a1), beta = b, V = 2.  By hand, dropping what
    is common to all four states (Gamma(x + 1) = x Gamma(x)):
        z = (0, 0): n_d = (2, 0), topic 0 holds one token of each word   a0 (a0 + 1) * b b / ((2b) (2b + 1))
        z = (1, 1): the same with a1
        z = (0, 1), (1, 0): n_d = (1, 1), each topic holds one token     a0 a1 * b b / ((2b) (2b))"""
    a0, a1, b = 0.7, 2.5, 0.3
    w = np.array([a0 * (a0 + 1) * b * b / (2 * b * (2 * b + 1)), a0 * a1 * b * b / (2 * b * 2 * b), a0 * a1 * b * b / (2 * b * 2 * b),
                  a1 * (a1 + 1) * b * b / (2 * b * (2 * b + 1))])
    got = LP.enumerate_posterior([0, 2], [0, 1], 2, 2, [a0, a1], b)
    assert (got.states == [[0, 0], [0, 1], [1, 0], [1, 1]]).all()
    assert np.allclose(got.p, w / w.sum(), rtol=1e-13, atol=0)
    assert LP.state_index([1, 0], 2) == 2


def test_permuting_topics_with_alpha_permutes_the_probabilities(post):
    perm = np.array([2, 0, 1])                                      # new topic j is old topic perm[j]
    q = LP.enumerate_posterior(A.doc_ptr, A.tokens, A.K, A.V, np.asarray(A.alpha)[perm], A.beta)
    relabelled = LP.state_index(perm[q.states], A.K)                # the old-label index of every new-label state
    assert np.allclose(q.p, post.p[relabelled], rtol=1e-12, atol=0)
    assert np.allclose(q.e_theta, post.e_theta[:, perm], atol=1e-14) and np.allclose(q.e_phi, post.e_phi[perm], atol=1e-14)
    assert not np.allclose(q.p, post.p, rtol=1e-3)                  # alpha is asymmetric: the labels are not exchangeable


def test_enumeration_refuses_large_state_spaces():
    with pytest.raises(ValueError):
        LP.enumerate_posterior([0, 13], [0] * 13, 2, 1, 0.1, 0.1)   # 2^13 = 8192 states
    with pytest.raises(ValueError):
        LP.enumerate_posterior(A.doc_ptr, A.tokens, 200, A.V, LP.fixture_b(200).alpha, A.beta)


def test_verdict_pools_and_keeps_every_observation():
    p = np.array([0.5, 0.3, 0.1995, 0.0003, 0.0002])
    idx = np.repeat(np.arange(5), [5000, 3000, 1995, 3, 2])
    v = LP.verdict(idx, p)
    assert v.cells == 4 and v.dof == 3 and v.n == 10000 and v.chi2 < 1e-20 and v.pvalue == 1.0 and v.tv < 1e-15
    v = LP.verdict(np.repeat(np.arange(5), [5000, 3000, 1990, 3, 7]), p)   # 10 observations in the pooled cell against 5 expected
    assert abs(v.chi2 - (25.0 / 1995 + 25.0 / 5)) < 1e-9


def test_fixture_b_and_what_a_padded_topic_weighs():
    """Fixture B is fixture A with topics of alpha = 1e-12 behind the three real ones.  Its own state space is beyond the
    enumeration, so the weight of a padded topic is enumerated on a corpus that still fits (three tokens, two documents,
    one padded topic, 4^3 states): all states that use it together hold less than 1e-9."""
    b = LP.fixture_b(5)
    assert b.K == 5 and b.alpha[:3] == A.alpha and b.alpha[3:] == (1e-12, 1e-12)
    assert (b.V, b.beta, b.doc_ptr, b.tokens) == (A.V, A.beta, A.doc_ptr, A.tokens)
    q = LP.enumerate_posterior([0, 2, 3], [0, 1, 1], 4, 3, list(A.alpha) + [LP.PAD_ALPHA], A.beta)
    assert 0 < q.p[(q.states == 3).any(axis=1)].sum() < 1e-9


# ---- the chains ---------------------------------------------------------------------------------------------------
def reference_chain(scheme, seed, mutant=None, n=N_SAMPLES):
    s = LP.ReferenceSampler(A, scheme, seed, mutant)
    return LP.run_chain(s.sweep, s.get_z, A.K, n, THIN[scheme], BURN_IN)


def accept(post, idx, what, n=N_SAMPLES):
    v = LP.verdict(idx, post.p)
    print("%s: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (what, v.chi2, v.cells, v.pvalue, v.tv))
    assert v.n == n
    assert v.pvalue > P_ACCEPT, "%s is not a sampler of the LDA posterior: %r" % (what, v)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_numpy_reference_sampler_is_accepted(post, scheme, seed):
    accept(post, reference_chain(scheme, seed), "NumPy %s, seed %d" % (scheme, seed))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "collapsed"])
def test_oracle_chain_is_accepted(oracle, post, scheme, seed):
    accept(post, LP.oracle_chain(oracle, A, scheme, seed), "oracle %s, seed %d" % (scheme, seed))


@pytest.mark.parametrize("seed", SEEDS)
def test_spalias_restatement_is_accepted(oracle, post, seed):
    accept(post, LP.spalias_chain(oracle, A, seed), "spalias restatement, seed %d" % seed)


# ---- power --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", [m for m in LP.MUTANTS if m])
def test_every_mutant_is_rejected(post, mutant):
    """Each slip in the scheme it imitates (LP.MUTANT_SCHEME), at that scheme's n and thin.  Measured, seed 1: beta_double
    p = 8e-52, no_exclude 6e-20, alpha_reversed 0, walk_late 8e-06.  The same slips in the OTHER scheme's sampler:
    beta_double (pcgs) 7e-56, alpha_reversed (pcgs) 0, but walk_late (pcgs) p = 0.29 -- n = 4000 does not resolve it there;
    test_pcgs_late_walk_is_rejected_by_the_longer_chain does."""
    scheme = LP.MUTANT_SCHEME[mutant]
    v = LP.verdict(reference_chain(scheme, 1, mutant), post.p)
    print("NumPy %s mutant %s: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (scheme, mutant, v.chi2, v.cells, v.pvalue, v.tv))
    assert v.pvalue < P_REJECT, "the statistic does not see %s in %s: %r" % (mutant, scheme, v)


def test_pcgs_late_walk_is_rejected_by_the_longer_chain(post):
    """A walk that lands one topic late for 3 % of the tokens, in the pcgs conditional: the pcgs chain forgets a perturbed
    draw about twice as fast as the ggs chain (hence thin 4 against 8), the slip moves its stationary distribution half as
    far, and n = 4000 gives p = 0.29.  At LP.N_LONG = 12000 samples (292 cells) it is rejected: measured p = 6e-8 (0.006 at
    n = 8000).  So pcgs is ALSO accepted at that n below and on the device; for spalias and the serial collapsed chain,
    whose restatements are too slow for 48 000 sweeps in this suite or have no sampler with the slip here, a late walk
    of that size stays below what this file sees (their walks are pinned draw by draw against their restatements)."""
    v = LP.verdict(reference_chain("pcgs", 1, "walk_late", LP.N_LONG), post.p)
    print("NumPy pcgs mutant walk_late, n = %d: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (v.n, v.chi2, v.cells, v.pvalue, v.tv))
    assert v.n == LP.N_LONG and v.pvalue < P_REJECT, v


def test_numpy_pcgs_is_accepted_at_the_longer_n(post):
    accept(post, reference_chain("pcgs", 1, None, LP.N_LONG), "NumPy pcgs, seed 1, n = %d" % LP.N_LONG, LP.N_LONG)


@pytest.mark.parametrize("seed", SEEDS)
def test_oracle_pcgs_is_accepted_at_the_longer_n(oracle, post, seed):
    accept(post, LP.oracle_chain(oracle, A, "pcgs", seed, LP.N_LONG), "oracle pcgs, seed %d, n = %d" % (seed, LP.N_LONG), LP.N_LONG)


def test_parallel_collapsed_schedule_is_rejected(oracle, post):
    """scheme=collapsed's parallel schedule (ggs_sweep with GGS_FLAG_COLLAPSED, orc_collapsed_parallel_sweep) samples every
    document against the counts of the sweep's start, AD-LDA style (ADLDA.java:302-332): an approximate sampler by design,
    whose stationary distribution is NOT p(z | w) -- and with three documents that shows at once.  That is why it is not
    in the acceptance list above; its parity tests pin it to its own restatement, and its distance from the serial
    chain is bounded by the held-out likelihood test (tests/test_collapsed_gpu.py).  Measured here (seed 1, n = 4000, thin 2):
    chi2 = 1840 on 147 cells, total variation 0.32 (the exact chains above: chi2 125 ... 172, total variation 0.11 ... 0.12)."""
    v = LP.verdict(LP.oracle_chain(oracle, A, "collapsed_parallel", 1), post.p)
    print("oracle collapsed, parallel schedule: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (v.chi2, v.cells, v.pvalue, v.tv))
    assert v.pvalue < P_REJECT, v


def test_polyaurn_restatement_runs_and_stays_in_range(oracle, post):
    """scheme=polyaurn is not an exact sampler of this posterior (Phi is a Poisson-normalised Polya-urn draw, and a document
    of one token draws its topic uniformly: PolyaUrnSpaliasLDA.java:261-278), so nothing is asserted about its distribution.
    Recorded fact (seed 1, n = 4000, thin 4, default Poisson threshold): chi2 = 2539 on 147 cells, total variation
    0.39, against 125 ... 172 and 0.11 ... 0.12 for the exact chains above."""
    from tests import polyaurn_restatement as P
    z0 = oracle.jrandom_ints(1, A.K, len(A.tokens))
    m = P.Model(A.K, A.V, np.asarray(A.alpha), A.beta, 1, A.doc_ptr, A.tokens, z0)
    m.init_phi()
    seen = []

    def get_z():
        seen.append(m.z.copy())
        return m.z
    idx = LP.run_chain(m.sweep, get_z, A.K, N_SAMPLES, THIN["polyaurn"], BURN_IN)
    v = LP.verdict(idx, post.p)
    print("polyaurn restatement: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (v.chi2, v.cells, v.pvalue, v.tv))
    z = np.array(seen)
    assert z.shape == (N_SAMPLES, 6) and z.min() >= 0 and z.max() < A.K and v.n == N_SAMPLES


# ---- Rao-Blackwell means -------------------------------------------------------------------------------------------
BATCHES, PER_BATCH = 40, 500


def mean_scores(post, theta, phi):
    """max |z| over the D K + K V entries of the chain means of theta and phi against the enumerated expectations"""
    zt = LP.batch_means_z(theta, post.e_theta, BATCHES)
    zp = LP.batch_means_z(phi, post.e_phi, BATCHES)
    return max(np.abs(zt).max(), np.abs(zp).max())


def test_oracle_ggs_means_of_theta_and_phi(oracle, post):
    """E[theta_dk | w] = E[(n_dk + alpha_k) / (N_d + sum alpha)] and E[phi_kw | w] = E[(n_kw + beta) / (n_k + V beta)] over
    the enumerated posterior; the chain's theta and phi draws average to them.  40 batches of 500 sweeps, standard errors
    from the batch means; 18 entries, so |z| < 4.5 holds for a correct chain with probability 1 - 1e-4."""
    o = oracle.OracleSampler(A.K, A.V, np.asarray(A.alpha), A.beta, 1)
    o.set_corpus(A.doc_ptr, A.tokens)
    o.init_z_java_lcg(1)
    o.init_phi()
    o.sweep(BURN_IN)
    theta, phi = [], []
    for _ in range(BATCHES * PER_BATCH):
        o.sweep(1)
        theta.append(o.get_theta())
        phi.append(o.get_phi())
    worst = mean_scores(post, theta, phi)
    print("oracle ggs: max |z| of the theta / phi means = %.2f" % worst)
    assert worst < Z_BAR


def test_means_statistic_sees_a_doubled_beta(post):
    s = LP.ReferenceSampler(A, "ggs", 1, "beta_double")
    s.sweep(BURN_IN)
    theta, phi = [], []
    for _ in range(BATCHES * PER_BATCH):
        s.sweep(1)
        theta.append(s.theta)
        phi.append(s.phi)
    worst = mean_scores(post, theta, phi)
    print("NumPy ggs with beta doubled: max |z| of the theta / phi means = %.2f" % worst)
    assert worst > Z_BAR


def test_batch_means_z_on_known_numbers():
    bm = np.array([1.0, 3.0, 5.0, 7.0])                             # four batches of five equal samples each
    z = LP.batch_means_z(np.repeat(bm, 5).reshape(20, 1), [3.0], batches=4)
    assert np.allclose(z, (4.0 - 3.0) / (bm.std(ddof=1) / 2.0))
    assert np.allclose(LP.batch_means_z(bm.reshape(4, 1), [3.0], batches=4), z)
