"""The held-out estimator's restatement (oracle/ggs_oracle.c:left_to_right) against the model: the enumerated
sequential-proposal limit of tests/heldout_model.py, with the estimator's own variance and second-order bias from the same
enumeration -- no measured tolerance.  What tests/test_heldout.py cannot see (everything that happens from the third token
on: the topic-beta bucket, the sorted localTopicIndex, the update of cachedCoefficients, topicBetaMass around a draw,
tokensSoFar beyond 1) moves the limit, and a slip there that the oracle and the kernel share fails here.

The mutants show the statistic's power at the same R and P (their measured values are in DESIGN section 2)."""
import numpy as np
import pytest

from tests import heldout_model as HM


@pytest.fixture(scope="module")
def limits():
    n_wk, n_k = HM.train_counts()
    return [HM.limit(doc, n_wk, n_k, HM.ALPHA, HM.BETA) for doc in HM.DOCS]


def oracle_on_fixture(O, seed, num_topics=HM.K, threads=8):
    """an oracle with the fixture's counts (set_z of the fixed z: nothing is swept)"""
    ptr, tok, z = HM.train_corpus()
    o = O.OracleSampler(num_topics, HM.V, HM.padded_alpha(num_topics), HM.BETA, seed, threads=threads)
    o.set_corpus(ptr, tok)
    o.set_z(z, redraw_phi=False)
    n_wk, n_k = HM.train_counts(num_topics)
    assert np.array_equal(o.get_type_topic_counts(), n_wk) and np.array_equal(o.get_topic_totals(), n_k)
    return o


# ---------------------------------------------------------------- the enumeration itself
def _phi_hat():
    n_wk, n_k = HM.train_counts()
    return (HM.BETA + n_wk) / (n_k + HM.BETA * HM.V)                     # [V][K]


def test_limit_of_one_token_is_the_closed_form():
    """tests/test_heldout.py::test_one_token_documents_are_exact's form, alpha asymmetric"""
    n_wk, n_k = HM.train_counts()
    alpha, phi = np.asarray(HM.ALPHA), _phi_hat()
    for w in range(HM.V):
        lim = HM.limit([w], n_wk, n_k, HM.ALPHA, HM.BETA)
        want = np.log((alpha * phi[w]).sum() / alpha.sum())
        assert abs(lim.log_e - want) <= 1e-13 * abs(want)
        assert lim.var_g <= 1e-28 and abs(lim.bias) <= 1e-28 and lim.var[0] <= 1e-28     # one token: exact whatever is drawn


def test_limit_of_two_tokens_is_the_exact_marginal():
    """tests/test_heldout.py::test_two_token_document_against_the_exact_marginal's form, alpha asymmetric: for two tokens
    the limit IS log p(w1, w2)"""
    n_wk, n_k = HM.train_counts()
    alpha, phi = np.asarray(HM.ALPHA), _phi_hat()
    for w1 in range(HM.V):
        for w2 in range(HM.V):
            p1k = alpha * phi[w1]
            p1 = p1k.sum() / alpha.sum()
            post = p1k / p1k.sum()
            p2 = sum(post[z1] * sum((alpha[z2] + (z1 == z2)) / (alpha.sum() + 1) * phi[w2][z2] for z2 in range(HM.K)) for z1 in range(HM.K))
            lim = HM.limit([w1, w2], n_wk, n_k, HM.ALPHA, HM.BETA)
            want = np.log(p1 * p2)
            assert abs(lim.log_e - want) <= 1e-13 * abs(want), (w1, w2)


def test_limit_is_unchanged_by_a_permutation_of_the_topics(limits):
    n_wk, n_k = HM.train_counts()
    for perm in ([1, 2, 0], [2, 1, 0], [0, 2, 1]):
        for doc, lim in zip(HM.DOCS, limits):
            got = HM.limit(doc, n_wk[:, perm], n_k[perm], np.asarray(HM.ALPHA)[perm], HM.BETA)
            assert abs(got.log_e - lim.log_e) <= 1e-13 * abs(lim.log_e)
            assert abs(got.var_g - lim.var_g) <= 1e-12 * lim.var_g and abs(got.bias - lim.bias) <= 1e-12 * abs(lim.bias)
            np.testing.assert_allclose(got.e, lim.e, rtol=1e-13)
            np.testing.assert_allclose(got.var, lim.var, rtol=1e-12, atol=1e-30)


def test_limit_paths_sum_to_one_and_the_fixture_is_what_the_issue_asks(limits):
    for lim in limits:
        assert abs(lim.paths_q - 1.0) <= 1e-13
    lens = sorted(len(d) for d in HM.DOCS)
    assert len(HM.DOCS) >= 4 and lens[0] >= 3 and lens[-1] <= 6
    assert any(len(set(d)) < len(d) for d in HM.DOCS) and any(len(set(d)) == len(d) for d in HM.DOCS)
    # from the third token on the limit is not log p(w): the estimator is pinned to what it converges to, not to p(w)
    n_wk, n_k = HM.train_counts()
    assert HM.limit(HM.DOCS[0], n_wk, n_k, HM.ALPHA, HM.BETA).var[2] > 0


def test_padding_moves_the_limit_far_below_the_standard_error(limits):
    """Topics padded with alpha = 1e-12 (what the device tests use to reach the other instantiations) move sum log E_n by
    order K * 1e-12: bounded by HM.padding_bound, asserted on limit() with the padded smoothing mass; in the
    statistic's unit, |mean z| sqrt(R), that is at most 0.05 of the 4.5 allowed."""
    n_wk, n_k = HM.train_counts()
    for num_topics in (100, 1024, 2049):
        for doc, lim in zip(HM.DOCS, limits):
            on_paths, leaked = HM.padding_bound(doc, n_wk, n_k, HM.ALPHA, HM.BETA, num_topics - HM.K)
            padded = HM.limit(doc, n_wk, n_k, HM.ALPHA, HM.BETA, pad_topics=num_topics - HM.K, pad_alpha=HM.PAD_ALPHA)
            assert abs(padded.log_e - lim.log_e) <= on_paths + leaked
            assert 0.0 <= 1.0 - padded.paths_q <= len(doc) * (num_topics - HM.K) * HM.PAD_ALPHA / (HM.V * sum(HM.ALPHA) * _phi_hat().min())
            assert (on_paths + leaked) / np.sqrt(lim.var_g / HM.P) * np.sqrt(HM.R) <= 0.05      # of the 4.5 that |mean z| sqrt(R) is held to


# ---------------------------------------------------------------- accepted chains
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_model_sampler_is_accepted(limits, seed):
    n_wk, n_k = HM.train_counts()
    est, which = HM.ParticleSampler(n_wk, n_k, HM.ALPHA, HM.BETA, seed).run()
    stats = HM.statistics(est, which, limits, HM.P)
    print("clean sampler, seed %d: (|mean z| sqrt(R), mean z^2, max |z|) per document %s" % (seed, np.round(stats, 2).tolist()))
    assert HM.accepted(stats), stats


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_oracle_is_accepted(oracle, limits, seed):
    o = oracle_on_fixture(oracle, seed)
    ptr, tok, which = HM.heldout_corpus()
    total, ll = o.heldout_log_likelihood(ptr, tok, HM.P)
    o.close()
    stats = HM.statistics(ll, which, limits, HM.P)
    print("oracle, Philox seed %d: (|mean z| sqrt(R), mean z^2, max |z|) per document %s" % (seed, np.round(stats, 2).tolist()))
    assert HM.accepted(stats), stats


# ---------------------------------------------------------------- rejected mutants
@pytest.mark.parametrize("mutant", HM.MUTANTS)
def test_every_mutant_is_rejected(limits, mutant):
    n_wk, n_k = HM.train_counts()
    est, which = HM.ParticleSampler(n_wk, n_k, HM.ALPHA, HM.BETA, 1, mutant).run()
    stats = HM.statistics(est, which, limits, HM.P)
    print("mutant %s: (|mean z| sqrt(R), mean z^2, max |z|) per document %s" % (mutant, np.round(stats, 2).tolist()))
    assert HM.rejected(stats), stats
