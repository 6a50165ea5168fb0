"""The hyperparameter step without a device: the two host entry points of the library (ggs_learn_parameters,
ggs_learn_symmetric_concentration) against the plain-Python restatement of their specification, bit for bit; a case computable by
hand; the estimators' defining property (they climb the Dirichlet-multinomial likelihood) instead of a tolerance; the configuration
keys and the reference's `interval > 1` rule."""
import math

import numpy as np
import pytest

from tests import hyperparameter_restatement as R
from tests.ranks import assert_bit_equal


# Histograms of random DOCUMENTS (Dirichlet-multinomial draws), not of random numbers: bins that no corpus could produce send the
# fixed points to 0 or infinity, where Python raises (1 / 0.0) what IEEE arithmetic answers with inf.
DOC_LENGTHS = {2: [0, 1, 1, 1], 21: [0, 1, 3, 20, 20], 22: [21, 21, 2], 500: [0, 1, 21, 21, 42, 63, 83, 83, 104, 124, 300, 499]}   # n_bins - 1 is the longest


def _documents(rng, K, n_bins, copies=6, empty_topic=None):
    """n_dk [D][K] of `copies` documents per length of DOC_LENGTHS[n_bins], optionally with one topic that no document uses"""
    lens = np.repeat(DOC_LENGTHS[n_bins], copies)
    theta = rng.dirichlet(np.full(K, 0.4), lens.size)
    n_dk = np.stack([rng.multinomial(n, t) for n, t in zip(lens, theta)])
    if empty_topic is not None:
        n_dk[:, (empty_topic + 1) % K] += n_dk[:, empty_topic]
        n_dk[:, empty_topic] = 0
    assert int(n_dk.sum(1).max()) == n_bins - 1
    return n_dk


def _hists_of(n_dk, n_bins):
    lengths = np.bincount(n_dk.sum(1), minlength=n_bins).astype(np.int32)
    obs = np.stack([np.bincount(n_dk[:, k], minlength=n_bins) for k in range(n_dk.shape[1])]).astype(np.int32)
    return obs, lengths


@pytest.mark.parametrize("K", [1, 3, 64])
@pytest.mark.parametrize("n_bins", [2, 21, 22, 500])
def test_learn_parameters_is_the_restatement(native, K, n_bins):
    rng = np.random.default_rng(1000 * K + n_bins)
    obs, lengths = _hists_of(_documents(rng, K, n_bins, empty_topic=K // 2 if K > 1 else None), n_bins)
    if K > 1:
        assert not obs[K // 2, 1:].any()                                        # an all-zero topic row beyond bin 0: nonZeroLimit = 0
        obs[K // 2, 0] = 0                                                      # ... and bin 0 emptied too: nonZeroLimit = -1 (no estimator reads bin 0)
    for iterations in (1, 3):
        start = rng.uniform(0.01, 3.0, K)
        want = [float(a) for a in start]
        want_sum = R.learn_parameters(want, obs, lengths, 1.001, 1.0, iterations)
        got = start.copy()
        got_sum = native.learn_parameters(got, obs, lengths, 1.001, 1.0, iterations)
        assert_bit_equal(got, np.asarray(want), "params K=%d n_bins=%d iterations=%d" % (K, n_bins, iterations))
        assert_bit_equal(np.float64(got_sum), np.float64(want_sum), "parametersSum")
    # other shape and scale, and a length histogram longer than the observations'
    lengths2 = np.concatenate([lengths, np.zeros(7, np.int32)])
    lengths2[-1] = 1
    want = [0.5] * K
    got = np.full(K, 0.5)
    assert_bit_equal(np.float64(native.learn_parameters(got, obs, lengths2, 2.5, 0.25, 2)), np.float64(R.learn_parameters(want, obs, lengths2, 2.5, 0.25, 2)), "sum")
    assert_bit_equal(got, np.asarray(want), "params, shape 2.5 scale 0.25")


# `current` through every branch of digamma: z < 1e-6 (current itself; current + len goes through the loop), the while loop alone
# (current < 9.5), and past 9.5 (no trip of the loop)
@pytest.mark.parametrize("current", [3e-7, 0.37, 5.0, 9.5, 12.25, 400.0])
@pytest.mark.parametrize("n_bins", [2, 21, 22, 500])
def test_learn_symmetric_concentration_is_the_restatement(native, current, n_bins):
    # DOC_LENGTHS[500] has gaps of exactly 20 (63 -> 83, 104 -> 124: summed term by term) and 21 (0 -> 21, 21 -> 42, 42 -> 63, 83 -> 104: the
    # digamma difference); [22] is the digamma branch from prev = 0, [21] the longest gap still summed term by term
    if n_bins == 500:
        gaps = set(np.diff(sorted(set(DOC_LENGTHS[500]))).tolist())
        assert {20, 21} <= gaps
    for dims in (1, 3, 64):
        rng = np.random.default_rng(100 * n_bins + dims)
        obs, lengths = _hists_of(_documents(rng, dims, n_bins), n_bins)
        count_hist = obs.sum(0).astype(np.int32)                                # every topic into one row (MSLDA:837-843)
        got = native.learn_symmetric_concentration(count_hist, lengths, dims, current)
        want = R.learn_symmetric_concentration(count_hist, lengths, dims, current)
        assert_bit_equal(np.float64(got), np.float64(want), "current=%r n_bins=%d dims=%d" % (current, n_bins, dims))


def test_digamma_branches_are_all_taken():
    """the three paths of the restated digamma differ, so the parametrisation above does reach them; values against the series' limit"""
    assert R.digamma(3e-7) == -0.5772156649015328606065121 - 1 / 3e-7
    assert abs(R.digamma(1.0) + 0.5772156649015329) < 1e-12                    # through the loop nine times
    assert abs(R.digamma(20.0) - (math.log(20.0) - 1 / 40.0 - 1 / 4800.0)) < 1e-6   # no trip of the loop
    assert abs(R.digamma(9.5) - (R.digamma(8.5) + 1 / 8.5)) < 1e-13             # the recurrence across the threshold


def test_every_document_of_length_one(native):
    """obs[k][1] = m_k documents whose one token has topic k: params[k] = old_k * (m_k / old_k + shape) / (D / sum - 1 / scale)"""
    m = np.array([7, 0, 12, 1], np.int32)
    old = np.array([0.3, 1.7, 0.05, 2.0])
    shape, scale = 1.001, 1.0
    D = int(m.sum())
    obs = np.zeros((4, 2), np.int32)
    obs[:, 1] = m
    lengths = np.array([0, D], np.int32)
    s = 0.0
    for a in old:
        s += float(a)
    # in the order the specification evaluates: dg = 1 / (sum + 1 - 1), denominator = D * dg - 1 / scale; dg = 1 / (old + 1 - 1), p = m * dg
    denominator = 0.0 + D * (0.0 + 1 / (s + 1 - 1)) - 1 / scale
    want = [float(a) * ((0.0 + int(mk) * (0.0 + 1 / (float(a) + 1 - 1))) + shape) / denominator if mk > 0 else float(a) * (0.0 + shape) / denominator
            for a, mk in zip(old, m)]
    got = old.copy()
    total = native.learn_parameters(got, obs, lengths, shape, scale, 1)
    assert_bit_equal(got, np.asarray(want), "params")
    t = 0.0
    for w in want:
        t += w
    assert_bit_equal(np.float64(total), np.float64(t), "parametersSum")
    # The closed form, evaluated in that order.  With parameters that are powers of two and a sum that is one, 1 / (old + 1 - 1) and
    # 1 / (sum + 1 - 1) are exact, so m * (1 / old) is m / old and D * (1 / sum) is D / sum to the bit: the hand computation IS the result.
    old2 = np.array([0.25, 0.25, 0.5, 1.0])
    s2 = 0.0
    for a in old2:
        s2 += float(a)
    assert s2 == 2.0
    closed = [float(a) * (int(mk) / float(a) + shape) / (D / s2 - 1 / scale) for a, mk in zip(old2, m)]
    got2 = old2.copy()
    native.learn_parameters(got2, obs, lengths, shape, scale, 1)
    assert_bit_equal(got2, np.asarray(closed), "params against old * (m / old + shape) / (D / sum - 1 / scale)")


def _dm_documents(rng, alpha, D, lo, hi):
    theta = rng.dirichlet(alpha, D)
    lens = rng.integers(lo, hi + 1, D)
    return np.stack([rng.multinomial(n, t) for n, t in zip(lens, theta)])


def _hists(n_dk):
    n_bins = int(n_dk.sum(1).max()) + 1
    lengths = np.bincount(n_dk.sum(1), minlength=n_bins).astype(np.int32)
    per_topic = np.stack([np.bincount(n_dk[:, k], minlength=n_bins) for k in range(n_dk.shape[1])]).astype(np.int32)
    return per_topic, lengths


def test_learn_parameters_climbs_the_likelihood(native):
    """Minka's fixed point: every iteration raises the Dirichlet-multinomial likelihood of the data (up to the rounding of its
    evaluation: n_terms * 2^-52 * |ll|).  30 single-iteration calls from a flat start, documents drawn from a known asymmetric alpha."""
    rng = np.random.default_rng(5)
    truth = np.array([0.05, 0.1, 0.2, 0.4, 0.8, 1.6, 0.3, 0.02])
    n_dk = _dm_documents(rng, truth, 600, 5, 60)
    obs, lengths = _hists(n_dk)
    alpha = np.full(truth.size, 1.0)
    ll0, n_terms = R.dm_log_likelihood(alpha, n_dk)
    prev = ll0
    for it in range(30):
        s = native.learn_parameters(alpha, obs, lengths, 1.001, 1.0, 1)
        assert (alpha > 0).all() and np.isfinite(alpha).all() and abs(s - alpha.sum()) <= 1e-12 * s
        ll, _ = R.dm_log_likelihood(alpha, n_dk)
        print("asymmetric iteration %d: ll %.17g (step %.3g, allowed -%.3g)" % (it + 1, ll, ll - prev, n_terms * 2.0 ** -52 * abs(prev)))
        assert ll >= prev - n_terms * 2.0 ** -52 * abs(prev), "iteration %d lowered the likelihood: %r -> %r" % (it + 1, prev, ll)
        prev = ll
    assert prev > ll0
    assert np.corrcoef(np.log(alpha), np.log(truth))[0, 1] > 0.95                # and it moved towards the alpha that made the data


def test_learn_symmetric_concentration_climbs_the_likelihood(native):
    rng = np.random.default_rng(6)
    K = 12
    n_dk = _dm_documents(rng, np.full(K, 0.3), 500, 5, 80)
    obs, lengths = _hists(n_dk)
    sym = obs.sum(0).astype(np.int32)                                           # every topic into one row (MSLDA:837-843)
    current = 50.0
    ll0, n_terms = R.dm_log_likelihood(np.full(K, current / K), n_dk)
    prev = ll0
    for it in range(30):
        current = native.learn_symmetric_concentration(sym, lengths, K, current)
        assert current > 0 and math.isfinite(current)
        ll, _ = R.dm_log_likelihood(np.full(K, current / K), n_dk)
        print("symmetric call %d: alphaSum %.17g ll %.17g (step %.3g)" % (it + 1, current, ll, ll - prev))
        assert ll >= prev - n_terms * 2.0 ** -52 * abs(prev), "call %d lowered the likelihood: %r -> %r" % (it + 1, prev, ll)
        prev = ll
    assert prev > ll0
    assert 0.2 < current / K < 0.45


def test_bad_arguments_are_refused(native):
    ok = np.ones(3, np.int32)
    L = native._lib.load()
    out = native.C.c_double()
    assert L.ggs_learn_symmetric_concentration(None, 3, native._ip(ok), 3, 2, 1.0, native.C.byref(out)) == native.ERR_BAD_ARG
    assert L.ggs_learn_symmetric_concentration(native._ip(ok), 0, native._ip(ok), 3, 2, 1.0, native.C.byref(out)) == native.ERR_BAD_ARG
    assert L.ggs_learn_symmetric_concentration(native._ip(ok), 3, native._ip(ok), 3, 0, 1.0, native.C.byref(out)) == native.ERR_BAD_ARG
    p = np.ones(1)
    assert L.ggs_learn_parameters(native._dp(p), 0, native._ip(ok), 3, native._ip(ok), 3, 1.0, 1.0, 1, native.C.byref(out)) == native.ERR_BAD_ARG
    assert L.ggs_learn_parameters(native._dp(p), 1, native._ip(ok), 3, native._ip(ok), 3, 1.0, 1.0, -1, native.C.byref(out)) == native.ERR_BAD_ARG
    with pytest.raises(ValueError):
        native.learn_parameters([1.0], ok[None, :], ok)                          # a list cannot be updated in place


# ---- configuration and the reference's rule ---------------------------------------------------------------------------------------
def test_configuration_keys_and_defaults():
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration
    c = SimpleLDAConfiguration()
    assert c.hyperparam_optim_interval == -1 and c.symmetric_alpha is False      # LDAConfiguration.java:46-47
    c = SimpleLDAConfiguration(hyperparam_optim_interval=25, symmetric_alpha=True)
    assert c.hyperparam_optim_interval == 25 and c.symmetric_alpha is True
    with pytest.raises(TypeError):
        SimpleLDAConfiguration(hyperparam_optim_intervall=2)


@pytest.mark.parametrize("interval", [-1, 0, 1])
def test_intervals_up_to_one_never_optimise(interval):
    """UPLDA:647,891: hyperparameterOptimizationInterval > 1 && iteration % interval == 0"""
    from ldagroupedgibbssampler_amd import sampler as S
    m = S.LDAGroupedGibbsSampler(S.SimpleLDAConfiguration(hyperparam_optim_interval=interval))
    assert not any(m.optimizes_at(it) for it in range(0, 50))


def test_interval_rule_and_the_classes_that_ignore_the_key():
    from ldagroupedgibbssampler_amd import sampler as S
    cfg = S.SimpleLDAConfiguration(hyperparam_optim_interval=3)
    for cls in (S.LDAGroupedGibbsSampler, S.LDAPartiallyCollapsedGibbsSampler, S.PolyaUrnSpaliasLDA, S.SpaliasUncollapsedParallelLDA, S.SpaliasUncollapsedParallelWithPriors,
                S.LightPCLDA, S.LightPCLDAtypeTopicProposal, S.PolyaUrnSparseLDA, S.NZVSSpaliasUncollapsedParallelLDA):
        assert [it for it in range(1, 10) if cls(cfg).optimizes_at(it)] == [3, 6, 9], cls.__name__
    for cls in (S.SerialCollapsedLDA, S.CollapsedLightLDA, S.ADLDA):             # as their Java classes: the key is not read
        assert not any(cls(cfg).optimizes_at(it) for it in range(1, 10)), cls.__name__


def test_restated_histograms_on_a_corpus_by_hand():
    doc_ptr = np.array([0, 0, 1, 4, 6], np.int64)
    z = np.array([2, 0, 0, 1, 1, 1], np.int32)
    sym = R.doc_topic_histogram(doc_ptr, z, 3, True, 4)
    asym = R.doc_topic_histogram(doc_ptr, z, 3, False, 4)
    assert asym.tolist() == [[3, 0, 1, 0], [2, 1, 1, 0], [3, 1, 0, 0]]           # the empty document counts n_dk == 0 for every topic
    assert sym.tolist() == [[8, 2, 2, 0]] and (asym.sum(0) == sym[0]).all()
    assert R.doc_length_counts(doc_ptr).tolist() == [1, 1, 1, 1]
    assert R.wrap_int32([2 ** 31 + 5]).tolist() == [-(2 ** 31) + 5]              # a Java int
