"""The hyperparameter step restated in plain Python, line for line from the specification in include/ggs_hip.h (MALLET 2.0.8's
Dirichlet.digamma, learnParameters and learnSymmetricConcentration as that header states them: the jar is in neither the reference
tree nor here), plus the numpy histograms of optimizeAlpha / optimizeBeta (MSLDA:812-905) that the device kernels are checked against.

Python floats are IEEE doubles and `a + b - c` groups left to right as Java and C++ do, so every function here is the specification
evaluated in its own order; math.log is the host libm's log, the one the library calls.  Nothing here needs a device."""
import math

import numpy as np


def digamma(z):
    if z < 1e-6:
        return -0.5772156649015328606065121 - 1 / z
    psi = 0.0
    while z < 9.5:
        psi -= 1 / z
        z += 1
    x = 1 / z
    y = x * x
    psi += math.log(z) - .5 * x - y * (1 / 12. - y * (1 / 120. - y * (1 / 252. - y * (1 / 240. - y * (1 / 132. - y * (691 / 32760. - y * (1 / 12.)))))))
    return psi


def learn_parameters(params, obs, obs_lengths, shape=1.001, scale=1.0, iterations=1):
    """params: a list of K floats, updated in place; obs: [K][n_bins] ints; returns parametersSum"""
    K = len(params)
    obs = [[int(v) for v in row] for row in obs]
    obs_lengths = [int(v) for v in obs_lengths]
    parametersSum = 0.0
    for k in range(K):
        parametersSum += params[k]
    nonZeroLimit = [-1] * K
    for k in range(K):
        for i in range(len(obs[k])):
            if obs[k][i] > 0:
                nonZeroLimit[k] = i
    for _ in range(iterations):
        denominator = 0.0
        dg = 0.0
        for i in range(1, len(obs_lengths)):
            dg += 1 / (parametersSum + i - 1)
            denominator += obs_lengths[i] * dg
        denominator -= 1 / scale
        parametersSum = 0.0
        for k in range(K):
            old = params[k]
            p = 0.0
            dg = 0.0
            for i in range(1, nonZeroLimit[k] + 1):
                dg += 1 / (old + i - 1)
                p += obs[k][i] * dg
            params[k] = old * (p + shape) / denominator
            parametersSum += params[k]
    return parametersSum


def learn_symmetric_concentration(count_hist, obs_lengths, num_dimensions, current):
    count_hist = [int(v) for v in count_hist]
    obs_lengths = [int(v) for v in obs_lengths]
    largest = 0
    for i in range(len(count_hist)):
        if count_hist[i] > 0:
            largest = i
    nz = [i for i in range(len(obs_lengths)) if obs_lengths[i] > 0]
    for _ in range(200):
        cp = current / num_dimensions
        dg = 0.0
        num = 0.0
        for i in range(1, largest + 1):
            dg += 1.0 / (cp + i - 1)
            num += count_hist[i] * dg
        dg = 0.0
        den = 0.0
        prev = 0
        cached = digamma(current)
        for length in nz:
            if length - prev > 20:
                dg = digamma(current + length) - cached
            else:
                for i in range(prev, length):
                    dg += 1.0 / (current + i)
            den += dg * obs_lengths[length]
            prev = length
        current = cp * num / den
    return current


# ---- the sufficient statistics, from host copies of the state ---------------------------------------------------------------------
def doc_topic_counts(doc_ptr, z, K):
    doc_of = np.repeat(np.arange(len(doc_ptr) - 1), np.diff(doc_ptr))
    n_dk = np.zeros((len(doc_ptr) - 1, K), np.int64)
    np.add.at(n_dk, (doc_of, np.asarray(z, np.int64)), 1)
    return n_dk


def wrap_int32(a):
    """bins are Java ints: modulo 2^32"""
    return (np.asarray(a, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def doc_topic_histogram(doc_ptr, z, K, symmetric, n_bins):
    """topicDocCounts (MSLDA:815-845): [K][n_bins], or [1][n_bins] with every topic in row 0; np.bincount per topic"""
    n_dk = doc_topic_counts(doc_ptr, z, K)
    assert n_dk.size == 0 or n_dk.max() < n_bins
    if symmetric:
        return wrap_int32(np.bincount(n_dk.ravel(), minlength=n_bins)[None, :])
    return wrap_int32(np.stack([np.bincount(n_dk[:, k], minlength=n_bins) for k in range(K)]))


def doc_length_counts(doc_ptr, n_bins=None):
    """docLengthCounts (UPLDA:377-432)"""
    lens = np.diff(doc_ptr)
    return np.bincount(lens, minlength=(int(lens.max()) + 1 if lens.size else 1) if n_bins is None else n_bins).astype(np.int32)


def cell_histogram(n_wk, n_bins):
    """countHistogram (MSLDA:867-880)"""
    return wrap_int32(np.bincount(np.asarray(n_wk).ravel(), minlength=n_bins))


def max_type_count(tokens, V):
    return int(np.bincount(tokens, minlength=V).max()) if len(tokens) else 0


def optimize(alpha, alpha_sum, beta_sum, symmetric, doc_ptr, tokens, V, z, n_wk, n_k):
    """One step (UPLDA:891-894) from host copies of the state: (alpha list, alphaSum, beta, betaSum), all by the restatement."""
    K = len(alpha)
    lengths = doc_length_counts(doc_ptr)
    hist = doc_topic_histogram(doc_ptr, z, K, symmetric, lengths.size)
    alpha = [float(a) for a in alpha]
    if symmetric:
        alpha_sum = learn_symmetric_concentration(hist[0], lengths, K, alpha_sum)
        alpha = [alpha_sum / K] * K
    else:
        alpha_sum = learn_parameters(alpha, hist, lengths, 1.001, 1.0, 1)
    count_hist = cell_histogram(n_wk, max_type_count(tokens, V) + 1)
    topic_size_hist = np.bincount(np.asarray(n_k), minlength=int(np.max(n_k)) + 1)
    beta_sum = learn_symmetric_concentration(count_hist, topic_size_hist, V, beta_sum)
    return alpha, alpha_sum, beta_sum / V, beta_sum


# ---- Dirichlet-multinomial log likelihoods (the property test) --------------------------------------------------------------------
def dm_log_likelihood(alpha, n_dk):
    """sum_d [lgamma(A) - lgamma(A + N_d) + sum_k (lgamma(alpha_k + n_dk) - lgamma(alpha_k))] and the number of gammaln terms summed"""
    from scipy.special import gammaln
    a = np.asarray(alpha, np.float64)
    n = np.asarray(n_dk, np.float64)
    A = float(a.sum())
    terms = np.concatenate([np.full(n.shape[0], gammaln(A)), -gammaln(A + n.sum(1)), gammaln(a + n).ravel(), -np.broadcast_to(gammaln(a), n.shape).ravel()])
    return float(terms.sum()), int(terms.size)
