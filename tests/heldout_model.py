"""The left-to-right held-out estimator (MarginalProbEstimatorPlain.evaluateLeftToRight without resampling) against the
model, for documents short enough to enumerate.  A test helper, not collected; the manner of tests/lda_posterior.py.

The model.  With the training counts n_wk, n_k fixed, phi_hat[k][w] = (n_wk + beta) / (n_k + V beta).  A particle walks a
test document w_0 .. w_{L-1}; before position n it holds topics z_<n with document counts c_k (sum c = n), and

    f_n(z_<n)            = sum_k (alpha_k + c_k) / (alphaSum + n) * phi_hat[k][w_n]          its word probability,
    q(z_n = k | z_<n)    ~ (alpha_k + c_k) * phi_hat[k][w_n]                                  its draw.

The estimator of one document is  sum_n log( (1 / P) sum_particles f_n ).  Without resampling every particle is an
independent path of q, so the inner mean converges to E_n = E_q[f_n], NOT to p(w_n | w_<n): the estimator's limit is the
sequential-proposal limit  sum_n log E_n, which is p(w) only for documents of one and two tokens (E_0 and E_1 are exact:
q(z_0) is the posterior of z_0).  For K = 3 and L <= 6 there are at most 729 paths and the limit is enumerated here.

The same enumeration gives the estimator's error to first order in 1 / P.  With g(path) = sum_n f_n / E_n,

    estimate - sum_n log E_n  =  mean_particles(g) - L  -  sum_n (mean f_n - E_n)^2 / (2 E_n^2)  + O(P^-3/2):

variance Var_q(g) / P and bias -sum_n Var_q(f_n) / (2 P E_n^2).  zscores() therefore needs no measured tolerance.

ParticleSampler is the estimator in NumPy from the two lines above (not from the three-bucket form of the Java text and
not from oracle/); its mutants exist only to show that the statistic has power.
"""
import collections
import itertools

import numpy as np

K = 3
V = 5
ALPHA = (0.3, 0.9, 1.7)                                             # the posterior fixture's values (tests/lda_posterior.py)
BETA = 0.4
PAD_ALPHA = 1e-12
P = 4000
R = 200
BOUND_MEAN = 4.5                                                    # |mean z| * sqrt(R): the bound of the Rao-Blackwell rows
BOUND_SQ = (0.7, 1.4)                                               # mean(z^2): +-4 sigma of a chi-square with 200 degrees of freedom, over 200

# The training corpus and its z: the counts are the fixture (laid down with set_z(z, redraw_phi=False)).
TRAIN_LENS = (5, 3, 6, 4, 2, 7, 4, 5)
TRAIN_TOKENS = (0, 1, 0, 2, 4, 3, 3, 1, 2, 2, 0, 4, 1, 2, 0, 0, 3, 4, 1, 4, 4, 1, 0, 2, 3, 3, 1, 2, 0, 4, 2, 1, 3, 0, 1, 4)
TRAIN_Z = (0, 1, 0, 2, 2, 1, 1, 1, 2, 2, 0, 1, 1, 2, 0, 0, 1, 2, 0, 2, 2, 1, 0, 2, 1, 2, 1, 2, 0, 0, 2, 1, 1, 0, 2, 1)
# Test documents of 3 to 6 tokens: a repeated word, all words different, one word but for one token, every word with one repeat.
DOCS = ((0, 0, 1), (0, 1, 2, 3), (2, 2, 2, 4, 2), (4, 3, 1, 0, 2, 3))


def train_corpus():
    """(doc_ptr, tokens, z)"""
    ptr = np.concatenate(([0], np.cumsum(TRAIN_LENS))).astype(np.int64)
    assert ptr[-1] == len(TRAIN_TOKENS) == len(TRAIN_Z)
    return ptr, np.asarray(TRAIN_TOKENS, np.int32), np.asarray(TRAIN_Z, np.int32)


def train_counts(num_topics=K):
    """(n_wk [V][num_topics], n_k [num_topics]) of the fixture's z"""
    n_wk = np.zeros((V, num_topics), np.int64)
    np.add.at(n_wk, (np.asarray(TRAIN_TOKENS), np.asarray(TRAIN_Z)), 1)
    return n_wk, n_wk.sum(axis=0)


def padded_alpha(num_topics):
    return np.concatenate((ALPHA, np.full(num_topics - K, PAD_ALPHA)))


def heldout_corpus(copies=R, docs=DOCS, pad_to=0, num_types=V):
    """(doc_ptr, tokens, which): every document `copies` times (copy r of document i is test document i * copies + r: another
    document index, another stream).  pad_to: out-of-vocabulary ids (num_types, num_types + 1, ...) before, between and after
    the words until the document has pad_to tokens; they take no draw and no tokensSoFar."""
    rows, which = [], []
    for i, doc in enumerate(docs):
        row = list(doc)
        if pad_to:
            extra = pad_to - len(row)
            head, mid = extra // 3, extra // 3
            row = [num_types] * head + row[:2] + [num_types + 1 + (j % 7) for j in range(mid)] + row[2:] + [2 ** 31 - 1] * (extra - head - mid)
            assert len(row) == pad_to
        rows += [row] * copies
        which += [i] * copies
    ptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    return ptr, np.array([t for r in rows for t in r], np.int32), np.asarray(which)


Limit = collections.namedtuple("Limit", "log_e var_g bias e var paths_q")


def limit(doc, n_wk, n_k, alpha, beta, pad_topics=0, pad_alpha=0.0):
    """The sequential-proposal limit of one document by enumeration of all K^L paths, in float64:
    Limit(sum_n log E_n, Var_q(g), the bias coefficient -sum_n Var_n / (2 E_n^2), E_n [L], Var_n [L], sum_paths q).

    pad_topics, pad_alpha: the same with pad_topics further topics of alpha = pad_alpha and no training token in the model
    (phi_hat = 1 / V each) -- their mass enters f_n and the normaliser of q, the paths that visit one are left out (paths_q
    then falls short of 1 by their probability)."""
    n_wk = np.asarray(n_wk, np.float64)
    alpha = np.asarray(alpha, np.float64)
    nK, nV, L = alpha.size, n_wk.shape[0], len(doc)
    phi = (n_wk + beta) / (np.asarray(n_k, np.float64) + nV * beta)           # [V][K]
    a_sum = float(alpha.sum()) + pad_topics * pad_alpha
    pad = pad_topics * pad_alpha * (beta / (nV * beta))                        # sum over the padded topics of alpha_k * phi_hat
    q_all, f_all = [], []
    for path in itertools.product(range(nK), repeat=L):
        c = np.zeros(nK)
        q, f = 1.0, np.empty(L)
        for n, w in enumerate(doc):
            weight = (alpha + c) * phi[w]
            total = float(weight.sum()) + pad
            f[n] = total / (a_sum + n)
            q *= weight[path[n]] / total
            c[path[n]] += 1.0
        q_all.append(q)
        f_all.append(f)
    q_all, f_all = np.asarray(q_all), np.asarray(f_all)
    e = q_all @ f_all
    var = q_all @ (f_all - e) ** 2
    g = (f_all / e).sum(axis=1)
    var_g = float(q_all @ (g - float(q_all @ g)) ** 2)
    return Limit(float(np.log(e).sum()), var_g, float(-(var / (2.0 * e * e)).sum()), e, var, float(q_all.sum()))


def zscores(est, lim, particles):
    """(est - sum log E_n - bias / P) / sqrt(Var_q(g) / P) for the estimates est [...] of one document"""
    return (np.asarray(est, np.float64) - lim.log_e - lim.bias / particles) / np.sqrt(lim.var_g / particles)


def statistics(est, which, limits, particles):
    """per document: (|mean z| * sqrt(R), mean(z^2), max |z|) of its copies' estimates"""
    out = []
    for i, lim in enumerate(limits):
        z = zscores(np.asarray(est)[which == i], lim, particles)
        out.append((abs(float(z.mean())) * np.sqrt(z.size), float((z * z).mean()), float(np.abs(z).max())))
    return out


def accepted(stats):
    return all(m < BOUND_MEAN and BOUND_SQ[0] < s < BOUND_SQ[1] for m, s, _ in stats)


def rejected(stats):
    return any(m > BOUND_MEAN for m, _, _ in stats)


MUTANTS = ("late", "beta_first", "coef_stuck", "so_far_stuck")


class ParticleSampler:
    """The estimator from the product form, vectorised over particles.

    mutant: None, or one slip --
      "late"          for 3 % of the tokens the draw lands one topic late (clamped to K - 1)
      "beta_first"    a draw that falls in the c_k * beta part of the weight returns the first topic with c_k > 0
      "coef_stuck"    the coefficient of the n_wk part does not follow the count beyond 1: (alpha_k + min(c_k, 1)) n_wk / (n_k + V beta)
      "so_far_stuck"  tokensSoFar does not advance beyond 1 in the denominator: alphaSum + min(n, 1)
    The last two are invisible to one- and two-token documents."""

    def __init__(self, n_wk, n_k, alpha, beta, seed, mutant=None):
        if mutant is not None and mutant not in MUTANTS:
            raise ValueError("mutant %r" % (mutant,))
        self.n_wk = np.asarray(n_wk, np.float64)
        self.alpha = np.asarray(alpha, np.float64)
        self.beta = float(beta)
        self.denom = np.asarray(n_k, np.float64) + self.n_wk.shape[0] * self.beta
        self.rng = np.random.default_rng(seed)
        self.mutant = mutant

    def estimate(self, doc, particles, copies):
        """[copies] estimates of one document, each from its own `particles` particles"""
        nK = self.alpha.size
        n_part = particles * copies
        c = np.zeros((n_part, nK))
        a_sum = float(self.alpha.sum())
        out = np.zeros(copies)
        for n, w in enumerate(doc):
            prior = self.alpha + c
            if self.mutant == "coef_stuck":
                weight = (prior * self.beta + (self.alpha + np.minimum(c, 1.0)) * self.n_wk[w]) / self.denom
            else:
                weight = prior * ((self.n_wk[w] + self.beta) / self.denom)
            total = weight.sum(axis=1)
            f = total / (a_sum + (min(n, 1) if self.mutant == "so_far_stuck" else n))
            out += np.log(f.reshape(copies, particles).mean(axis=1))
            cum = np.cumsum(weight, axis=1)
            x = self.rng.random(n_part) * total
            k = np.minimum((cum <= x[:, None]).sum(axis=1), nK - 1)
            if self.mutant == "late":
                k = np.minimum(k + (self.rng.random(n_part) < 0.03), nK - 1)
            elif self.mutant == "beta_first":
                # the weight of topic k is [alpha_k beta + alpha_k' n_wk] + c_k beta, over denom_k: a draw is in the second
                # part with probability c_k beta / denom_k / total -- taken here as a second uniform against that share
                share = c * self.beta / self.denom
                in_beta = self.rng.random(n_part) * total < share.sum(axis=1)
                redo = np.cumsum(weight - share, axis=1)
                y = self.rng.random(n_part) * redo[:, -1]
                k = np.where(in_beta, np.argmax(c > 0, axis=1), np.minimum((redo <= y[:, None]).sum(axis=1), nK - 1))
            c[np.arange(n_part), k] += 1.0
        return out

    def run(self, docs=DOCS, particles=P, copies=R):
        """(estimates, which) in the layout of heldout_corpus()"""
        est = np.concatenate([self.estimate(doc, particles, copies) for doc in docs])
        return est, np.repeat(np.arange(len(docs)), copies)


def padding_bound(doc, n_wk, n_k, alpha, beta, pad_topics, pad_alpha=PAD_ALPHA):
    """(what the padded smoothing mass can move sum log E_n by on the unpadded paths, what the paths that visit a padded topic
    can): both absolute, in the estimate's own unit.

    f_n is a convex combination of phi_hat[.][w_n] (the weights (alpha_k + c_k) / (alphaSum + n) sum to 1), so f_n and E_n lie
    between lo_n and hi_n, the least and largest phi_hat of the word (1 / V of a padded topic included).  With
    delta = pad_topics * pad_alpha, S = alphaSum and A = sum_k (alpha_k + c_k) phi_hat[k][w_n] >= S lo_n:
      on the unpadded paths  f' / f = (1 + delta / (V A)) / (1 + delta / (S + n)), so |log f' - log f| <= r_n = delta (1 / (V S lo_n) + 1 / S),
        and a path's weight q moves by at most the factors of its earlier draws: log E_n moves by at most r_n + sum_{m<n} r_m;
      a path has visited a padded topic before position n with probability at most sum_{m<n} delta / (V S lo_m), and moves E_n by
        at most that times (hi_n - lo_n): log E_n by at most that times hi_n / lo_n."""
    n_wk = np.asarray(n_wk, np.float64)
    nV = n_wk.shape[0]
    phi = (n_wk + beta) / (np.asarray(n_k, np.float64) + nV * beta)
    s = float(np.sum(alpha))
    delta = pad_topics * pad_alpha
    on_paths = leaked = 0.0
    r_before = p_before = 0.0
    for w in doc:
        lo, hi = float(phi[w].min()), max(float(phi[w].max()), 1.0 / nV)
        lo = min(lo, 1.0 / nV)
        r = delta * (1.0 / (nV * s * lo) + 1.0 / s)
        on_paths += r + r_before
        leaked += p_before * hi / lo
        r_before += r
        p_before += delta / (nV * s * lo)
    return on_paths, leaked
