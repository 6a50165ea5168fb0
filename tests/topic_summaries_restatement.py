"""The five topic summaries of cc/mallet/util/LDAUtils.java restated in numpy, for tests/test_topic_summaries_model.py (CPU)
and tests/test_topic_summaries_gpu.py (the kernels of csrc/ggs_topic_summaries.hpp, bit for bit).

  top          getTopWords / getTopWordIndices :874-911      (double) n_wk
  relevance    getTopRelevanceWords :566-590                 lambda * L + (1 - lambda) * (L - log(p_w[w])),  L = log(p_wk)
  distinctive  getTopDistinctiveWords :592-617, :654-664     0.0 + P * log(P / p_w[w])
  salient      getTopSalientWords :619-644, :674-685         p_w[w] * distinctive
  k1           getK1ReWeightedWords :752-801                 p_wk / (sum over k in index order of p_wk)

p_wk = (n_wk + beta) / mass_k (calcWordProbGivenTopic :803-818), p_w = rowsum_w / total (calcWordProb :704-720),
P = p_wk * (mass_k / total) / p_w, left to right (calcTopicProbGivenWord :826-856).  The three normalisers are Java running
sums from 0.0 over (double) n_wk + beta: np.cumsum is sequential, so cumsum(...)[-1] is that chain.  numpy rounds every
element-wise product, sum and quotient on its own.  log is the oracle's fdlibm log.  The rank is IDSorter's: falling score,
equal scores by FALLING id (-0.0 == +0.0)."""
import numpy as np

KINDS = ("top", "relevance", "distinctive", "salient", "k1")


def _log(x):
    from oracle import oracle as O
    O.build()
    return O.log(np.ascontiguousarray(x, np.float64)).reshape(np.shape(x))


def normalisers(counts, beta):
    """(mass_k [K], rowsum_w [V], total): the chains in Java index order."""
    x = np.asarray(counts).astype(np.float64) + np.float64(beta)
    mass = np.cumsum(x, axis=0)[-1]
    rowsum = np.cumsum(x, axis=1)[:, -1]
    total = np.cumsum(x.reshape(-1))[-1]
    return mass, rowsum, total


def scores(counts, beta, kind, lam=0.6, log=None):
    """all_scores [V][K] of the kind."""
    log = log or _log
    counts = np.asarray(counts)
    if kind == "top":
        return counts.astype(np.float64)
    lam = np.float64(lam)
    x = counts.astype(np.float64) + np.float64(beta)
    mass, rowsum, total = normalisers(counts, beta)
    with np.errstate(all="ignore"):
        p_wk = x / mass[None, :]
        p_w = rowsum / total
        if kind == "relevance":
            L = log(p_wk)
            return lam * L + (1 - lam) * (L - log(p_w)[:, None])
        if kind == "k1":
            return p_wk / np.cumsum(p_wk, axis=1)[:, -1][:, None]
        P = p_wk * (mass / total)[None, :] / p_w[:, None]
        d = 0.0 + P * log(P / p_w[:, None])
        if kind == "distinctive":
            return d
        if kind == "salient":
            return p_w[:, None] * d
    raise ValueError(kind)


def rank(all_scores, n):
    """idx [K][n]: per topic the n best word ids, by (-score, -id)."""
    s = np.asarray(all_scores, np.float64) + 0.0               # -0.0 + 0.0 = +0.0: the zeros compare equal anyway
    V, K = s.shape
    ids = np.arange(V)
    return np.stack([np.lexsort((-ids, -s[:, k]))[:n] for k in range(K)]).astype(np.int32)


def top_words(counts, beta, kind, n, lam=0.6):
    """(idx [K][n], score [K][n], all_scores [V][K])"""
    a = scores(counts, beta, kind, lam)
    idx = rank(a, n)
    return idx, a[idx, np.arange(a.shape[1])[:, None]], a


# ---- LDAUtils.java, statement for statement, on Python floats: the twin that checks the numpy form ----------------------
class IDSorter:
    """cc.mallet.types.IDSorter: compareTo puts the larger weight first and, for equal weights, the larger id."""

    def __init__(self, wi, p):
        self.wi, self.p = wi, p

    def compare_to(self, o):
        if o.p > self.p:
            return 1
        if o.p < self.p:
            return -1
        if o.wi > self.wi:
            return 1
        if o.wi < self.wi:
            return -1
        return 0


def literal(counts, beta, kind, n, lam=0.6):
    """(idx [K][n] as lists, all_scores [V][K] as lists) by the Java loops and Arrays.sort with IDSorter.compareTo."""
    import functools
    import math
    from oracle import oracle as O
    O.build()
    log = lambda v: float(O.log(np.array([v], np.float64))[0]) if v > 0 else (-math.inf if v == 0 else math.nan)   # noqa: E731
    c = np.asarray(counts)
    V, K = c.shape
    beta = float(beta)
    cell = [[float(int(c[w, k])) + beta for k in range(K)] for w in range(V)]
    if kind == "top":
        sc = [[float(int(c[w, k])) for k in range(K)] for w in range(V)]
    else:
        word_mass, word_probs = 0.0, [0.0] * V                         # calcWordProb
        for w in range(V):
            for k in range(K):
                word_mass += cell[w][k]
                word_probs[w] += cell[w][k]
        p_w = [word_probs[w] / word_mass for w in range(V)]
        p_wk = [[0.0] * K for _ in range(V)]                           # calcWordProbGivenTopic
        masses = []
        for k in range(K):
            m = 0.0
            for w in range(V):
                m += cell[w][k]
            masses.append(m)
            for w in range(V):
                p_wk[w][k] = cell[w][k] / m
        if kind == "relevance":
            sc = [[lam * log(p_wk[w][k]) + (1 - lam) * (log(p_wk[w][k]) - log(p_w[w])) for k in range(K)] for w in range(V)]
        elif kind == "k1":
            sc = [[0.0] * K for _ in range(V)]
            for w in range(V):
                m = 0.0
                for k in range(K):
                    m += p_wk[w][k]
                for k in range(K):
                    sc[w][k] = p_wk[w][k] / m
        else:
            topic_prob, type_sum, tot = [0.0] * K, [0.0] * V, 0.0      # calcTopicProbGivenWord
            for w in range(V):
                for k in range(K):
                    topic_prob[k] += cell[w][k]
                    type_sum[w] += cell[w][k]
                    tot += cell[w][k]
            ptw = [[0.0] * K for _ in range(V)]
            for w in range(V):
                for k in range(K):
                    a = cell[w][k] / topic_prob[k]
                    b = topic_prob[k] / tot
                    cc = type_sum[w] / tot
                    ptw[w][k] = a * b / cc
            dist = [[0.0] * K for _ in range(V)]
            for w in range(V):
                for k in range(K):
                    dist[w][k] += ptw[w][k] * log(ptw[w][k] / p_w[w])
            sc = dist if kind == "distinctive" else [[p_w[w] * dist[w][k] for k in range(K)] for w in range(V)]
    idx = []
    for k in range(K):
        order = sorted((IDSorter(w, sc[w][k]) for w in range(V)), key=functools.cmp_to_key(lambda a, b: a.compare_to(b)))
        idx.append([o.wi for o in order[:n]])
    return idx, sc


# ---- inputs of the GPU cases ---------------------------------------------------------------------------------------------
def zipf_counts(V, K, seed, density=0.08):
    """Sparse, Zipf-like counts [V][K]: word frequencies falling as 1 / rank (ranks shuffled over the ids), every word's tokens
    spread over the topics by a Dirichlet(0.3) draw -- nine cells in ten are zero at K = 100; `density` scales the frequencies."""
    rng = np.random.default_rng([V, K, seed])
    freq = (2.0 * V + 50.0) * (density / 0.08) / (1.0 + rng.permutation(V))
    theta = rng.dirichlet(np.full(K, 0.3), V) if K > 1 else np.ones((V, 1))
    return np.ascontiguousarray(rng.poisson(freq[:, None] * theta), np.int32)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)
