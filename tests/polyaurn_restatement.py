"""CPU restatement of scheme=polyaurn (PolyaUrnSpaliasLDA) as this library defines it (include/ggs_hip.h,
GGS_FLAG_POLYAURN; DESIGN.md "Scheme polyaurn"): the Poisson tables, the Phi draw, the z step and a whole sweep, in numpy
and plain Python.  A test helper, not collected.  The Philox streams come from the oracle's uniforms / gaussians; every
floating-point operation is the one the kernels perform, in their order, so results compare bit for bit.
"""
import math

import numpy as np

from oracle import oracle as O

PURPOSE_Z, PURPOSE_PHI, PURPOSE_INIT_PHI = 1, 3, 4
DEFAULT_THRESHOLD = 100


def threshold_of(L):
    return DEFAULT_THRESHOLD if L == 0 else int(L)


def poisson_table(beta, L):
    """[L][2L]: row c = the cumulative table of Poisson(beta + c) truncated to 2L terms, renormalised, last entry 1.0."""
    L = threshold_of(L)
    n = 2 * L
    T = np.empty((L, n), np.float64)
    for c in range(L):
        lam = beta + float(c)
        p = math.exp(-lam)
        acc = 0.0
        S = [0.0] * n
        for j in range(n):
            if j > 0:
                p = p * lam / float(j)
            acc += p
            S[j] = acc
        for j in range(n - 1):
            T[c, j] = S[j] / S[n - 1]
        T[c, n - 1] = 1.0
    return T


def poisson_from_streams(counts, beta, L, u, g, table=None):
    """X for each count given the element's first uniform u and first Gaussian g (g is read only where c >= L)."""
    L = threshold_of(L)
    counts = np.asarray(counts, np.int64)
    T = poisson_table(beta, L) if table is None else table
    X = np.zeros(counts.shape, np.int64)
    small = counts < L
    for c in np.unique(counts[small]):
        sel = counts == c
        X[sel] = np.searchsorted(T[c], u[sel], side="right")        # the smallest j with u < T_c[j]
    big = ~small
    if big.any():
        lam = beta + counts[big].astype(np.float64)
        x = np.floor(np.sqrt(lam) * g[big] + lam + 0.5)
        X[big] = np.maximum(x, 0.0).astype(np.int64)
    return X


def poisson_draw(counts, beta, L, seed, iteration, purpose, elem0, table=None):
    """X of elements elem0 + i with counts[i] -- what ggs_debug_poisson returns."""
    counts = np.asarray(counts, np.int64).ravel()
    n = counts.size
    u = O.uniforms(seed, iteration, purpose, elem0, n)
    g = O.gaussians(seed, iteration, purpose, elem0, n) if (counts >= threshold_of(L)).any() else np.zeros(n)
    return poisson_from_streams(counts, beta, L, u, g, table)


def phi_draw(n_kw, beta, L, seed, iteration, initial, table=None):
    """(phi [K][V], X [K][V], tot [K]) from the corpus-wide counts n_kw [K][V]: element k * V + v."""
    n_kw = np.asarray(n_kw, np.int64)
    K, V = n_kw.shape
    X = poisson_draw(n_kw.ravel(), beta, L, seed, iteration, PURPOSE_INIT_PHI if initial else PURPOSE_PHI, 0, table).reshape(K, V)
    tot = X.sum(axis=1)
    phi = np.zeros((K, V), np.float64)
    nz = tot > 0
    phi[nz] = X[nz].astype(np.float64) / tot[nz, None].astype(np.float64)
    return phi, X, tot


def uniform_topic(U, K):
    return min(int(U * float(K)), K - 1)


def z_step(doc_ptr, tokens, z, phi, alpha, seed, iteration, tok_base=0):
    """One z step in place on z (UPLDA:1466-1544 as oracle/ggs_oracle.c:732-781 restates it, with the two rules of
    PolyaUrnSpaliasLDA.java:261-278).  Returns the number of tokens the rules drew uniformly."""
    K = phi.shape[0]
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    N = len(tokens)
    Us = O.uniforms(seed, iteration, PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    uniform_draws = 0
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        n = e - b
        if n == 0:
            continue
        cnt = np.bincount(z[b:e], minlength=K).astype(np.int64)
        for pos in range(b, e):
            w, old = int(tokens[pos]), int(z[pos])
            cnt[old] -= 1
            scores = (cnt.astype(np.float64) + alpha) * phi[:, w]
            sums = np.cumsum(scores)                                 # Java's sequential sum
            total = float(sums[-1])
            U = float(Us[pos])
            if n == 1 or total == 0.0:
                new = uniform_topic(U, K)
                uniform_draws += 1
            else:
                chain = np.cumsum(np.concatenate(([U * total], -scores)))   # sample -= score[k], in k order
                if not chain[0] > 0:
                    raise RuntimeError("invalid topic (sample <= 0) at token %d" % pos)
                past = np.flatnonzero(~(chain[1:] > 0))
                if past.size == 0:
                    raise RuntimeError("invalid topic (walk ran past K) at token %d" % pos)
                new = int(past[0])
            cnt[new] += 1
            z[pos] = new
    return uniform_draws


def counts_of(tokens, z, K, V):
    """n_kw [K][V] from the assignments."""
    n = np.zeros((K, V), np.int64)
    np.add.at(n, (np.asarray(z, np.int64), np.asarray(tokens, np.int64)), 1)
    return n


class Model:
    """A whole polyaurn run: init_phi, then sweeps (iteration += 1, z step, counts, Phi draw, the phi mean's gating)."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, L=0, save_phi_mean=False, phi_burn_in=0, phi_thin=1, tok_base=0):
        self.K, self.V, self.alpha, self.beta, self.seed, self.tok_base = K, V, alpha, beta, seed, tok_base
        self.L = threshold_of(L)
        self.table = poisson_table(beta, self.L)
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.iteration = 0
        self.save_phi_mean, self.phi_burn_in, self.phi_thin = save_phi_mean, phi_burn_in, max(1, phi_thin)
        self.phi_sum = np.zeros((K, V), np.float64)
        self.n_sampled = 0
        self.phi = None

    def counts(self):
        return counts_of(self.tokens, self.z, self.K, self.V)

    def init_phi(self):
        self.phi, _, _ = phi_draw(self.counts(), self.beta, self.L, self.seed, self.iteration, True, self.table)

    def sweep(self, n=1):
        for _ in range(n):
            self.iteration += 1
            z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.alpha, self.seed, self.iteration, self.tok_base)
            self.phi, _, _ = phi_draw(self.counts(), self.beta, self.L, self.seed, self.iteration, False, self.table)
            if self.save_phi_mean and self.phi_burn_in > 0 and self.iteration > self.phi_burn_in and self.iteration % self.phi_thin == 0:
                self.phi_sum += self.phi
                self.n_sampled += 1

    def phi_mean(self):
        return self.phi_sum / self.n_sampled if self.n_sampled else np.zeros_like(self.phi_sum)
