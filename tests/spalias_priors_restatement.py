"""CPU restatement of scheme=spalias_priors (SpaliasUncollapsedParallelWithPriors) as this library defines it
(include/ggs_hip.h, ggs_set_topic_priors; DESIGN.md "6f. Scheme spalias_priors").  A test helper, not collected.

  * the z step is tests/spalias_restatement.py's with the reference's prior factor written out literally at list index >= 1
    (score = cnt * phi * prior, SpaliasUncollapsedParallelWithPriors.java:256,263);
  * the initial Phi is the oracle's, multiplied by the priors (:63-72), rows not renormalised;
  * the Phi of a sweep is ConditionalDirichlet.nextConditionalDistribution (ConditionalDirichlet.java:80-101) over each topic's
    allowed words: the oracle's unnormalised gammas of the current counts (OracleSampler.phi_gammas_range: the same Philox
    elements k*V + v, shape ((beta + n) / m) * m with m over ALL v), g <= 0 -> 1e-4, both sums sequential (np.cumsum), then
    (g / sum_gamma) * sum_phi.

With cells=None the Model is spalias_restatement.Model (haveTopicPriors == false).
"""
import numpy as np

from oracle import oracle as O
from tests import spalias_restatement as R

MIN_GAMMA = 0.0001                                                  # ConditionalDirichlet.java:90-92


def priors_matrix(K, V, cells):
    P = np.ones((K, V), np.float64)
    topics, words = cells
    if len(topics):
        P[np.asarray(topics, np.int64), np.asarray(words, np.int64)] = 0.0
    return P


def random_cells(rng, K, V, n_anchor, n_third, counts=None):
    """A cell list: the n_anchor most frequent words (by counts [V]; a random order without) anchored to one random topic each,
    and a random third of the topics masked for the n_third words after them."""
    order = np.argsort(-np.asarray(counts), kind="stable") if counts is not None else rng.permutation(V)
    t, w = [], []
    for v in order[:n_anchor]:
        keep = int(rng.integers(K))
        for k in range(K):
            if k != keep:
                t.append(k), w.append(int(v))
    for v in order[n_anchor:n_anchor + n_third]:
        for k in rng.choice(K, max(1, K // 3), replace=False):
            t.append(int(k)), w.append(int(v))
    return np.asarray(t, np.int32), np.asarray(w, np.int32)


def token_draw(st, old, phi_w, prior_w, ps_w, a_w, tn, U):
    """spalias_restatement.token_draw with the prior factor at every list position but the first."""
    nnz = len(st.list)
    if nnz:
        idx = np.asarray(st.list, np.int64)
        scores = np.asarray([st.cnt[k] for k in st.list], np.float64) * phi_w[idx]
        scores[1:] = scores[1:] * prior_w[idx[1:]]                  # cnt * phi * prior, left to right
        cum = np.cumsum(scores)
        s = float(cum[-1])
    else:
        cum = np.zeros(0)
        s = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = np.float64(tn) / (np.float64(tn) + np.float64(s))
        prior = bool(U < thr)
    if prior:
        return R.alias_sample(ps_w, a_w, U + (s * U) / tn), True
    ul = U * (tn + s) - tn
    if nnz == 0:
        return old, False
    return st.list[R.list_search(cum, ul)], False


def z_step(doc_ptr, tokens, z, phi, P, tables, seed, iteration, tok_base=0):
    """One z step in place on z, the prior factor included.  Returns the number of tokens drawn from the alias tables."""
    ps, a, tn = tables
    K = phi.shape[0]
    N = len(tokens)
    Us = O.uniforms(seed, iteration, R.PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    phiT, PT = np.ascontiguousarray(phi.T), np.ascontiguousarray(P.T)
    n_prior = 0
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        st = R.DocState(K, z[b:e])
        for pos in range(b, e):
            w, old = int(tokens[pos]), int(z[pos])
            st.remove(old)
            new, from_table = token_draw(st, old, phiT[w], PT[w], ps[w], a[w], float(tn[w]), float(Us[pos]))
            n_prior += from_table
            st.add(new)
            z[pos] = new
    return n_prior


def conditional_phi(phi_old, gam, P):
    """nextConditionalDistribution for every topic: (new phi [K][V], clamped cells per topic, unclamped cells per topic)."""
    K, V = phi_old.shape
    new = phi_old.copy()
    clamped, unclamped = np.zeros(K, np.int64), np.zeros(K, np.int64)
    for k in range(K):
        idx = np.flatnonzero(P[k] != 0.0)                           # :343-356, ascending
        g = gam[k, idx].copy()
        low = g <= 0
        g[low] = MIN_GAMMA
        clamped[k], unclamped[k] = int(low.sum()), int((~low).sum())
        sum_gamma = float(np.cumsum(g)[-1])                         # sequential, from 0.0
        sum_phi = float(np.cumsum(phi_old[k, idx])[-1])
        new[k, idx] = (g / sum_gamma) * sum_phi                     # the division first
    return new, clamped, unclamped


class Model(R.Model):
    """A whole spalias_priors run.  The oracle keeps the counts and draws the gammas; Phi and the running phi mean live here."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, cells=None, save_phi_mean=False, phi_burn_in=0, phi_thin=1, tok_base=0):
        super().__init__(K, V, alpha, beta, seed, doc_ptr, tokens, z0, save_phi_mean=save_phi_mean, phi_burn_in=phi_burn_in, phi_thin=phi_thin, tok_base=tok_base)
        self.P = None if cells is None else priors_matrix(K, V, cells)
        self._gating = (bool(save_phi_mean), int(phi_burn_in), int(phi_thin))
        self._mean_sum, self._mean_n = np.zeros((K, V), np.float64), 0
        self.clamped = self.unclamped = None                        # of the last sweep, per topic

    def init_phi(self):
        if self.P is None:
            return super().init_phi()
        self.o.init_phi()
        self.phi = self.o.get_phi() * self.P                        # :63-72
        self.tables = R.alias_tables(self.phi, self.alpha)

    def set_phi(self, phi):
        if self.P is None:
            return super().set_phi(phi)
        phi = np.asarray(phi, np.float64)
        if (phi[self.P == 0.0] != 0.0).any():
            raise ValueError("phi is not zero in a cell the topic priors zero")     # ours (ggs_set_phi: GGS_ERR_BAD_ARG)
        self.phi = phi.copy()
        self.tables = R.alias_tables(self.phi, self.alpha)
        self._mean_sum[:] = 0.0                                     # UPLDA:1897-1902: the running sum restarts

    def sample_z_given_phi(self, n=1):
        if self.P is None:
            return super().sample_z_given_phi(n)
        for _ in range(n):
            self.iteration += 1
            self.n_prior += z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.P, self.tables, self.seed, self.iteration, self.tok_base)

    def sweep(self, n=1):
        if self.P is None:
            return super().sweep(n)
        save, burn_in, thin = self._gating
        for _ in range(n):
            self.sample_z_given_phi(1)
            self.o.set_iteration(self.iteration)
            self.o.set_z(self.z.astype(np.int32), redraw_phi=False)   # the counts of the new assignments
            gam, _ = self.o.phi_gammas_range(0, self.K)
            self.phi, self.clamped, self.unclamped = conditional_phi(self.phi, gam, self.P)
            if save and burn_in > 0 and self.iteration > burn_in and self.iteration % thin == 0:   # UPLDA:1350-1352
                self._mean_sum += self.phi                          # :363-367, zeros included
                self._mean_n += 1
            self.tables = R.alias_tables(self.phi, self.alpha)

    def phi_mean(self):
        if self.P is None:
            return super().phi_mean()
        return (self._mean_sum / self._mean_n, self._mean_n) if self._mean_n else (None, 0)
