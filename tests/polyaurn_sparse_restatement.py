"""CPU restatement of scheme=polyaurn_sparse as this library defines it (include/ggs_hip.h, GGS_FLAG_POLYAURN_SPARSE;
DESIGN.md "6e. Scheme polyaurn_sparse"): polyaurn's Poisson Phi, spalias's alias tables and document lists, the words'
lists of non-zero topics and the doubly sparse z step of PolyaUrnSpaliasLDA.sampleTopicAssignmentsParallel, in numpy and
plain Python.  A test helper, not collected.  Every floating-point operation is the one the kernels perform, in their
order, so results compare bit for bit.
"""
import numpy as np

from oracle import oracle as O
from tests.polyaurn_restatement import (counts_of, phi_draw, poisson_draw, poisson_from_streams, poisson_table,  # noqa: F401
                                        threshold_of, uniform_topic)
from tests.spalias_restatement import DocState, InvalidTopic, alias_sample, alias_tables, list_search  # noqa: F401

PURPOSE_Z = 1
WORD, DOC, UNIFORM = 0, 1, 2                                        # which list a token took: the index into the statistics


def word_lists(phi):
    """(nw [V], lists): per word the topics k with phi[k][w] != 0.0 in ascending k -- what GGSHandle.word_topic_lists()
    returns (there as [V][K], -1 behind the entries)."""
    phi = np.asarray(phi, np.float64)
    lists = [np.flatnonzero(phi[:, w] != 0.0).astype(np.int64) for w in range(phi.shape[1])]
    return np.array([l.size for l in lists], np.int32), lists


def padded(lists, K):
    """the lists as the getter lays them out: int32 [V][K], -1 past nw[w]"""
    out = np.full((len(lists), K), -1, np.int32)
    for w, l in enumerate(lists):
        out[w, :l.size] = l
    return out


def token_draw(st, phi_w, nzw_w, ps_w, a_w, tn, U, K, detail=None):
    """The new topic of one token whose old topic has already been removed from st.  phi_w = the word's Phi column [K],
    nzw_w = the word's list.  detail["kind"] = WORD / DOC / UNIFORM, detail["n"] = the number of candidates; with
    candidates also cand, cum, sum, thr, prior, and then ul (the walk) or x, ups, i, frac and, where i < K, ps_i (the
    alias draw)."""
    nd, nw = len(st.list), len(nzw_w)
    use_word = nw < nd                                              # a tie goes to the document's list
    cand = [int(k) for k in nzw_w] if use_word else st.list
    n = len(cand)
    if detail is not None:
        detail.update(kind=UNIFORM if n == 0 else WORD if use_word else DOC, n=n)
    if n == 0:
        return uniform_topic(U, K)
    scores = np.asarray([st.cnt[k] for k in cand], np.float64) * phi_w[np.asarray(cand, np.int64)]
    cum = np.cumsum(scores)                                         # score first, running sum second, in candidate order
    s = float(cum[-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = np.float64(tn) / (np.float64(tn) + np.float64(s))
        prior = bool(U < thr)
        if detail is not None:
            detail.update(cand=cand, cum=cum, sum=s, thr=float(thr), prior=prior)
        if prior:
            x = U + (s * U) / tn
            if detail is not None:                                  # alias_sample's own quantities, for the edge builders
                ups = x * float(K)
                i = int(ups)
                detail.update(x=x, ups=ups, i=i, frac=ups - float(i))
                if i < K:
                    detail["ps_i"] = float(ps_w[i])
            return alias_sample(ps_w, a_w, x)
        ul = U * (tn + s) - tn
    if detail is not None:
        detail["ul"] = float(ul)
    return cand[list_search(cum, ul)]


def z_step(doc_ptr, tokens, z, phi, tables, lists, seed, iteration, tok_base=0, stats=None, over64=None):
    """One z step in place on z.  stats [4] += (word-list tokens, document-list tokens, uniform draws, sum of n);
    over64 [2] += the word-list / document-list tokens with more than 64 candidates."""
    ps, a, tn = tables
    K = phi.shape[0]
    N = len(tokens)
    Us = O.uniforms(seed, iteration, PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    phiT = np.ascontiguousarray(phi.T)
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        st = DocState(K, z[b:e])
        for pos in range(b, e):
            w = int(tokens[pos])
            st.remove(int(z[pos]))
            det = {}
            new = token_draw(st, phiT[w], lists[w], ps[w], a[w], float(tn[w]), float(Us[pos]), K, det)
            if stats is not None:
                stats[det["kind"]] += 1
                stats[3] += det["n"]
            if over64 is not None and det["kind"] != UNIFORM and det["n"] > 64:
                over64[det["kind"]] += 1
            st.add(new)
            z[pos] = new


class Model:
    """A whole polyaurn_sparse run: init_phi, then sweeps (iteration += 1, z step, counts, Poisson Phi draw, the phi mean's
    gating); set_phi / sample_z_given_phi as the handle's.  The tables and the words' lists follow every Phi."""

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
        self.phi = self.tables = self.nw = self.lists = None
        self.stats = np.zeros(4, np.int64)
        self.over64 = np.zeros(2, np.int64)

    def counts(self):
        return counts_of(self.tokens, self.z, self.K, self.V)

    def _new_phi(self, phi):
        self.phi = phi
        self.tables = alias_tables(phi, self.alpha)
        self.nw, self.lists = word_lists(phi)

    def init_phi(self):
        self._new_phi(phi_draw(self.counts(), self.beta, self.L, self.seed, self.iteration, True, self.table)[0])

    def set_phi(self, phi):
        self._new_phi(np.array(phi, np.float64))
        self.phi_sum[:] = 0.0                                       # setPhi restarts the running sum (UPLDA:1897-1902)

    def sample_z_given_phi(self, n=1):
        for _ in range(n):
            self.iteration += 1
            z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.tables, self.lists, self.seed, self.iteration, self.tok_base, stats=self.stats,
                   over64=self.over64)

    def sweep(self, n=1):
        for _ in range(n):
            self.sample_z_given_phi(1)
            self._new_phi(phi_draw(self.counts(), self.beta, self.L, self.seed, self.iteration, False, self.table)[0])
            if self.save_phi_mean and self.phi_burn_in > 0 and self.iteration > self.phi_burn_in and self.iteration % self.phi_thin == 0:
                self.phi_sum += self.phi
                self.n_sampled += 1

    def phi_mean(self):
        return self.phi_sum / self.n_sampled if self.n_sampled else np.zeros_like(self.phi_sum)
