"""CPU restatement of scheme=adlda (ADLDA, ParallelLDA.java:409-412; MyWorkerRunnable.sampleTopicsForOneDoc,
MyWorkerRunnable.java:32-409) as this library defines it (include/ggs_hip.h, GGS_FLAG_ADLDA; DESIGN.md "6i. Scheme adlda"):
the SparseLDA bucket z step over the collapsed model on scheme=collapsed's parallel schedule, in numpy and plain Python.  A
test helper, not collected.  The uniforms come from the oracle's Philox; every floating-point operation is the one the
kernels perform, in their order (Python floats are IEEE doubles, one rounding per operation), so results compare bit for bit.

Sweep head, from the sweep-start counts N [V][K], T [K]:
    den0[k] = float(T[k]) + betaSum;  S0 = the k-order sum from 0.0 of (alpha_k * beta) / den0[k];
    L_w = the ascending list of the topics with N[w][k] > 0.
Per token (word w, old topic z0, U = the first uniform of block 0 of its Z stream), counts converted to float first, every
expression left to right:
    1. the token leaves the document (spalias's list discipline)
    2. T'(k) = T[k] - [k == z0], G'(k) = N[w][k] - [k == z0], den(k) = float(T'(k)) + betaSum
    3. S = S0 - (alpha_z0 * beta) / den0[z0] + (alpha_z0 * beta) / den(z0)
    4. R = the list-order sum from 0.0 of (beta * n_d[c]) / den(c) over the document's list
    5. Q = the list-order sum from 0.0 of score_j = ((alpha_k + n_d[k]) / den(k)) * G'(k), k = L_w[j]
    6. sample = U * (S + R + Q)
    7. the bucket and its walk (token_draw below)
    8. the token joins the document at its new topic.
"""
import numpy as np

from oracle import oracle as O
from tests import spalias_restatement as SR

InvalidTopic = SR.InvalidTopic
DocState = SR.DocState
PURPOSE_Z = SR.PURPOSE_Z
BUCKET_Q, BUCKET_R, BUCKET_S = 0, 1, 2


def head(n_wk, n_k, alpha, beta):
    """(den0 [K] list of floats, S0, nw [V], lists [V][K] with -1 behind the entries)"""
    n_wk = np.asarray(n_wk)
    V, K = n_wk.shape
    beta_sum = beta * float(V)
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    den0 = [float(int(n_k[k])) + beta_sum for k in range(K)]
    s0 = 0.0
    for k in range(K):
        s0 = s0 + (float(alpha[k]) * beta) / den0[k]
    nw, lists = np.zeros(V, np.int32), np.full((V, K), -1, np.int32)
    for w in range(V):
        lst = np.flatnonzero(n_wk[w] > 0)
        nw[w] = lst.size
        lists[w, :lst.size] = lst
    return den0, s0, nw, lists


def token_masses(st, z0, row_w, list_w, T, den0, s0, alpha, beta, beta_sum, mutant=None):
    """Steps 2 to 5 for one token whose old topic z0 has ALREADY been removed from st (step 1): S, R, Q, the word's scores and
    the terms of the other two walks, everything the draw needs that does not depend on U.  row_w = N[w][.] and T = T[.] of
    the sweep start, list_w = L_w (a sequence of topics).  `mutant` (tests only): "G" forgets the - [k == z0] in G', "T"
    forgets it in T', "zero" lets the Q walk move on to an entry of score 0.0 that follows the one it stopped at."""
    K = len(den0)
    cnt = st.cnt

    def den(k):                                                     # 2.
        if k == z0 and mutant != "T":
            return float(int(T[k]) - 1) + beta_sum
        return den0[k]

    def G(k):
        return int(row_w[k]) - (1 if (k == z0 and mutant != "G") else 0)

    ab = float(alpha[z0]) * beta
    S = s0 - ab / den0[z0] + ab / den(z0)                           # 3.
    R = 0.0
    for c in st.list:                                               # 4.
        R = R + (beta * float(cnt[c])) / den(c)
    scores = []
    Q = 0.0
    for k in list_w:                                                # 5.
        k = int(k)
        sc = ((float(alpha[k]) + float(cnt[k])) / den(k)) * float(G(k))
        scores.append(sc)
        Q = Q + sc
    return dict(K=K, S=S, R=R, Q=Q, scores=scores, list_w=[int(k) for k in list_w], doc_list=list(st.list), beta=beta,
                r_walk=[float(cnt[c]) / den(c) for c in st.list], s_walk=[float(alpha[k]) / den(k) for k in range(K)], mutant=mutant)


def token_walk(m, U, detail=None):
    """Steps 6 and 7: (topic, bucket) at the uniform U.  An invalid walk raises InvalidTopic carrying the clamped (topic,
    bucket) in its args[1]."""
    K, Q, R, scores, list_w = m["K"], m["Q"], m["R"], m["scores"], m["list_w"]
    sample = U * (m["S"] + R + Q)                                   # 6.
    if detail is not None:
        detail.update(S=m["S"], R=R, Q=Q, sample=sample)
    if sample < Q:                                                  # 7.
        i = -1
        while sample > 0:
            i += 1
            if i >= len(scores):
                raise InvalidTopic("the Q walk at U = %r runs past the word's last entry" % U, (list_w[len(scores) - 1], BUCKET_Q))
            sample -= scores[i]
        if m["mutant"] == "zero" and i + 1 < len(scores) and scores[i + 1] == 0.0:
            i += 1
        if detail is not None:
            detail["index"] = max(i, 0)
        return list_w[max(i, 0)], BUCKET_Q
    sample -= Q
    if sample < R:
        sample /= m["beta"]
        for i, c in enumerate(m["doc_list"]):
            sample -= m["r_walk"][i]
            if sample <= 0.0:
                if detail is not None:
                    detail["index"] = i
                return c, BUCKET_R
        if detail is not None:
            detail["fallback"] = True
        return K - 1, BUCKET_R                                      # :332-336, no error
    sample -= R
    sample /= m["beta"]
    k = 0
    sample -= m["s_walk"][0]
    while sample > 0.0:
        k += 1
        if k == K:
            raise InvalidTopic("the S walk at U = %r reaches K" % U, (K - 1, BUCKET_S))
        sample -= m["s_walk"][k]
    return k, BUCKET_S


def token_draw(st, z0, row_w, list_w, T, den0, s0, alpha, beta, beta_sum, U, detail=None, mutant=None):
    """The new topic and the bucket of one token whose old topic z0 has already been removed from st."""
    return token_walk(token_masses(st, z0, row_w, list_w, T, den0, s0, alpha, beta, beta_sum, mutant), U, detail)


def z_step(doc_ptr, tokens, z, n_wk, n_k, alpha, beta, seed, iteration, tok_base=0, mutant=None):
    """One z step in place on z against the sweep-start counts n_wk [V][K], n_k [K] (left untouched).  Returns the four
    counters [Q, R, S, sum of nnz_w + nnz_d].  An invalid topic raises after the whole step, as the device reports it."""
    n_wk = np.asarray(n_wk)
    V, K = n_wk.shape
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    beta_sum = beta * float(V)
    den0, s0, nw, lists = head(n_wk, n_k, alpha, beta)
    N = len(tokens)
    Us = O.uniforms(seed, iteration, PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    T = [int(x) for x in n_k]
    rows, lsts = {}, {}
    stats = [0, 0, 0, 0]
    bad = None
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        st = DocState(K, z[b:e])
        for pos in range(b, e):
            w, z0 = int(tokens[pos]), int(z[pos])
            if w not in rows:
                rows[w] = n_wk[w].tolist()
                lsts[w] = lists[w, :int(nw[w])].tolist()
            st.remove(z0)
            stats[3] += len(lsts[w]) + len(st.list)
            try:
                new, bucket = token_draw(st, z0, rows[w], lsts[w], T, den0, s0, alpha, beta, beta_sum, float(Us[pos]), mutant=mutant)
            except InvalidTopic as ex:
                bad = ex
                new, bucket = ex.args[1]
            stats[bucket] += 1
            st.add(new)
            z[pos] = new
    if bad is not None:
        raise bad
    return stats


def count(tokens, z, V, K):
    """the merge: the (word, z) histogram, then tokensPerTopic"""
    n_wk = np.zeros((V, K), np.int64)
    np.add.at(n_wk, (np.asarray(tokens, np.int64), np.asarray(z, np.int64)), 1)
    return n_wk, n_wk.sum(axis=0)


class Model:
    """A whole adlda run: sweeps of (iteration += 1, head, z step, merge).  There is no theta and no Phi."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, tok_base=0):
        self.K, self.V, self.alpha, self.beta, self.seed, self.tok_base = K, V, alpha, beta, seed, tok_base
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.n_wk, self.n_k = count(self.tokens, self.z, V, K)
        self.iteration = 0
        self.stats = np.zeros(4, np.int64)

    def sweep(self, n=1):
        for _ in range(n):
            self.iteration += 1
            self.stats += np.asarray(z_step(self.doc_ptr, self.tokens, self.z, self.n_wk, self.n_k, self.alpha, self.beta, self.seed,
                                            self.iteration, self.tok_base), np.int64)
            self.n_wk, self.n_k = count(self.tokens, self.z, self.V, self.K)

    def counts(self):
        return self.n_wk.astype(np.int32)

    def topic_totals(self):
        return self.n_k.astype(np.int32)

    def lists(self):
        """(nw [V], topics [V][K]) of the current counts, as ggs_get_word_topic_lists returns them"""
        _, _, nw, lists = head(self.n_wk, self.n_k, self.alpha, self.beta)
        return nw, lists

    def phi(self):
        """the point estimate ggs_get_phi returns for the count form: (beta + n_wk) / (betaSum + n_k), [K][V]"""
        return ((self.beta + self.n_wk.astype(np.float64)) / (self.beta * float(self.V) + self.n_k.astype(np.float64))).T.copy()
