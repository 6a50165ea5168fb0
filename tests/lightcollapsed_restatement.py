"""CPU restatement of scheme=lightcollapsed (CollapsedLightLDA.java; ParallelLDA.java:429-433) as this library defines it
(include/ggs_hip.h, GGS_FLAG_LIGHTCOLLAPSED; DESIGN.md "6g. Scheme lightcollapsed"): the per-word tables and lists over the
counts, one token's two Metropolis-Hastings proposals, the z step with its three counters, the merge and whole sweeps, in
numpy and plain Python.  A test helper, not collected.  The Philox blocks come from the oracle; every floating-point
operation is the one the kernels perform, in their order, so results compare bit for bit.

The schedule.  schedule="parallel" is the device's: AD-LDA with one worker per document, the decomposition of
scheme=collapsed's parallel schedule.  The reference's per-batch private copy of typeTopicCounts / tokensPerTopic
(CollapsedLightLDA.java:795-802, moved by balanceGlobalCounts :1130-1135) shrinks to the sweep-start counts with the token in
flight moved: while a token of word w is processed, z0 its old topic and s its current one (z0, or an accepted word proposal),
    G(k) = n_wk[start][w][k] - [k == z0] + [k == s]        stands for globalTypeTopicCounts[type][k]
    T(k) = n_k[start][k]     - [k == z0] + [k == s]        stands for globalTokensPerTopic[k]
and earlier tokens of the same document do not move G or T.  n is the document's histogram with the token in flight (at s),
ni the same without it (localTopicCounts, localTopicCounts_i: both run along the document as in the reference).
With b = beta, bS = betaSum = beta * V, every count converted to double first, the five and four quotients multiplied left to
right (calculateWordAcceptanceProbability :1094-1128, calculateDocumentAcceptanceProbability :1050-1091):
    pi_w (t = word proposal != s = z0, a = alpha[z0]):
        (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1.0)) * (bS + (T(s) - 1.0)) / (bS + T(t))
                                  * (b + G(s)) / (b + G(t))         * (bS + T(t)) / (bS + T(s))
    pi_d (t = document proposal != s, a = alpha[s]):
        (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1.0)) * (bS + (T(s) - 1.0)) / (bS + T(t)) * (a + n[s]) / (a + n[t])
    accepted if pi > 1, else if U < pi (:967-986, :1014-1027).
schedule="serial" is the reference with batches = 1: one worker over all documents, G and T the one private copy moved in
place by every token.  It exists for the posterior measurement of tests/test_lightcollapsed_model.py; the device does not run it.

Decided here where the reference leaves the result to thread timing or history: a word's list is in ascending topic order;
topicCountBetaHat[k] = (double)n_k + betaSum, formed afresh each sweep; tokensPerType[w] = the integer sum of the word's
sweep-start row; table entries a build never pairs read a[i] = i, ps[i] = 1.0.
"""
import numpy as np

from tests import lightpclda_restatement as LR
from tests import spalias_restatement as SR

InvalidTopic = SR.InvalidTopic
WORD, DOC, STAY = LR.WORD, LR.DOC, LR.STAY                          # the three counters: where a token's new topic came from
TABLE, BETA = 0, 1                                                  # the two branches of the word proposal
token_uniforms = LR.token_uniforms
alpha_sum = LR.alpha_sum
accepts = LR.accepts
doc_proposal = LR.doc_proposal                                      # :994-1001, exactly as in LightPCLDA


def word_table(row, n_k, beta_sum):
    """One word's list and table from its count row [K] (TypeTopicParallelTableBuilder.java:38-51 over the ascending list;
    OptimizedGentleAliasMethodDynamicSize.reGenerateAliasTable :55-82 with k = nnz).  Returns (list [nnz], ps [nnz], a [nnz],
    typeMass, tokensPerType); a word without tokens builds nothing: ([], [], [], 0.0, 0)."""
    lst = [k for k in range(len(row)) if row[k] > 0]
    if not lst:
        return lst, np.zeros(0), np.zeros(0, np.int32), 0.0, 0
    p = [float(row[k]) / (float(n_k[k]) + beta_sum) for k in lst]   # p_i = n_w,L[i] / topicCountBetaHat[L[i]]
    ps, a, mass = SR.alias_table(p)                                 # typeMass: the i-order sum from 0.0; bs[i] = p_i / typeMass - 1.0 / nnz
    return lst, ps, a, mass, int(sum(int(row[k]) for k in lst))


def build_tables(n_wk, n_k, beta, V=None):
    """(ps [V][K], a [V][K], type_norm [V], nw [V], lists [V][K], tokens_per_type [V]) as the getters return them: behind
    nw[w] ps = 1.0, a = the index, the list -1."""
    n_wk = np.asarray(n_wk)
    V, K = n_wk.shape
    beta_sum = beta * float(V)
    ps, a = np.ones((V, K), np.float64), np.tile(np.arange(K, dtype=np.int32), (V, 1))
    tn, nw, lists, tpt = np.zeros(V, np.float64), np.zeros(V, np.int32), np.full((V, K), -1, np.int32), np.zeros(V, np.int64)
    nk = [int(x) for x in n_k]
    for w in range(V):
        lst, p, al, mass, tot = word_table(n_wk[w].tolist(), nk, beta_sum)
        n = len(lst)
        nw[w], tn[w], tpt[w] = n, mass, tot
        ps[w, :n], a[w, :n], lists[w, :n] = p, al, lst
    return ps, a, tn, nw, lists, tpt


def word_proposal(ps_w, a_w, list_w, nnz, tpt, beta, K, U1):
    """(topic, branch) of :946-954.  A table draw with i == nnz and a beta-branch topic == K raise (Java would index out of
    bounds)."""
    bK = beta * float(K)
    u_w = U1 * (float(tpt) + bK)
    if u_w < float(tpt):
        u = u_w / float(tpt)
        ups = u * float(nnz)                                        # generateSample(u), k = nnz
        i = int(ups)
        if i >= nnz:
            raise InvalidTopic("table draw at U1 = %r reaches nnz" % U1)
        if (ups - float(i)) > ps_w[i]:
            i = int(a_w[i])
        return int(list_w[i]), TABLE
    t = int(((u_w - float(tpt)) / bK) * float(K))
    if t >= K:
        raise InvalidTopic("beta branch at U1 = %r reaches K" % U1)
    return t, BETA


def word_ratio(a, b, bS, ni_t, ni_s, G_t, G_s, T_t, T_s):
    """calculateWordAcceptanceProbability, :1122-1126"""
    pi = (a + float(ni_t)) / (a + float(ni_s))
    pi *= (b + float(G_t)) / (b + (float(G_s) - 1.0))
    pi *= (bS + (float(T_s) - 1.0)) / (bS + float(T_t))
    pi *= (b + float(G_s)) / (b + float(G_t))
    pi *= (bS + float(T_t)) / (bS + float(T_s))
    return pi


def doc_ratio(a, b, bS, ni_t, ni_s, n_t, n_s, G_t, G_s, T_t, T_s):
    """calculateDocumentAcceptanceProbability, :1082-1088"""
    pi = (a + float(ni_t)) / (a + float(ni_s))
    pi *= (b + float(G_t)) / (b + (float(G_s) - 1.0))
    pi *= (bS + (float(T_s) - 1.0)) / (bS + float(T_t))
    pi *= (a + float(n_s)) / (a + float(n_t))
    return pi


def token_step(n, zdoc, pos, G, T, alpha, alpha_total, beta, beta_sum, table, U, detail=None):
    """One token, in place on the document's counts n [K] (the token still counted), its indicator array zdoc, and the
    worker's copy G (the word's row) / T (the topic totals), which hold the token at z0 on entry and at its new topic on
    return.  table = (ps_w, a_w, list_w, nnz, tokensPerType[w]).  Returns (WORD | DOC | STAY, TABLE | BETA).  Both proposals
    are formed before anything can raise, as the kernel forms them."""
    K = len(n)
    U1, U2, U3, U4 = U
    z0 = s = int(zdoc[pos])
    bad = None
    try:
        wp, branch = word_proposal(*table, beta, K, U1)
    except InvalidTopic as e:                                       # clamped to the last valid one
        bad = e
        u_w = U1 * (float(table[4]) + beta * float(K))
        wp, branch = (int(table[2][table[3] - 1]), TABLE) if u_w < float(table[4]) else (K - 1, BETA)
    try:
        dt, idx = doc_proposal(zdoc, alpha_total, K, U3)            # position pos still holds z0
    except InvalidTopic as e:
        bad, dt, idx = e, K - 1, None
    ni = lambda k: n[k] - (1 if k == s else 0)                      # noqa: E731 -- n without the token in flight
    acc_w = acc_d = False
    if wp != s:
        pi_w = word_ratio(float(alpha[s]), beta, beta_sum, ni(wp), ni(s), G[wp], G[s], T[wp], T[s])
        if detail is not None:
            detail["pi_w"] = pi_w
        acc_w = accepts(pi_w, U2)
        if acc_w:                                                   # :968-971 / :977-984, balanceGlobalCounts
            n[s] -= 1; n[wp] += 1
            G[s] -= 1; G[wp] += 1
            T[s] -= 1; T[wp] += 1
            s = wp
    new = z0                                                        # :928: kept when the proposal equals s (:1008)
    if dt != s:
        pi_d = doc_ratio(float(alpha[s]), beta, beta_sum, ni(dt), ni(s), n[dt], n[s], G[dt], G[s], T[dt], T[s])
        acc_d = accepts(pi_d, U4)
        new = dt if acc_d else s
        if detail is not None:
            detail["pi_d"] = pi_d
    n[s] -= 1                                                       # :1037-1045
    zdoc[pos] = new
    n[new] += 1
    G[s] -= 1; G[new] += 1
    T[s] -= 1; T[new] += 1
    if detail is not None:
        detail.update(word=wp, branch=branch, acc_w=acc_w, doc=dt, idx=idx, acc_d=acc_d, s=s, new=new)
    if bad is not None:
        raise bad
    return (DOC if acc_d else WORD if new != z0 else STAY), branch


def z_step(doc_ptr, tokens, z, n_wk, n_k, alpha, beta, tables, seed, iteration, tok_base=0, schedule="parallel", branches=None, on_token=None):
    """One z step in place on z.  n_wk [V][K], n_k [K]: the sweep-start counts; left untouched by schedule="parallel", moved
    in place by schedule="serial".  Returns the three counters [word kept, document accepted, left on z0]; `branches` [2]
    counts the word proposal's branch per token.  An invalid topic raises after the whole step, as the device reports it."""
    ps, a, _, nw, lists, tpt = tables
    V, K = n_wk.shape
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    total = alpha_sum(alpha, K)
    beta_sum = beta * float(V)
    stats = [0, 0, 0]
    bad = None
    T = [int(x) for x in n_k]
    rows = {}
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        zdoc = [int(k) for k in z[b:e]]
        n = [0] * K
        for k in zdoc:
            n[k] += 1
        for pos in range(e - b):
            w = int(tokens[b + pos])
            if w not in rows:
                rows[w] = n_wk[w].tolist()
            G = rows[w]
            z0 = zdoc[pos]
            det = {} if on_token is not None else None
            try:
                out, br = token_step(n, zdoc, pos, G, T, alpha, total, beta, beta_sum, (ps[w], a[w], lists[w], int(nw[w]), int(tpt[w])),
                                     token_uniforms(seed, iteration, tok_base + b + pos), det)
                stats[out] += 1
                if branches is not None:
                    branches[br] += 1
            except InvalidTopic as ex:
                bad = ex
            if on_token is not None:
                on_token(d, pos, det)
            if schedule == "parallel":                              # earlier tokens do not move G or T
                new = zdoc[pos]
                G[new] -= 1; G[z0] += 1
                T[new] -= 1; T[z0] += 1
        z[b:e] = zdoc
    if schedule == "serial":
        for w, G in rows.items():
            n_wk[w] = G
        n_k[:] = T
    if bad is not None:
        raise bad
    return stats


def count(tokens, z, V, K):
    """the merge: the (word, z) histogram, then tokensPerTopic"""
    n_wk = np.zeros((V, K), np.int64)
    np.add.at(n_wk, (np.asarray(tokens, np.int64), np.asarray(z, np.int64)), 1)
    return n_wk, n_wk.sum(axis=0)


class Model:
    """A whole lightcollapsed run: sweeps of (iteration += 1, table build, z step, merge).  There is no theta and no Phi."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, tok_base=0, schedule="parallel"):
        assert schedule in ("parallel", "serial")
        self.K, self.V, self.alpha, self.beta, self.seed, self.tok_base, self.schedule = K, V, alpha, beta, seed, tok_base, schedule
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.n_wk, self.n_k = count(self.tokens, self.z, V, K)
        self.iteration = 0
        self.stats = np.zeros(3, np.int64)
        self.branches = np.zeros(2, np.int64)
        self.on_token = None

    def tables(self):
        """of the current counts: what the next sweep builds at its head"""
        return build_tables(self.n_wk, self.n_k, self.beta)

    def sweep(self, n=1):
        for _ in range(n):
            self.iteration += 1
            self.stats += z_step(self.doc_ptr, self.tokens, self.z, self.n_wk, self.n_k, self.alpha, self.beta, self.tables(), self.seed,
                                 self.iteration, self.tok_base, self.schedule, self.branches, self.on_token)
            if self.schedule == "parallel":
                self.n_wk, self.n_k = count(self.tokens, self.z, self.V, self.K)

    def counts(self):
        return self.n_wk.astype(np.int32)

    def topic_totals(self):
        return self.n_k.astype(np.int32)

    def phi(self):
        """the point estimate ggs_get_phi returns for the count form: (beta + n_wk) / (betaSum + n_k), [K][V]"""
        return ((self.beta + self.n_wk.astype(np.float64)) / (self.beta * float(self.V) + self.n_k.astype(np.float64))).T.copy()
