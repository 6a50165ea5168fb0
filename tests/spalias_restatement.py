"""CPU restatement of scheme=spalias (SpaliasUncollapsedParallelLDA) as this library defines it (include/ggs_hip.h,
GGS_FLAG_SPALIAS; DESIGN.md "6c. Scheme spalias"): the alias tables, the draw from one, the sparse z step and a whole
sweep, in numpy and plain Python.  A test helper, not collected.  The Philox uniforms come from the oracle, Phi from the
oracle's pcgs sampler (spalias draws Phi exactly as pcgs does); every floating-point operation of the tables and the z
step is the one the kernels perform, in their order, so results compare bit for bit.
"""
import numpy as np

from oracle import oracle as O

PURPOSE_Z = 1


class InvalidTopic(RuntimeError):
    pass


def alias_table(pi):
    """(ps [K], a [K], typeNorm) of the unnormalised weights pi [K] -- reGenerateAliasTable, with ps = 1.0 wherever the
    pairing loop never writes it (ours)."""
    pi = np.asarray(pi, np.float64)
    K = pi.size
    tn = float(np.cumsum(pi)[-1])                                   # sequential, in k order; 0.0 + pi[0] is pi[0]
    inv_k = 1.0 / K
    with np.errstate(invalid="ignore", divide="ignore"):
        bs = (pi / tn - inv_k).tolist()
    lows = [k for k in range(K) if bs[k] < 0.0]
    highs = [k for k in range(K) if not bs[k] < 0.0]                # NaN lands here
    a = list(range(K))
    ps = [1.0] * K
    fk = float(K)
    while lows and highs:
        l = lows.pop()
        h = highs[-1]
        c, d = bs[l], bs[h]
        bs[l] = 0.0
        bs[h] = c + d
        if bs[h] <= 0.0:
            highs.pop()
        if bs[h] < 0.0:
            lows.append(h)
        a[l] = h
        ps[l] = 1.0 + fk * c
    return np.array(ps, np.float64), np.array(a, np.int32), tn


def alias_tables(phi, alpha):
    """(ps [V][K], a [V][K], typeNorm [V]) for phi [K][V] -- what ggs_debug_alias and GGSHandle.alias_tables() return."""
    phi = np.asarray(phi, np.float64)
    K, V = phi.shape
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    ps, a, tn = np.empty((V, K), np.float64), np.empty((V, K), np.int32), np.empty(V, np.float64)
    for w in range(V):
        ps[w], a[w], tn[w] = alias_table(phi[:, w] * alpha)
    return ps, a, tn


def alias_sample(ps, a, x):
    """sample(w, x) on one word's table; i == K raises (Java would throw)."""
    K = len(ps)
    ups = x * float(K)
    i = int(ups)
    if i >= K:
        raise InvalidTopic("alias draw at x = %r reaches K" % x)
    if (ups - float(i)) > ps[i]:
        i = int(a[i])
    return i


def implied_probabilities(ps, a):
    """what a table draws with: ps[i] / K to i and (1 - ps[i]) / K to a[i]"""
    K = len(ps)
    q = np.zeros(K, np.float64)
    for i in range(K):
        q[i] += ps[i] / K
        q[int(a[i])] += (1.0 - ps[i]) / K
    return q


class DocState:
    """A document's topic counts and the list of its non-zero topics in the reference's discipline."""

    def __init__(self, K, z_doc):
        self.cnt = [0] * K
        self.list = []
        self.pos = {}
        for k in z_doc:
            self.add(int(k))

    def add(self, k):
        self.cnt[k] += 1
        if self.cnt[k] == 1:                                        # appended
            self.pos[k] = len(self.list)
            self.list.append(k)

    def remove(self, k):
        self.cnt[k] -= 1
        if self.cnt[k] == 0:                                        # the list's last entry takes its slot
            i = self.pos.pop(k)
            last = self.list.pop()
            if last != k:
                self.list[i] = last
                self.pos[last] = i


def list_search(cum, ul):
    """the list index of the likelihood branch: the smallest i with ul <= cum[i]; ours: the last one if there is none"""
    return min(int(np.searchsorted(cum, ul, side="left")), len(cum) - 1)


def token_draw(st, old, phi_w, ps_w, a_w, tn, U, detail=None):
    """The new topic of one token whose old topic has already been removed from st.  phi_w = the word's Phi column [K]."""
    nnz = len(st.list)
    if nnz:
        idx = np.asarray(st.list, np.int64)
        scores = np.asarray([st.cnt[k] for k in st.list], np.float64) * phi_w[idx]
        cum = np.cumsum(scores)                                     # score first, running sum second, in list order
        s = float(cum[-1])
    else:
        cum = np.zeros(0)
        s = 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = np.float64(tn) / (np.float64(tn) + np.float64(s))
        prior = bool(U < thr)
    if detail is not None:
        detail.update(cum=cum, sum=s, thr=float(thr), prior=prior)
    if prior:
        return alias_sample(ps_w, a_w, U + (s * U) / tn)
    ul = U * (tn + s) - tn
    if detail is not None:
        detail["ul"] = ul
    if nnz == 0:
        return old                                                  # ours: slot 0 of Java's array still holds it
    return st.list[list_search(cum, ul)]


def z_step(doc_ptr, tokens, z, phi, tables, seed, iteration, tok_base=0):
    """One z step in place on z.  Returns (tokens drawn from the alias tables, sum of nnz over tokens)."""
    ps, a, tn = tables
    K = phi.shape[0]
    N = len(tokens)
    Us = O.uniforms(seed, iteration, PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    phiT = np.ascontiguousarray(phi.T)
    n_prior = nnz_sum = 0
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        st = DocState(K, z[b:e])
        for pos in range(b, e):
            w, old = int(tokens[pos]), int(z[pos])
            st.remove(old)
            det = {}
            new = token_draw(st, old, phiT[w], ps[w], a[w], float(tn[w]), float(Us[pos]), det)
            n_prior += det["prior"]
            nnz_sum += len(st.list)
            st.add(new)
            z[pos] = new
    return n_prior, nnz_sum


class Model:
    """A whole spalias run: init_phi, then sweeps (iteration += 1, z step, counts, Phi draw, the phi mean's gating).  Phi and
    the phi mean are the oracle's pcgs ones; the tables follow every Phi."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, save_phi_mean=False, phi_burn_in=0, phi_thin=1, tok_base=0):
        self.K, self.V, self.alpha, self.seed, self.tok_base = K, V, alpha, seed, tok_base
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.o = O.OracleSampler(K, V, alpha, beta, seed)
        self.o.set_scheme("pcgs")
        self.o.set_corpus(doc_ptr, np.asarray(tokens, np.int32))
        self.o.set_phi_mean_gating(save_phi_mean, phi_burn_in, phi_thin)
        self.o.set_z(self.z.astype(np.int32), redraw_phi=False)
        self.iteration = 0
        self.phi = self.tables = None
        self.n_prior = self.nnz_sum = 0

    def _new_phi(self):
        self.phi = self.o.get_phi()
        self.tables = alias_tables(self.phi, self.alpha)

    def init_phi(self):
        self.o.init_phi()
        self._new_phi()

    def set_phi(self, phi):
        self.o.set_phi(phi)
        self._new_phi()

    def sample_z_given_phi(self, n=1):
        for _ in range(n):
            self.iteration += 1
            p, s = z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.tables, self.seed, self.iteration, self.tok_base)
            self.n_prior += p
            self.nnz_sum += s

    def sweep(self, n=1):
        for _ in range(n):
            self.sample_z_given_phi(1)
            self.o.set_iteration(self.iteration)
            self.o.set_z(self.z.astype(np.int32), redraw_phi=False)   # the counts of the new assignments
            self.o.sample_phi()
            self._new_phi()

    def counts(self):
        return self.o.get_type_topic_counts()

    def phi_mean(self):
        return self.o.get_phi_mean()
