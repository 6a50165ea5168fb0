"""CPU restatement of scheme=lightpcldaw2 (LightPCLDAtypeTopicProposal.java:101-274) as this library defines it
(include/ggs_hip.h, GGS_FLAG_LIGHTPCLDAW2; DESIGN.md "6m. Scheme lightpcldaw2"): one token's two Metropolis-Hastings
proposals, the z step with its three counters and whole sweeps, in plain Python.  A test helper, not collected.  The Philox
blocks come from the oracle, Phi from the oracle's pcgs sampler (the scheme draws Phi exactly as pcgs does), the lists and
tables from tests/lightcollapsed_restatement.py (count_alias_build_kernel's: the tables the class declares); every
floating-point operation of the z step is the one the kernel performs, in its order, so results compare bit for bit.

Per token, G = the word's row of the SWEEP-START type-topic counts and bhat[k] = (double)n_k + betaSum of the sweep start:
nothing moves them for the token in flight, and earlier tokens do not either.  n is the document's histogram with the token in
flight (at s), ni the same without it.
    pi_w (t = word proposal != s = z0):  nom = phi[t][w] * (alpha[s] + ni[t]) * (beta + G[s]) * bhat[t]
                                         den = phi[s][w] * (alpha[s] + ni[s]) * (beta + G[t]) * bhat[s],  nom / den  (:270-272)
    pi_d: LightPCLDA's (tests/lightpclda_restatement.py doc_ratio; :254-256)
each product left to right, counts converted first; accepted if pi > 1, else if U < pi.
"""
import numpy as np

from oracle import oracle as O
from tests import lightcollapsed_restatement as LC
from tests import lightpclda_restatement as LR

InvalidTopic = LR.InvalidTopic
WORD, DOC, STAY = LR.WORD, LR.DOC, LR.STAY
TABLE, BETA = LC.TABLE, LC.BETA
token_uniforms = LR.token_uniforms
alpha_sum = LR.alpha_sum
accepts = LR.accepts
doc_proposal = LR.doc_proposal
doc_ratio = LR.doc_ratio
word_proposal = LC.word_proposal
build_tables = LC.build_tables
count = LC.count


def bhat(n_k, beta_sum):
    """topicCountBetaHat, formed afresh from the sweep-start tokensPerTopic"""
    return [float(int(x)) + beta_sum for x in n_k]


def word_ratio(phi_t, phi_s, alpha_s, ni_t, ni_s, beta, G_s, G_t, bhat_t, bhat_s):
    """nom / denom of calculateWordAcceptanceProbability, :270-272: left to right, counts converted first; IEEE as it falls"""
    nom = np.float64(phi_t) * np.float64(alpha_s + float(ni_t)) * np.float64(beta + float(G_s)) * np.float64(bhat_t)
    den = np.float64(phi_s) * np.float64(alpha_s + float(ni_s)) * np.float64(beta + float(G_t)) * np.float64(bhat_s)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return float(nom / den)


def token_step(n, zdoc, pos, phi_w, G, bh, alpha, alpha_total, beta, table, U, detail=None):
    """One token, in place on the document's counts n [K] (the token still counted) and its indicator array zdoc.  phi_w = the
    word's Phi column [K], G = the word's sweep-start count row [K], bh = bhat [K]; table = (ps_w, a_w, list_w, nnz,
    tokensPerType[w]).  Returns (WORD | DOC | STAY, TABLE | BETA).  Both proposals are formed before anything can raise, as the
    kernel forms them."""
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
        pi_w = word_ratio(phi_w[wp], phi_w[s], float(alpha[s]), ni(wp), ni(s), beta, G[s], G[wp], bh[wp], bh[s])
        if detail is not None:
            detail["pi_w"] = pi_w
        acc_w = accepts(pi_w, U2)
        if acc_w:                                                   # :168-185
            n[s] -= 1
            n[wp] += 1
            s = wp
    new = z0                                                        # :130: kept when the proposal equals s (:207)
    if dt != s:
        pi_d = doc_ratio(phi_w[dt], phi_w[s], float(alpha[s]), ni(dt), ni(s), n[dt], n[s])
        acc_d = accepts(pi_d, U4)
        new = dt if acc_d else s
        if detail is not None:
            detail["pi_d"] = pi_d
    n[s] -= 1                                                       # :235-241
    zdoc[pos] = new
    n[new] += 1
    if detail is not None:
        detail.update(word=wp, branch=branch, acc_w=acc_w, doc=dt, idx=idx, acc_d=acc_d, s=s, new=new)
    if bad is not None:
        raise bad
    return (DOC if acc_d else WORD if new != z0 else STAY), branch


def z_step(doc_ptr, tokens, z, phi, n_wk, n_k, alpha, beta, tables, seed, iteration, tok_base=0, branches=None, on_token=None):
    """One z step in place on z.  phi [K][V]; n_wk [V][K], n_k [K]: the sweep-start counts, left untouched.  Returns the three
    counters [word kept, document accepted, left on z0]; `branches` [2] counts the word proposal's branch per token.  An
    invalid topic raises after the whole step, as the device reports it."""
    ps, a, _, nw, lists, tpt = tables
    V, K = np.asarray(n_wk).shape
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    total = alpha_sum(alpha, K)
    bh = bhat(n_k, beta * float(V))
    phiT = np.ascontiguousarray(np.asarray(phi).T)
    stats = [0, 0, 0]
    bad = None
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
                rows[w] = (phiT[w].tolist(), [int(x) for x in n_wk[w]], (ps[w], a[w], lists[w], int(nw[w]), int(tpt[w])))
            phi_w, G, table = rows[w]
            det = {} if on_token is not None else None
            try:
                out, br = token_step(n, zdoc, pos, phi_w, G, bh, alpha, total, beta, table, token_uniforms(seed, iteration, tok_base + b + pos), det)
                stats[out] += 1
                if branches is not None:
                    branches[br] += 1
            except InvalidTopic as ex:
                bad = ex
            if on_token is not None:
                on_token(d, pos, det)
        z[b:e] = zdoc
    if bad is not None:
        raise bad
    return stats


class Model:
    """A whole lightpcldaw2 run: init_phi, then sweeps (iteration += 1, table build on the sweep-start counts, z step, counts,
    Phi draw, the phi mean's gating).  Phi and the phi mean are the oracle's pcgs ones."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, save_phi_mean=False, phi_burn_in=0, phi_thin=1, tok_base=0):
        self.K, self.V, self.alpha, self.beta, self.seed, self.tok_base = K, V, alpha, beta, seed, tok_base
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.o = O.OracleSampler(K, V, alpha, beta, seed)
        self.o.set_scheme("pcgs")
        self.o.set_corpus(doc_ptr, np.asarray(tokens, np.int32))
        self.o.set_phi_mean_gating(save_phi_mean, phi_burn_in, phi_thin)
        self.o.set_z(self.z.astype(np.int32), redraw_phi=False)
        self.iteration = 0
        self.phi = None
        self.stats = np.zeros(3, np.int64)
        self.branches = np.zeros(2, np.int64)
        self.on_token = None

    def start_counts(self):
        return count(self.tokens, self.z, self.V, self.K)

    def tables(self):
        """of the current counts: what the next z step builds at its head"""
        n_wk, n_k = self.start_counts()
        return build_tables(n_wk, n_k, self.beta)

    def init_phi(self):
        self.o.init_phi()
        self.phi = self.o.get_phi()

    def set_phi(self, phi):
        self.o.set_phi(phi)
        self.phi = self.o.get_phi()

    def set_z(self, z):
        self.z = np.array(z, np.int64)
        self.o.set_z(self.z.astype(np.int32), redraw_phi=False)

    def sample_z_given_phi(self, n=1):
        for _ in range(n):
            self.iteration += 1
            n_wk, n_k = self.start_counts()
            self.stats += z_step(self.doc_ptr, self.tokens, self.z, self.phi, n_wk, n_k, self.alpha, self.beta, build_tables(n_wk, n_k, self.beta),
                                 self.seed, self.iteration, self.tok_base, self.branches, self.on_token)

    def sweep(self, n=1):
        for _ in range(n):
            self.sample_z_given_phi(1)
            self.o.set_iteration(self.iteration)
            self.o.set_z(self.z.astype(np.int32), redraw_phi=False)   # the counts of the new assignments
            self.o.sample_phi()
            self.phi = self.o.get_phi()

    def counts(self):
        return self.o.get_type_topic_counts()

    def topic_totals(self):
        return self.o.get_topic_totals()

    def phi_mean(self):
        return self.o.get_phi_mean()
