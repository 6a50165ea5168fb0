"""CPU restatement of scheme=lightpclda (LightPCLDA.java:86-221) as this library defines it (include/ggs_hip.h,
GGS_FLAG_LIGHTPCLDA; DESIGN.md "6d. Scheme lightpclda"): one token's two Metropolis-Hastings proposals, the z step with
its three counters and a whole sweep, in plain Python.  A test helper, not collected.  The Philox blocks come from the
oracle, Phi from the oracle's pcgs sampler (lightpclda draws Phi exactly as pcgs does), the tables from
tests/spalias_restatement.py (they are spalias's: the reference's PhiTableBuilderFactory is never installed); every
floating-point operation of the z step is the one the kernel performs, in its order, so results compare bit for bit.
"""
import numpy as np

from oracle import oracle as O
from tests import spalias_restatement as SR

PURPOSE_Z = 1
InvalidTopic = SR.InvalidTopic
WORD, DOC, STAY = 0, 1, 2                                           # the three counters: where a token's new topic came from


def u53(a, b):
    """the library's 53-bit double of two Philox words (ggs_device_math.hpp u53, the oracle's bits_to_double)"""
    return float(((a >> 6) << 27) + (b >> 5)) * 2.0 ** -53


def token_uniforms(seed, iteration, gtok):
    """(U1, U2, U3, U4): the two doubles of block 0 and the two of block 1 of the token's Z stream"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = []
    for blk in (0, 1):
        o = O.philox((gtok & 0xFFFFFFFF, (gtok >> 32) & 0xFFFFFFFF, (PURPOSE_Z << 24) | blk, iteration), key)
        out += [u53(o[0], o[1]), u53(o[2], o[3])]
    return tuple(out)


def alpha_sum(alpha, K):
    """the k-order sum of alpha (ours)"""
    s = 0.0
    for a in np.broadcast_to(np.asarray(alpha, np.float64), (K,)).tolist():
        s = s + a
    return s


def word_ratio(alpha_s, ni_t, ni_s):
    """pi_w of LightPCLDA.java:138"""
    return (alpha_s + float(ni_t)) / (alpha_s + float(ni_s))


def doc_ratio(phi_t, phi_s, alpha_s, ni_t, ni_s, n_t, n_s):
    """nom / denom of LightPCLDA.java:181-183: left to right, counts converted first; IEEE as it falls"""
    nom = np.float64(phi_t) * np.float64(alpha_s + float(ni_t)) * np.float64(alpha_s + float(n_s))
    den = np.float64(phi_s) * np.float64(alpha_s + float(ni_s)) * np.float64(alpha_s + float(n_t))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(nom / den)


def accepts(ratio, u):
    """`ratio > 1`, else `u < ratio`: NaN accepts nothing, inf accepts"""
    return bool(ratio > 1.0) or bool(u < ratio)


def doc_proposal(zdoc, alpha_total, K, U3):
    """The document proposal of a token: zdoc is the document's indicator array as the reference holds it at that moment
    (new topics before the position, old ones from it on).  Returns (topic, index or None); the alpha branch reaching K
    raises (Java would index out of bounds)."""
    n = len(zdoc)
    ui = U3 * (float(n) + alpha_total)
    if ui < float(n):
        return int(zdoc[int(ui)]), int(ui)
    t = int(((ui - float(n)) / alpha_total) * float(K))
    if t >= K:
        raise InvalidTopic("alpha branch at U3 = %r reaches K" % U3)
    return t, None


def token_step(n, zdoc, pos, phi_w, alpha, alpha_total, ps_w, a_w, U, detail=None):
    """One token, in place on the document's counts n [K] (ints, the token still counted) and its indicator array zdoc.
    phi_w = the word's Phi column [K], alpha [K], U = (U1, U2, U3, U4).  Returns WORD, DOC or STAY.  Both proposals are
    formed before anything can raise, as the kernel forms them."""
    K = len(n)
    U1, U2, U3, U4 = U
    z0 = s = int(zdoc[pos])
    bad = None
    try:
        wp = SR.alias_sample(ps_w, a_w, U1)
    except InvalidTopic as e:
        bad, wp = e, K - 1
    try:
        dt, idx = doc_proposal(zdoc, alpha_total, K, U3)            # position pos still holds z0
    except InvalidTopic as e:
        bad, dt, idx = e, K - 1, None
    ni = lambda k: n[k] - (1 if k == s else 0)                      # noqa: E731 -- n without the token in flight
    acc_w = acc_d = False
    if wp != s:
        pi_w = word_ratio(float(alpha[s]), ni(wp), ni(s))
        if detail is not None:
            detail["pi_w"] = pi_w
        acc_w = accepts(pi_w, U2)
        if acc_w:
            n[s] -= 1
            n[wp] += 1
            s = wp
    new = z0                                                        # LightPCLDA.java:115: kept when the proposal equals s
    if dt != s:
        ratio = doc_ratio(phi_w[dt], phi_w[s], float(alpha[s]), ni(dt), ni(s), n[dt], n[s])
        acc_d = accepts(ratio, U4)
        new = dt if acc_d else s
        if detail is not None:
            detail["ratio"] = ratio
    n[s] -= 1
    zdoc[pos] = new
    n[new] += 1
    if detail is not None:
        detail.update(word=wp, acc_w=acc_w, doc=dt, idx=idx, acc_d=acc_d, s=s, new=new)
    if bad is not None:
        raise bad
    return DOC if acc_d else WORD if new != z0 else STAY


def z_step(doc_ptr, tokens, z, phi, alpha, tables, seed, iteration, tok_base=0):
    """One z step in place on z.  Returns the three counters [word kept, document accepted, left on z0].  An invalid
    topic raises after the whole step, as the device reports it."""
    ps, a, _ = tables
    K = phi.shape[0]
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    total = alpha_sum(alpha, K)
    phiT = np.ascontiguousarray(phi.T)
    stats = [0, 0, 0]
    bad = None
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
            try:
                stats[token_step(n, zdoc, pos, phiT[w], alpha, total, ps[w], a[w], token_uniforms(seed, iteration, tok_base + b + pos))] += 1
            except InvalidTopic as ex:
                bad = ex
        z[b:e] = zdoc
    if bad is not None:
        raise bad
    return stats


class Model:
    """A whole lightpclda run: init_phi, then sweeps (iteration += 1, z step, counts, Phi draw, the phi mean's gating).
    Phi and the phi mean are the oracle's pcgs ones; the tables follow every Phi."""

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
        self.stats = np.zeros(3, np.int64)

    def _new_phi(self):
        self.phi = self.o.get_phi()
        self.tables = SR.alias_tables(self.phi, self.alpha)

    def init_phi(self):
        self.o.init_phi()
        self._new_phi()

    def set_phi(self, phi):
        self.o.set_phi(phi)
        self._new_phi()

    def sample_z_given_phi(self, n=1):
        for _ in range(n):
            self.iteration += 1
            self.stats += z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.alpha, self.tables, self.seed, self.iteration, self.tok_base)

    def sweep(self, n=1):
        for _ in range(n):
            self.sample_z_given_phi(1)
            self.o.set_iteration(self.iteration)
            self.o.set_z(self.z.astype(np.int32), redraw_phi=False)   # the counts of the new assignments
            self.o.sample_phi()
            self._new_phi()

    def counts(self):
        return self.o.get_type_topic_counts()

    def topic_totals(self):
        return self.o.get_topic_totals()

    def phi_mean(self):
        return self.o.get_phi_mean()
