"""CPU restatement of scheme=nzvsspalias as this library defines it (include/ggs_hip.h, GGS_FLAG_NZVSSPALIAS; DESIGN.md
"6h. Scheme nzvsspalias"): NZVSSpaliasUncollapsedParallelLDA over VSDirichlet, in numpy and plain Python.  A test helper, not
collected.  Every floating-point operation is the one the kernels perform, in their order, so results compare bit for bit.

  * strict_exp is fdlibm's __ieee754_exp (StrictMath.exp), lgS MALLET's Dirichlet.logGammaStirling over the oracle's StrictMath.log;
  * indicator_probability is VSDirichlet.calculateIndicatorProbIsOne (:102-112);
  * sequential_chain is the indicator half of VSDirichlet.nextDistribution (:46-84), cell by cell;
  * rounds_chain is a numpy model of vs_chain_kernel's rounds (csrc/ggs_phi_vs.hpp);
  * vs_phi is the whole draw: the chain, Gamma(n + beta) for the drawn cells, the index-order sum, the division (ours: a row
    of sum 0 becomes zeros);
  * the initial Phi, the gammas and the uniforms come from the oracle, the alias tables and the documents' lists from
    tests/spalias_restatement.py, the doubly sparse walk from tests/polyaurn_sparse_restatement.py; a token without a
    candidate draws from its word's alias table (NZVSSpaliasUncollapsedParallelLDA.java:252-254).
"""
import struct

import numpy as np

from oracle import oracle as O
from tests import polyaurn_sparse_restatement as PS
from tests import spalias_restatement as R

PURPOSE_Z, PURPOSE_PHI, PURPOSE_VS = 1, 3, 6
WORD, DOC, ALIAS = 0, 1, 2                                          # which way a token took: the index into the statistics

_LN2HI, _LN2LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
_INVLN2 = 1.44269504088896338700e+00
_O_THRESHOLD, _U_THRESHOLD = 7.09782712893383973096e+02, -7.45133219101941108420e+02
_TWOM1000 = 9.33263618503218878990e-302
_P1, _P2, _P3, _P4, _P5 = (1.66666666666666019037e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05,
                           -1.65339022054652515390e-06, 4.13813679705723846039e-08)


def _words(x):
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return b >> 32, b & 0xFFFFFFFF


def _add_to_hi(x, n):
    hi, lo = _words(x)
    return struct.unpack("<d", struct.pack("<Q", (((hi + n) & 0xFFFFFFFF) << 32) | lo))[0]


def strict_exp(x):
    """fdlibm 5.3 e_exp.c, operation by operation"""
    x = float(x)
    hx, lx = _words(x)
    xsb = (hx >> 31) & 1
    hx &= 0x7FFFFFFF
    hi = lo = 0.0
    k = 0
    if hx >= 0x40862E42:                                            # |x| >= 709.78...
        if hx >= 0x7FF00000:
            if (hx & 0xFFFFF) | lx:
                return x + x                                        # NaN
            return x if xsb == 0 else 0.0
        if x > _O_THRESHOLD:
            return float("inf")                                     # huge * huge
        if x < _U_THRESHOLD:
            return 0.0                                              # twom1000 * twom1000
    if hx > 0x3FD62E42:                                             # |x| > 0.5 ln2
        if hx < 0x3FF0A2B2:                                         # and |x| < 1.5 ln2
            hi = x - (-_LN2HI if xsb else _LN2HI)
            lo = -_LN2LO if xsb else _LN2LO
            k = 1 - xsb - xsb
        else:
            k = int(_INVLN2 * x + (-0.5 if xsb else 0.5))           # (int): towards zero
            t = float(k)
            hi = x - t * _LN2HI
            lo = t * _LN2LO
        x = hi - lo
    elif hx < 0x3E300000:                                           # |x| < 2^-28
        if 1.0e300 + x > 1.0:
            return 1.0 + x
    t = x * x
    c = x - t * (_P1 + t * (_P2 + t * (_P3 + t * (_P4 + t * _P5))))
    if k == 0:
        return 1.0 - ((x * c) / (c - 2.0) - x)
    y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi)
    if k >= -1021:
        return _add_to_hi(y, k << 20)
    return _add_to_hi(y, (k + 1000) << 20) * _TWOM1000


HALF_LOG_TWO_PI = 0.91893853320467274178


def lgS(z):
    """Dirichlet.logGammaStirling of an array, as the device's log_gamma_stirling"""
    z = np.array(z, np.float64).reshape(-1)
    shift = np.zeros(z.size, np.int64)
    with np.errstate(all="ignore"):
        while (z < 2).any():
            m = z < 2
            z[m] += 1.0
            shift[m] += 1
        result = HALF_LOG_TWO_PI + (z - 0.5) * O.log(z) - z + 1 / (12 * z) - 1 / (360 * z * z * z) + 1 / (1260 * z * z * z * z * z)
        while (shift > 0).any():
            m = shift > 0
            shift[m] -= 1
            z[m] -= 1.0
            result[m] -= O.log(z[m])
    return result


def indicator_exponent(s, n_k, beta):
    """lgS(a + beta) + lgS(a + n_k) - lgS(a + beta + n_k) - lgS(a) for a = s * beta, arrays of s"""
    a = np.asarray(s, np.float64) * beta
    nk = float(int(n_k))
    with np.errstate(all="ignore"):
        return lgS(a + beta) + lgS(a + nk) - lgS(a + beta + nk) - lgS(a)


def indicator_probability(s, n_k, beta, pi):
    """calculateIndicatorProbIsOne for an array of s"""
    e = indicator_exponent(np.atleast_1d(s), n_k, beta)
    odds = pi / (1 - pi)
    with np.errstate(all="ignore"):
        r = np.array([strict_exp(x) for x in e], np.float64) * odds
        return r / (1 + r)


class Probabilities:
    """p(s) of one topic, computed in stretches and kept"""

    def __init__(self, n_k, beta, pi):
        self.n_k, self.beta, self.pi = int(n_k), beta, pi
        self.known = {}

    def __call__(self, s):
        s = int(s)
        if s not in self.known:
            half = max(48, len(self.known) // 2)                    # a chain that has wandered far goes on wandering
            want = [t for t in range(max(0, s - half), s + half + 1) if t not in self.known]
            for t, p in zip(want, indicator_probability(np.array(want), self.n_k, self.beta, self.pi)):
                self.known[t] = float(p)
        return self.known[s]

    def many(self, s):
        return np.array([self(t) for t in s], np.float64)


def out_of_range(p):
    return bool(p > 1 or p < 0)                                     # the reference's check: NaN passes it


def sequential_chain(counts, prev_phi, U, beta, pi):
    """The indicators of one topic as VSDirichlet.nextDistribution decides them: (drawn [V] bool, s behind the last cell,
    True if the reference's range check would throw)."""
    counts = np.asarray(counts)
    V = counts.size
    n_k = int(np.sum(counts, dtype=np.int64))
    s = int(np.sum(np.asarray(prev_phi) == 0.0))
    P = Probabilities(n_k, beta, pi)
    drawn = np.ones(V, bool)
    bad = False
    for v in range(V):
        if counts[v] != 0:
            continue
        p = P(s)
        bad |= out_of_range(p)
        if U[v] > p:
            drawn[v] = False
            if prev_phi[v] != 0.0:
                s += 1
        elif prev_phi[v] == 0.0:
            s -= 1
    return drawn, s, bad


def rounds_chain(counts, prev_phi, U, beta, pi, confirm=True, max_rounds=None):
    """vs_chain_kernel's rounds: s is kept at the start of every 32-cell word (s0 everywhere before the first round); a round
    walks every word cell by cell from its start, then the starts become s0 + the exclusive scan of the words' steps; rounds
    repeat until one changes no decision and no start.  confirm=False ends at the first round that changes no DECISION,
    without confirming that the starts it has just moved leave the decisions standing (the tests show that this is wrong);
    max_rounds ends after that many rounds whatever they changed (wrong too: tests/test_nzvs_knife_edge_model.py).
    Returns (drawn [V] bool, s behind the last cell, rounds)."""
    counts = np.asarray(counts)
    V = counts.size
    W = (V + 31) // 32
    cz, pz, Uw = np.zeros(W * 32, bool), np.zeros(W * 32, bool), np.zeros(W * 32, np.float64)
    cz[:V], pz[:V], Uw[:V] = counts == 0, np.asarray(prev_phi) == 0.0, U
    cz, pz, Uw = cz.reshape(W, 32), pz.reshape(W, 32), Uw.reshape(W, 32)
    n_k, s0 = int(np.sum(counts, dtype=np.int64)), int(pz.sum())
    P = Probabilities(n_k, beta, pi)
    sw, und = np.full(W, s0, np.int64), np.zeros((W, 32), bool)
    rounds = 0
    live = [b for b in range(32) if cz[:, b].any()]                 # a position at which no word has a cell without a count decides nothing
    while True:
        s, un = sw.copy(), np.zeros((W, 32), bool)
        for b in live:
            with np.errstate(invalid="ignore"):
                above = Uw[:, b] > P.many(s)                        # false for a NaN p
            undrawn, kept = cz[:, b] & above, cz[:, b] & ~above
            s = s + (undrawn & ~pz[:, b]) - (kept & pz[:, b])
            un[:, b] = undrawn
        d = s - sw
        new_sw = s0 + np.concatenate(([0], np.cumsum(d)[:-1]))
        changed = bool((un != und).any()) or (confirm and bool((new_sw != sw).any()))
        und, sw, s_end = un, new_sw, s0 + int(d.sum())
        rounds += 1
        if not changed or rounds == max_rounds:
            break
        assert rounds <= V + 2
    return ~und.reshape(-1)[:V], s_end, rounds


def vs_phi(counts_kv, prev_phi, beta, pi, seed, iteration, U=None):
    """One variable-selection draw of all topics: (phi [K][V], drawn [K][V] bool, s_end [K]).  U [K][V]: the indicators'
    uniforms, the oracle's Philox stream GGS_PURPOSE_VS by default."""
    counts_kv = np.asarray(counts_kv)
    K, V = counts_kv.shape
    if U is None:
        U = O.uniforms(seed, iteration, PURPOSE_VS, 0, K * V).reshape(K, V)
    gam = O.gammas(seed, iteration, PURPOSE_PHI, 0, (counts_kv.astype(np.float64) + beta).reshape(-1)).reshape(K, V)
    phi, drawn, s_end = np.zeros((K, V), np.float64), np.zeros((K, V), bool), np.zeros(K, np.int64)
    for k in range(K):
        drawn[k], s_end[k], bad = sequential_chain(counts_kv[k], prev_phi[k], U[k], beta, pi)
        if bad:
            raise ArithmeticError("Inconsistent Indicator probability")
        row = np.where(drawn[k], gam[k], 0.0)                       # an undrawn cell uses none of its gamma stream
        total = float(np.cumsum(row)[-1])                           # sequential, from 0.0
        phi[k] = row / total if total > 0 else 0.0                  # ours: the reference writes NaN for a row of sum 0
    return phi, drawn, s_end


def drawn_lists(drawn):
    """(nw [V], lists): per word the topics whose cell was drawn, ascending (nonZeroTypeTopicIdxs, :517-524)"""
    lists = [np.flatnonzero(drawn[:, w]).astype(np.int64) for w in range(drawn.shape[1])]
    return np.array([l.size for l in lists], np.int32), lists


def token_draw(st, phi_w, nzw_w, ps_w, a_w, tn, U, K, detail=None):
    """polyaurn_sparse_restatement.token_draw, except that a token without a candidate draws from its word's alias table"""
    nd, nw = len(st.list), len(nzw_w)
    if (nw if nw < nd else nd) == 0:
        if detail is not None:
            detail.update(kind=ALIAS, n=0)
        return R.alias_sample(ps_w, a_w, U)
    return PS.token_draw(st, phi_w, nzw_w, ps_w, a_w, tn, U, K, detail)


def z_step(doc_ptr, tokens, z, phi, tables, lists, seed, iteration, tok_base=0, stats=None, trace=None):
    """One z step in place on z.  stats [4] += (word-list tokens, document-list tokens, alias-only tokens, sum of n);
    trace, a list, receives per token (position, word, counts before the draw, document list, U, kind, new topic)."""
    ps, a, tn = tables
    K = phi.shape[0]
    N = len(tokens)
    Us = O.uniforms(seed, iteration, PURPOSE_Z, tok_base, N) if N else np.zeros(0)
    phiT = np.ascontiguousarray(phi.T)
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        if e == b:
            continue
        st = R.DocState(K, z[b:e])
        for pos in range(b, e):
            w = int(tokens[pos])
            st.remove(int(z[pos]))
            det = {}
            if trace is not None:
                before = (list(st.cnt), list(st.list))
            new = token_draw(st, phiT[w], lists[w], ps[w], a[w], float(tn[w]), float(Us[pos]), K, det)
            if stats is not None:
                stats[det["kind"]] += 1
                stats[3] += det["n"]
            if trace is not None:
                trace.append(dict(pos=pos, w=w, cnt=before[0], list=before[1], U=float(Us[pos]), kind=det["kind"], new=new))
            st.add(new)
            z[pos] = new


class Model:
    """A whole nzvsspalias run.  The oracle's pcgs sampler keeps the counts and draws the initial Phi; the variable-selection
    Phi, the lists and the statistics live here."""

    def __init__(self, K, V, alpha, beta, seed, doc_ptr, tokens, z0, pi=0.5, tok_base=0):
        self.K, self.V, self.alpha, self.beta, self.seed, self.pi, self.tok_base = K, V, alpha, beta, seed, pi, tok_base
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int64)
        self.z = np.array(z0, np.int64)
        self.o = O.OracleSampler(K, V, alpha, beta, seed)
        self.o.set_scheme("pcgs")
        self.o.set_corpus(doc_ptr, np.asarray(tokens, np.int32))
        self.o.set_z(self.z.astype(np.int32), redraw_phi=False)
        self.iteration = 0
        self.phi = self.tables = self.nw = self.lists = self.drawn = None
        self.stats = np.zeros(4, np.int64)
        self.n_undrawn = 0

    def counts(self):
        return PS.counts_of(self.tokens, self.z, self.K, self.V)   # [K][V]

    def _new_phi(self, phi, lists):
        self.phi = phi
        self.tables = R.alias_tables(phi, self.alpha)
        self.nw, self.lists = lists

    def init_phi(self):
        self.o.set_z(self.z.astype(np.int32), redraw_phi=False)
        self.o.init_phi()
        empty = [np.zeros(0, np.int64)] * self.V                    # the reference fills no list before its first samplePhi
        self._new_phi(self.o.get_phi(), (np.zeros(self.V, np.int32), empty))
        self.n_undrawn = 0

    def set_phi(self, phi):
        phi = np.array(phi, np.float64)
        self._new_phi(phi, PS.word_lists(phi))                      # ours: the cells with phi != 0.0

    def sample_z_given_phi(self, n=1):
        for _ in range(n):
            self.iteration += 1
            z_step(self.doc_ptr, self.tokens, self.z, self.phi, self.tables, self.lists, self.seed, self.iteration, self.tok_base, stats=self.stats)

    def sweep(self, n=1):
        for _ in range(n):
            self.sample_z_given_phi(1)
            phi, self.drawn, self.s_end = vs_phi(self.counts(), self.phi, self.beta, self.pi, self.seed, self.iteration)
            self.n_undrawn = int((~self.drawn).sum())
            self._new_phi(phi, drawn_lists(self.drawn))

    def vs_stats_first_two(self):
        return self.n_undrawn, int((self.phi == 0.0).sum())


# ---- rows for the chain's tests (tests/test_nzvs_model.py and tests/test_nzvs_gpu.py share them) ------------------------
def states_before(counts, prev_phi, U, beta, pi):
    """s as the sequential chain holds it BEFORE each cell [V]"""
    counts = np.asarray(counts)
    n_k = int(np.sum(counts, dtype=np.int64))
    s = int(np.sum(np.asarray(prev_phi) == 0.0))
    P = Probabilities(n_k, beta, pi)
    out = np.zeros(counts.size, np.int64)
    for v in range(counts.size):
        out[v] = s
        if counts[v] != 0:
            continue
        if U[v] > P(s):
            s += prev_phi[v] != 0.0
        else:
            s -= prev_phi[v] == 0.0
    return out


def random_row(rng, V, zero_count=0.8, zero_prev=0.5):
    """(counts, prev_phi, U): about zero_count of the cells without tokens, about zero_prev of the old cells 0.0"""
    counts = np.where(rng.random(V) < zero_count, 0, rng.integers(1, 40, V)).astype(np.int32)
    prev = np.where(rng.random(V) < zero_prev, 0.0, rng.random(V) + 1e-3)
    return counts, prev, rng.random(V)


def edge_row(rng, V, cell, above, beta, pi):
    """A random row whose cell `cell` has no tokens and U exactly on p(s) (drawn) or, `above`, one ulp over it (undrawn)"""
    counts, prev, U = random_row(rng, V)
    counts[cell] = 0
    if counts.sum() == 0 and V > 1:
        counts[(cell + 1) % V] = 7                                   # n_k > 0
    s = int(states_before(counts, prev, U, beta, pi)[cell])
    p = Probabilities(int(counts.sum()), beta, pi)(s)
    if not (p == p and 0.0 < p < 1.0):                              # s == 0: p is 0 or NaN, no edge to stand on
        prev[:] = np.where(prev == 0.0, 0.5, prev)
        prev[(cell + 1) % V if V > 1 else 0] = 0.0 if V > 1 else prev[0]
        s = int(states_before(counts, prev, U, beta, pi)[cell])
        p = Probabilities(int(counts.sum()), beta, pi)(s)
    U[cell] = np.nextafter(p, 2.0) if above else p
    return counts, prev, U


def back_to_zero_row(V, beta, pi):
    """s0 = 5 falls to 0 inside the first word (five old zeros, all kept: U = 0) and stays there: from then on p = 0 and a cell
    is undrawn unless U == 0.  Cell 64, at the start of the third word, carries U = p(5): kept by a round that still believes
    s0, undrawn in the chain -- the row a stop without the confirming round gets wrong."""
    assert V >= 65
    counts, prev, U = np.zeros(V, np.int32), np.full(V, 0.25), np.zeros(V)
    counts[40] = 50
    prev[:5] = 0.0
    U[64] = Probabilities(50, beta, pi)(5)
    return counts, prev, U


def chain_cases(beta=0.01, seed=11):
    """[(name, counts [V], prev_phi [V], U [V], pi)]: the rows the issue names"""
    rng = np.random.default_rng(seed)
    out = []
    for V in (1, 2, 63, 64, 65, 4097):
        for pi in (0.5, 0.01):
            out.append(("random V=%d pi=%g" % (V, pi),) + random_row(rng, V) + (pi,))
        c, p, u = random_row(rng, V)
        out.append(("all counts zero (n_k == 0) V=%d" % V, np.zeros(V, np.int32), p, u, 0.5))
        out.append(("no count zero V=%d" % V, np.maximum(c, 1), p, u, 0.5))
        out.append(("s0 == 0 V=%d" % V, c, np.where(p == 0.0, 0.5, p), u, 0.5))
        out.append(("s0 == V V=%d" % V, c, np.zeros(V), u, 0.5))
        out.append(("n_k == 0 and s0 == 0 V=%d" % V, np.zeros(V, np.int32), np.full(V, 0.5), u, 0.5))
    for V in (65, 4097):
        out.append(("s returns to 0 V=%d" % V,) + back_to_zero_row(V, beta, 0.5) + (0.5,))
    for V, cells in ((65, (0, 64)), (4097, (0, 64, 4096))):
        for cell in cells:
            for above in (False, True):
                out.append(("U %s p(s) at cell %d, V=%d" % ("one ulp above" if above else "on", cell, V),) + edge_row(rng, V, cell, above, beta, 0.5) + (0.5,))
    return out


def exp_grid():
    """the 10^5 points of the exp tests and the special values behind them"""
    x = np.random.default_rng(1).uniform(-745.0, 710.0, 100000)
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), 7.09782712893383973096e+02, np.nextafter(7.09782712893383973096e+02, 1e9),
               -7.45133219101941108420e+02, np.nextafter(-7.45133219101941108420e+02, -1e9), 1e-10, -1e-10, 0.3, -0.3, 1.0, -1.0, 0.5 * np.log(2.0), 1.5 * np.log(2.0)]
    return np.concatenate((x, np.array(special)))
