"""Knife-edge rows for scheme=nzvsspalias (a test helper, not collected; the manner of tests/polyaurn_sparse_knife_edge.py and
tests/adlda_knife_edge.py).  tests/test_nzvs_knife_edge_model.py checks the rows on the CPU, tests/test_nzvs_knife_edge_gpu.py
sends them through the device.

The chain (vs_chain_kernel, csrc/ggs_phi_vs.hpp)
  cascade_row     a row that needs one round per 32-cell word.  Every cell carries a count except the first cell of each of
                  the W whole words; the tail behind them carries counts throughout.  The first cell of an even word is an
                  old zero with U = p(s) exactly: kept, s falls by one.  The first cell of an odd word is an old non-zero with
                  U one ulp above p(s): undrawn, s rises by one.  So s alternates between s0 and s0 - 1, and every word
                  decides right only from its right start: p increases in s (asserted where the row is built), so an even
                  word keeps its cell iff its start is >= s0 and an odd word leaves its cell iff its start is <= s0 - 1.
                  A round's scan hands word j its right start only once the words before it are right: W rounds settle the
                  row and one more confirms it.
  window_report   the rounds once more, with the kernel's table rule: w0 = max(0, s_min - 32), tn = min(kVsTab, s_max + 32 -
                  w0 + 1); a lookup with ti = s - w0 < tn reads the table, any other computes p on the spot.  While tn is not
                  clamped the table reaches s_max + 32 and a word moves s by at most 31 before its last lookup: ti <= tn - 2.
                  So ti == tn - 1, ti == tn and ti > tn exist only under the clamp at kVsTab, where the starts span more
                  than kVsTab - 65 values of s.
  staircase_row   that span, with every lookup decisive: `steps` cells without a count at the head of the row, each an exact
                  tie.  Down: old zeros with U = p(s), kept, s falls through s0 .. s0 - steps.  Up: old non-zeros with U one
                  ulp above p(s), undrawn, s rises.  From the second round on the starts span the staircase, the table is
                  clamped, and the chain passes through every s: through w0 + kVsTab - 1 (the table's last entry) and
                  w0 + kVsTab (the first computed on the spot).  A table filled one entry short would decide a tie from
                  stale LDS.

The z step (nzvs_wave_kernel = sparse_wave_body<true, PolyaurnSparseParams, true>)
  Every row of tests/polyaurn_sparse_knife_edge.py has at least three candidates, and so has every prefix token there (a
  one-hot word in a document of three or more topics): under nzvsspalias the draw is polyaurn_sparse's, and those fixtures
  run as they are.  The kernel's own branch is the token WITHOUT a candidate: sample(w, U) on the word's alias table,
  i = (int)(U K), the alias a[w][i] if U K - i > ps[w][i].
  AliasEdge       one-token documents: the old topic leaves, nd = 0, and the draw is the table's whatever nw is.  U, and with
                  it i and frac = U K - i, are the stream's and cannot be steered, so the "cell" edge (U K against an integer)
                  is out of reach; what can be steered is ps[w][i].  Entry i of the target word's Phi column is aimed at the
                  share frac / K (a share under 1 / K: ps[w][i] = K pi_i / typeNorm), bisected on its bit pattern for the flip
                  of frac > ps[w][i] and scanned over 2 * SCAN + 1 neighbouring doubles: "tie" (frac == ps[w][i]: not above,
                  the draw is i), "below" / "above" (ps[w][i] within two ulps over / under frac), "far".  Rows whose frac
                  does not suit or whose aim found no flip are "plain".  Behind them a few documents of several tokens with a
                  word whose column is all zero ("zero column": nw = 0 < nd, the same branch with use_word true; its table
                  is the identity, the draw is i)."""
import numpy as np

from oracle import oracle as O
from tests import nzvs_restatement as R
from tests import polyaurn_sparse_restatement as PS
from tests import spalias_restatement as SR

# csrc/ggs_phi_vs.hpp (tests/test_nzvs_knife_edge_model.py holds these against the header's text)
KVS_BLOCK, KVS_TAB = 256, 1024
KVS_LDS_MAX_V = 32 * ((48 * 1024) // 20)

BETA = 0.01
CASCADE_W = (2, 9, 129, 257)                                        # one block of the scan, and (257 > kVsBlock) two words to a thread
CASCADE_TAILS = (1, 31)


def _geometry(counts, prev_phi, U):
    counts = np.asarray(counts)
    V = counts.size
    W = (V + 31) // 32
    cz, pz, Uw = np.zeros(W * 32, bool), np.zeros(W * 32, bool), np.zeros(W * 32, np.float64)
    cz[:V], pz[:V], Uw[:V] = counts == 0, np.asarray(prev_phi) == 0.0, U
    return V, W, cz.reshape(W, 32), pz.reshape(W, 32), Uw.reshape(W, 32), int(np.sum(counts, dtype=np.int64))


# ---- the chain ------------------------------------------------------------------------------------------------------
def cascade_row(W, tail, beta, pi, zeros=None):
    """(counts, prev_phi, U) of V = 32 * W + tail cells; zeros = the old zeros under cells with a count (they only lift s0:
    by default enough that no round's s comes near 0)"""
    V = 32 * W + tail
    counts = np.full(V, 3, np.int32)
    first = 32 * np.arange(W)
    counts[first] = 0
    prev = np.full(V, 0.25)
    prev[first[0::2]] = 0.0
    counted = np.flatnonzero(counts)
    if zeros is None:
        zeros = min(counted.size - 7, W // 2 + 64)                  # a round's starts fall at most W / 2 under s0
    prev[counted[:zeros]] = 0.0
    U = np.full(V, 0.5)
    P = R.Probabilities(int(counts.sum()), beta, pi)
    s0 = int((prev == 0.0).sum())
    assert 0.0 < P(s0 - 1) < P(s0) < 1.0, "p does not increase from s0 - 1 to s0"
    s = s0
    for j in range(W):
        if j % 2 == 0:
            U[32 * j] = P(s)
            s -= 1
        else:
            U[32 * j] = np.nextafter(P(s), 2.0)
            s += 1
    return counts, prev, U


def cascade_group(W, tail, beta, pi):
    """three cascade rows of one length, s0 lifted by 0, 1 and 7 more old zeros: one call of the device's, a row per topic"""
    base = min(31 * W + tail - 7, W // 2 + 64)
    return [cascade_row(W, tail, beta, pi, zeros=base + more) for more in (0, 1, 7)]


def staircase_row(steps, up, beta, pi, lift=100, rest=200):
    """(counts, prev_phi, U): `steps` exact ties at the head of the row, `rest` cells with counts behind them, `lift` old zeros
    among those"""
    V = steps + rest
    counts = np.full(V, 2, np.int32)
    counts[:steps] = 0
    prev = np.full(V, 0.25)
    if not up:
        prev[:steps] = 0.0
    prev[steps:steps + lift] = 0.0
    U = np.full(V, 0.5)
    P = R.Probabilities(int(counts.sum()), beta, pi)
    s = int((prev == 0.0).sum())
    for v in range(steps):
        p = P(s)
        assert 0.0 < p < 1.0
        U[v] = np.nextafter(p, 2.0) if up else p
        s += 1 if up else -1
    return counts, prev, U


def window_report(counts, prev_phi, U, beta, pi):
    """R.rounds_chain with vs_chain_kernel's table rule.  dict(drawn, s_end, rounds, at_last, at_end, above = the lookups at
    ti == tn - 1, ti == tn, ti > tn (ti unsigned, as the kernel compares it), w0_clamped, tn_clamped = whether some round's
    window was clamped at 0 / at kVsTab)."""
    V, W, cz, pz, Uw, n_k = _geometry(counts, prev_phi, U)
    s0 = int(pz.sum())
    P = R.Probabilities(n_k, beta, pi)
    sw, und = np.full(W, s0, np.int64), np.zeros((W, 32), bool)
    s_min = s_max = s0
    rep = dict(rounds=0, at_last=0, at_end=0, above=0, w0_clamped=False, tn_clamped=False)
    live = [b for b in range(32) if cz[:, b].any()]
    while True:
        w0 = max(0, s_min - 32)
        tn = min(KVS_TAB, s_max + 32 - w0 + 1)
        rep["w0_clamped"] |= s_min - 32 < 0
        rep["tn_clamped"] |= s_max + 32 - w0 + 1 > KVS_TAB
        s, un = sw.copy(), np.zeros((W, 32), bool)
        for b in live:
            ti = (s - w0)[cz[:, b]]
            ti = np.where(ti < 0, ti + (1 << 32), ti)
            rep["at_last"] += int((ti == tn - 1).sum())
            rep["at_end"] += int((ti == tn).sum())
            rep["above"] += int((ti > tn).sum())
            with np.errstate(invalid="ignore"):
                above = Uw[:, b] > P.many(s)
            undrawn, kept = cz[:, b] & above, cz[:, b] & ~above
            s = s + (undrawn & ~pz[:, b]) - (kept & pz[:, b])
            un[:, b] = undrawn
        d = s - sw
        new_sw = s0 + np.concatenate(([0], np.cumsum(d)[:-1]))
        changed = bool((un != und).any()) or bool((new_sw != sw).any())
        und, sw = un, new_sw
        s_min, s_max = int(new_sw.min()), int(new_sw.max())
        rep["rounds"] += 1
        if not changed:
            break
        assert rep["rounds"] <= V + 2
    rep.update(drawn=~und.reshape(-1)[:V], s_end=s0 + int(d.sum()))
    return rep


WINDOW_CATEGORIES = ("at_last", "at_end", "above", "w0_clamped", "tn_clamped")


def window_rows(beta=BETA):
    """[(name, counts, prev_phi, U, pi)]: the rows of R.chain_cases whose lookups leave the table or whose window is clamped
    (V = 4097: the starts of a random row span thousands of values of s; V <= 65: s_min < 32), and the two staircases"""
    rows = [r for r in R.chain_cases(beta) if r[1].size == 4097 and (r[0].startswith("random") or r[0].startswith("s0 == V"))]
    rows += [r for r in R.chain_cases(beta) if r[0] in ("random V=65 pi=0.5", "s returns to 0 V=65")]
    for up in (False, True):
        rows.append(("staircase %s, 1100 ties" % ("up" if up else "down"),) + staircase_row(1100, up, beta, 0.5) + (0.5,))
    return rows


def long_row_inputs(V, K=3, seed=0):
    """counts, prev_phi [K][V] of R.random_row's kind for the long rows (V = 8193: two words to a thread of the scan, the last
    thread's stretch short; 16385: three; kVsLdsMaxV: the longest row in LDS; kVsLdsMaxV + 1: the shortest in global scratch)"""
    rng = np.random.default_rng(V + seed)
    rows = [R.random_row(rng, V) for _ in range(K)]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows])


LONG_V = (8193, 16385, KVS_LDS_MAX_V, KVS_LDS_MAX_V + 1)


# ---- the z step: a token without a candidate ------------------------------------------------------------------------
ALPHA = 0.1
SEED = 4242
ITERATION = 1
SCAN = 40
MIN_PER_CATEGORY = 8
EDGE_CATS = ("tie", "below", "above")


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(b):
    return float(np.int64(b).view(np.float64))


class Row:
    pass


class AliasEdge:
    def __init__(self, K, n_rows=48, n_zero=4, seed=1):
        self.K, self.J = K, 2 * SCAN + 1
        rng = np.random.default_rng(seed)
        tokens = [K + r for r in range(n_rows)]                     # document r is token r alone: its uniform is element r
        z0 = [int(t) for t in rng.integers(0, K, n_rows)]
        doc_ptr = list(range(n_rows + 1))
        zero_targets = []
        for r in range(n_zero):                                     # nw == 0 < nd: one-hot words around a word with a zero column
            topics = [int(t) for t in rng.permutation(K)[:3]]
            before, after = topics + topics[:2], topics[1:] + topics[:1]
            zero_targets.append(len(tokens) + len(before))
            tokens += before + [K + n_rows + r] + after
            z0 += before + [topics[0]] + after
            doc_ptr.append(len(tokens))
        self.doc_ptr, self.tokens, self.z0 = np.asarray(doc_ptr, np.int64), np.asarray(tokens, np.int32), np.asarray(z0, np.int32)
        self.V = K + n_rows + n_zero
        self.zero_targets = zero_targets
        U = O.uniforms(SEED, ITERATION, R.PURPOSE_Z, 0, len(tokens))
        self.U = U
        self.rows = []
        for r in range(n_rows):
            row = Row()
            row.word, row.target, row.U = K + r, r, float(U[r])
            row.ups = row.U * float(K)
            row.i = int(row.ups)
            row.frac = row.ups - float(row.i)
            assert row.i < K                                        # (1 - 2^-53) K rounds below K for these K: no ST_INVALID_TOPIC here
            row.shift = int(rng.integers(-SCAN // 2, SCAN // 2 + 1))
            self._solve(row, rng)
            self.rows.append(row)
        base = np.zeros((K, self.V))
        base[np.arange(K), np.arange(K)] = 1.0
        self._base = base
        self._base_tables = SR.alias_tables(base, ALPHA)
        self._base_lists = PS.word_lists(base)[1]
        self._survey, self._steps = None, {}

    def _table(self, col):
        return SR.alias_table(col * ALPHA)

    def _solve(self, row, rng):
        K, i, frac = self.K, row.i, row.frac
        col = rng.uniform(0.1, 1.0, K)
        row.kind, row.col, row.centre = "plain", col / (1.2 * col.max()), None
        if not 0.05 < frac < 0.95:
            return
        share = frac / K                                            # ps[w][i] = K pi_i / typeNorm for a share under 1 / K
        col[i] = share * (col.sum() - col[i]) / (1.0 - share)
        col /= 1.2 * col.max()

        def above(bits):
            c = col.copy()
            c[i] = _dbl(bits)
            return frac > float(self._table(c)[0][i])
        lo, hi = _bits(col[i] / 1.5), _bits(col[i] * 1.5)
        if not (above(lo) and not above(hi)):
            return
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if above(mid):
                lo = mid
            else:
                hi = mid
        row.kind, row.col, row.centre = "aimed", col, lo

    def column(self, row, j):
        if row.kind == "plain":
            return row.col
        c = row.col.copy()
        c[row.i] = _dbl(row.centre + (j - SCAN - row.shift))
        return c

    def phi(self, j):
        """Phi [K][V] of scan value j: the one-hot words, the rows' columns, the zero columns"""
        phi = self._base.copy()
        for row in self.rows:
            phi[:, row.word] = self.column(row, j)
        return phi

    def classify(self, row, j):
        """(category, the restatement's draw, dict(ps_i, a_i)) of a one-token row at scan value j"""
        ps, a, tn = self._table(self.column(row, j))
        new = R.token_draw(SR.DocState(self.K, []), self.column(row, j), np.flatnonzero(self.column(row, j)), ps, a, tn, row.U, self.K)
        ps_i, a_i = float(ps[row.i]), int(a[row.i])
        det = dict(ps_i=ps_i, a_i=a_i)
        if row.kind == "plain":
            return "plain", new, det
        if row.frac == ps_i:
            return "tie", new, det
        d = _bits(ps_i) - _bits(row.frac)
        if abs(d) <= 2:
            return ("below" if d > 0 else "above"), new, det
        return "far", new, det

    def survey(self):
        """dict(evals=[row][j] -> (category, draw, det), values[category] = scan values, rows[category] = rows with at least one)"""
        if self._survey is None:
            evals = [[self.classify(row, j) for j in range(self.J)] for row in self.rows]
            values, rows = {}, {}
            for ev in evals:
                for cat in {e[0] for e in ev}:
                    rows[cat] = rows.get(cat, 0) + 1
                for e in ev:
                    values[e[0]] = values.get(e[0], 0) + 1
            self._survey = dict(evals=evals, values=values, rows=rows)
        return self._survey

    def restatement_z(self, j):
        """(z, stats [4], trace) of the restatement's whole step with Phi matrix j"""
        if j not in self._steps:
            phi = self.phi(j)
            ps, a, tn = (t.copy() for t in self._base_tables)
            lists = list(self._base_lists)
            for row in self.rows:
                ps[row.word], a[row.word], tn[row.word] = self._table(phi[:, row.word])
                lists[row.word] = np.flatnonzero(phi[:, row.word] != 0.0).astype(np.int64)
            z, stats, trace = self.z0.astype(np.int64), np.zeros(4, np.int64), []
            R.z_step(self.doc_ptr, self.tokens, z, phi, (ps, a, tn), lists, SEED, ITERATION, stats=stats, trace=trace)
            self._steps[j] = (z, stats, trace)
        return self._steps[j]


_built = {}


def alias_fixture(K):
    """the rows without a candidate at K = 8 or K = 160, built once per process and left unchanged"""
    if K not in _built:
        _built[K] = AliasEdge(K, seed=K)
    return _built[K]
