"""Knife-edge rows for the token step of scheme=lightpclda (a test helper, not collected; the manner of
tests/spalias_knife_edge.py).

The token step (LightPCLDA.java:131-201, tests/lightpclda_restatement.token_step) makes five comparisons:

  a  alias cell      frac = U1 * K - i          >  ps[w][i]                         (the word proposal: a[w][i] or i)
  b  word accept     U2                         <  pi_w = (alpha[s] + ni[t]) / (alpha[s] + ni[s])
  c  length branch   ui = U3 * (len + alphaSum) <  len                              (z[(int)ui], or the alpha branch)
  d  alpha cell      (int)(((ui - len) / alphaSum) * K)  on either side of an integer m
  e  doc accept      U4                         <  ratio = nom / den                (three roundings each)

A row is a document of its own.  Word k < K has a one-hot Phi column (phi[k][k] = 1): a token of it, on topic k, keeps
k (its table proposes only k; a document proposal t != k has phi[t][k] = 0, so nom = 0 and nothing accepts; t == k
leaves z0).  Every token of a row but one is such a token, so the counts at the TARGET token are what the builder laid
down and do not move during the step.  The target has a word of its own with a full positive column; its uniforms are
known from the stream (R.token_uniforms(seed, iteration, global index)).  Its comparison is then put on the edge:

  PhiEdges    a and e: the knob is one entry of the target word's column (phi[i][w] for a; phi[dt][w] or phi[s][w] for
              e), bisected on its bit pattern for the flip of the comparison and scanned over 2 * SCAN + 1 neighbouring
              doubles, scan value j into Phi matrix j: one set_phi and one z step per matrix, all from the same z and
              iteration, so every row keeps its uniforms.  K = 8, alpha asymmetric (so that alpha[wp] after an accepted
              word proposal is not alpha[z0]).  a rows take a target whose frac is at least 0.5: below that ps moves on a
              2^-53 grid while frac's neighbours are closer, and only ties could be reached.
  AlphaEdges  b, c and d: counts are integers, so the knob is alpha.  A b row owns a topic s_r (only its document uses
              it; the target sits on it) and alpha[s_r] is solved so that pi_w is pred(U2), U2 or succ(U2); c and d rows
              move alphaSum through the alpha of a slack topic (the last one, which no row uses) so that ui is
              pred(len), len, succ(len), or ((ui - len) / alphaSum) * K is pred(m), m, succ(m).  alphaSum is global: one
              c or d row is aimed per alpha VECTOR, and every vector is a handle of its own (N_VECTORS <= MAX_HANDLES).
              Vector v carries tag TAGS[v % 3] for its c or d row and for all b rows.  Ties of d are reached for
              m = 1, 12, 16 and 24 of K = 25 (first, two middle ones, last); where K * ulp(x) exceeds the spacing of
              the doubles at m (m = 13 .. 15) they are not, and no row aims there (AlphaEdges.CELLS).

Tags: "tie" the computed side equals the uniform or bound; "below" / "above" it is the neighbouring double under / over
it.  A (row, scan value or vector) counts only where forcing the comparison one way and the other gives two different
new topics for the target (`useful`): an edge that cannot show in z is no test.

step() is the builder's own arithmetic of the token step -- plain Python floats, written apart from the restatement --
with switchable slips (SLIPS) and with `force` (a comparison's outcome imposed).  The builder asserts through the
restatement that no other token moves under any matrix or vector and that the restatement draws what step() predicts at
every target."""
import numpy as np

from tests import lightpclda_restatement as R
from tests import spalias_restatement as SR

K = 8
ALPHA = np.array([0.1, 0.12, 0.08, 0.1, 0.15, 0.1, 0.09, 0.11])     # PhiEdges; AlphaEdges: 0.1 but for the knobs
BETA = 0.01
SEED = 4242
ITERATION = 1
SCAN = 32
TAGS = ("below", "tie", "above")
SOURCES = ("alpha", "old", "chunk", "earlier")                      # where dt came from (e rows)
MIN_PER_CATEGORY = 8                                                # a, b, e: rows per (comparison, tag)
MIN_ALPHA_ROWS = 4                                                  # c, d: rows per tag (each costs a handle)
MIN_PER_SOURCE = 4                                                  # e: rows per (dt source, state)
MAX_HANDLES = 32
N_VECTORS = 24
OUT_OF_BOUNDS = -1                                                  # step(): a slip indexed z[len]

# slip -> the comparison it belongs to
SLIPS = {"assoc": "e", "div_first": "e", "alias_ge": "a", "word_le": "b", "doc_le": "e", "len_le": "c", "cell_mul_first": "d",
         "alpha_z0": "e"}
ORDER_SLIPS = tuple(s for s in SLIPS if s != "alpha_z0")            # must not show on random data


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(b):
    return float(np.int64(b).view(np.float64))


def _next(x, up):
    return float(np.nextafter(x, np.inf if up else -np.inf))


def tag_of(computed, bound):
    if computed == bound:
        return "tie"
    if computed == _next(bound, False):
        return "below"
    if computed == _next(bound, True):
        return "above"
    return None


def _div(a, b):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(a) / np.float64(b))


def step(n, zdoc, pos, phi_w, alpha, alpha_total, ps_w, a_w, U, slip=None, force=None, detail=None):
    """The new topic of the token at pos; n (the document's histogram, the token counted) and zdoc are left alone.
    slip: one of SLIPS.  force = (comparison, outcome): "alias" / "word" / "len" / "doc" with a bool, "cell" with the
    alpha-branch topic."""
    nK = len(n)
    fK = float(nK)
    U1, U2, U3, U4 = U
    fname, fval = force if force is not None else (None, None)
    z0 = s = int(zdoc[pos])
    ups = U1 * fK
    i = int(ups)
    if i >= nK:
        raise R.InvalidTopic("alias draw reaches K")
    frac = ups - float(i)
    up = frac >= ps_w[i] if slip == "alias_ge" else frac > ps_w[i]
    if fname == "alias":
        up = fval
    wp = int(a_w[i]) if up else i
    flen = float(len(zdoc))
    ui = U3 * (flen + alpha_total)
    inside = ui <= flen if slip == "len_le" else ui < flen
    if fname == "len":
        inside = fval
    idx = v = None
    if inside:
        idx = min(int(ui), len(zdoc) - 1) if fname == "len" else int(ui)
        if idx >= len(zdoc):
            return OUT_OF_BOUNDS
        dt = int(zdoc[idx])
    else:
        v = (ui - flen) * fK / alpha_total if slip == "cell_mul_first" else ((ui - flen) / alpha_total) * fK
        dt = int(v)
        if fname == "cell":
            dt = fval
        dt = max(dt, 0) if fname == "len" else dt
        if dt >= nK:
            raise R.InvalidTopic("alpha branch reaches K")
    cnt = list(n)
    pi_w = ratio = None
    acc_w = acc_d = False
    if wp != s:
        pi_w = (alpha[s] + float(cnt[wp])) / (alpha[s] + float(cnt[s] - 1))
        acc_w = pi_w > 1.0 or (U2 <= pi_w if slip == "word_le" else U2 < pi_w)
        if fname == "word":
            acc_w = fval
        if acc_w:
            cnt[s] -= 1
            cnt[wp] += 1
            s = wp
    new = z0
    if dt != s:
        a_s = alpha[z0] if slip == "alpha_z0" else alpha[s]
        x1, x2 = a_s + float(cnt[dt]), a_s + float(cnt[s])          # ni[t] = n[t]: t is not s
        y1, y2 = a_s + float(cnt[s] - 1), a_s + float(cnt[dt])
        if slip == "assoc":
            ratio = _div(phi_w[dt] * (x1 * x2), phi_w[s] * (y1 * y2))
        elif slip == "div_first":
            ratio = _div(phi_w[dt], phi_w[s]) * _div(x1 * x2, y1 * y2)
        else:
            ratio = _div(phi_w[dt] * x1 * x2, phi_w[s] * y1 * y2)
        acc_d = ratio > 1.0 or (U4 <= ratio if slip == "doc_le" else U4 < ratio)
        if fname == "doc":
            acc_d = fval
        new = dt if acc_d else s
    if detail is not None:
        detail.update(cell=i, frac=frac, ps=float(ps_w[i]), up=up, word=wp, pi_w=pi_w, acc_w=acc_w, ui=ui, inside=inside, idx=idx, v=v, doc=dt,
                      s=s, ratio=ratio, acc_d=acc_d, new=new)
    return new


def z_step(doc_ptr, tokens, z, phi, alpha, tables, seed, iteration, slip=None, uniforms=None):
    """R.z_step with step(): one z step in place on z; returns how many tokens left the array's bounds (a slip can)."""
    ps, a, _ = tables
    nK = phi.shape[0]
    alpha = [float(x) for x in np.broadcast_to(np.asarray(alpha, np.float64), (nK,))]
    total = R.alpha_sum(alpha, nK)
    phiT = np.ascontiguousarray(phi.T)
    out = 0
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        zdoc = [int(k) for k in z[b:e]]
        n = [0] * nK
        for k in zdoc:
            n[k] += 1
        for pos in range(e - b):
            w = int(tokens[b + pos])
            U = uniforms[b + pos] if uniforms is not None else R.token_uniforms(seed, iteration, b + pos)
            try:
                new = step(n, zdoc, pos, phiT[w], alpha, total, ps[w], a[w], U, slip)
            except R.InvalidTopic:
                new = nK - 1
            if new == OUT_OF_BOUNDS:
                out += 1
                continue
            n[zdoc[pos]] -= 1
            n[new] += 1
            zdoc[pos] = new
        z[b:e] = zdoc
    return out


def dt_source(idx, pos):
    if idx is None:
        return "alpha"
    if idx >= pos:
        return "old"
    return "chunk" if idx >= pos - pos % 64 else "earlier"


def _bisect(f, lo, hi):
    """lo, hi: bit patterns with f(lo) != f(hi); returns adjacent (lo, lo + 1) that still differ, or None."""
    flo = f(_dbl(lo))
    if flo == f(_dbl(hi)):
        return None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if f(_dbl(mid)) == flo:
            lo = mid
        else:
            hi = mid
    return lo


class Row:
    kind = "plain"
    tags = None


class _Edges:
    """What both builders share: the corpus of one-hot tokens around one target per document, and the checks."""

    def _layout(self, lens):
        self.doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        N = int(self.doc_ptr[-1])
        self.U = [R.token_uniforms(SEED, ITERATION, t) for t in range(N)]
        self.tokens = np.zeros(N, np.int32)
        self.z0 = np.zeros(N, np.int32)
        self.rows = []

    def _row(self, d, pos, zdoc):
        """the document d gets its tokens: one-hot words on zdoc's topics, the target at pos with word nK + d"""
        row = Row()
        row.doc, row.beg, row.pos = d, int(self.doc_ptr[d]), pos
        row.target = row.beg + pos
        row.word = self.nK + d
        row.zdoc = [int(k) for k in zdoc]
        row.n = np.bincount(row.zdoc, minlength=self.nK).tolist()
        row.U = self.U[row.target]
        row.tags = {}
        self.tokens[row.beg:row.beg + len(zdoc)] = zdoc
        self.tokens[row.target] = row.word
        self.z0[row.beg:row.beg + len(zdoc)] = zdoc
        self.rows.append(row)
        return row

    def eval(self, row, col, alpha, total=None, slip=None, force=None):
        """(new topic or None where Java would throw, detail) of the row's target with column col"""
        alpha = [float(x) for x in alpha]
        ps, a, _ = SR.alias_table(np.asarray(col) * np.asarray(alpha))
        det = {}
        try:
            new = step(row.n, row.zdoc, row.pos, col, alpha, R.alpha_sum(alpha, self.nK) if total is None else total, ps, a, row.U, slip, force, det)
        except R.InvalidTopic:
            new = None
        return new, det

    FORCES = {"a": "alias", "b": "word", "c": "len", "e": "doc"}

    def useful(self, row, col, alpha, det):
        """the row's comparison forced one way and the other moves the target's new topic"""
        if row.kind == "d":
            sides = [("cell", row.m - 1), ("cell", row.m)]
        else:
            sides = [(self.FORCES[row.kind], False), (self.FORCES[row.kind], True)]
        return self.eval(row, col, alpha, force=sides[0])[0] != self.eval(row, col, alpha, force=sides[1])[0]

    def sides(self, row, det):
        """(the computed side, the uniform or bound) of the row's comparison, or None where the step did not make it"""
        if row.kind == "a":
            return (det["ps"], det["frac"]) if det["cell"] == row.cell else None
        if row.kind == "b":
            return (det["pi_w"], row.U[1]) if det["pi_w"] is not None and det["word"] == row.t else None
        if row.kind == "c":
            return det["ui"], float(len(row.zdoc))
        if row.kind == "d":
            return (det["v"], float(row.m)) if det["v"] is not None else None
        if row.kind == "e":
            return (det["ratio"], row.U[3]) if det["ratio"] is not None and (det["s"], det["doc"]) == (row.s, row.dt) else None
        return None

    def outcome(self, row, det):
        """which way the row's comparison went"""
        return {"a": det["up"], "b": det["acc_w"], "c": det["inside"], "d": det["doc"], "e": det["acc_d"]}[row.kind]

    def check_step(self, phi, alpha, what):
        """The restatement's z step over the whole corpus: nothing but targets moves, and every target lands where
        step() says.  Returns (z, the three counters), or None where the restatement raises what Java would throw."""
        z = self.z0.astype(np.int64)
        tables = SR.alias_tables(phi, alpha)
        try:
            stats = R.z_step(self.doc_ptr, self.tokens, z, phi, alpha, tables, SEED, ITERATION)
        except R.InvalidTopic:
            return None
        moved = np.flatnonzero(z != self.z0)
        targets = {row.target: row for row in self.rows}
        assert all(int(t) in targets for t in moved), "%s: a one-hot token moved: %s" % (what, moved[:8])
        for row in self.rows:
            want, _ = self.eval(row, phi[:, row.word], np.broadcast_to(alpha, (self.nK,)))
            assert want == z[row.target], "%s: the restatement draws %d at token %d (%s row), the builder %s" % (
                what, z[row.target], row.target, row.kind, want)
        return z, np.asarray(stats, np.int64)

    def describe(self, row):
        return "%s row, token %d (document %d, position %d of %d)" % (row.kind, row.target, row.doc, row.pos, len(row.zdoc))


class PhiEdges(_Edges):
    """a and e rows: K = 8, one Phi matrix per scan value."""
    nK = K
    alpha = ALPHA

    def __init__(self, n_short=100, n_long=20, seed=1):
        rng = np.random.default_rng(seed)
        lens = np.concatenate((rng.integers(3, 13, n_short), rng.integers(66, 73, n_long - 4), rng.integers(128, 132, 4)))
        self._layout(lens)
        self.V = K + len(lens)
        self.total = R.alpha_sum(ALPHA, K)
        short_plan = ("a", "alpha", "a", "old", "a", "chunk", "alpha")
        long_plan = ("earlier", "chunk", "old", "earlier")
        for d, L in enumerate(int(x) for x in lens):
            want = short_plan[d % len(short_plan)] if d < n_short else long_plan[d % len(long_plan)]
            order = list(rng.permutation(L)) if d < n_short else [p for p in [(64, 127, 63, 0)[(d + i) % 4] for i in range(4)] if p < L] + \
                list(65 + rng.permutation(L - 65))
            pos = None
            for p in order:
                U = self.U[int(self.doc_ptr[d]) + int(p)]
                f = U[0] * K - int(U[0] * K)
                if want == "a" and 0.5 <= f <= 0.97:
                    pos = int(p)
                    break
                if want != "a" and 0.05 <= U[3] <= 0.95 and self._source(L, int(p), U[2]) == want:
                    pos = int(p)
                    break
            if pos is None:
                want, pos = "plain", int(order[0])
            if want == "a":
                row = self._aim_a(d, L, pos, rng)
            elif want == "plain":
                row = self._plain(d, L, pos, rng)
            else:
                row = self._aim_e(d, L, pos, rng, after=bool((d // 2) % 2))
            self._classify(row)
        self.checked = {}

    def _source(self, L, pos, U3):
        ui = U3 * (float(L) + self.total)
        return dt_source(int(ui) if ui < float(L) else None, pos)

    def _plain(self, d, L, pos, rng):
        row = self._row(d, pos, rng.integers(0, K, L))
        row.cols = [rng.uniform(0.2, 1.0, K)] * (2 * SCAN + 1)
        return row

    def _scan(self, row, col, knob, f, width):
        """bisect col[knob] for the flip of f, then the scan columns; False where there is no flip to find"""
        def at(x):
            c = col.copy()
            c[knob] = x
            return f(c)
        lo = _bisect(at, _bits(col[knob] * (1.0 - width)), _bits(col[knob] * (1.0 + width)))
        if lo is None:
            return False
        row.knob, row.cols = knob, []
        for j in range(-SCAN, SCAN + 1):
            c = col.copy()
            c[knob] = _dbl(lo + j)
            row.cols.append(c)
        return True

    def _aim_a(self, d, L, pos, rng):
        U = self.U[int(self.doc_ptr[d]) + pos]
        i = int(U[0] * K)
        frac = U[0] * K - i
        for _ in range(20):
            topics = rng.permutation(K)
            zdoc = topics[1:5][rng.integers(0, 4, L)]
            zdoc[pos] = topics[0]                                   # alone on its topic: ni[z0] = 0, every word proposal accepts
            col = rng.uniform(0.2, 1.0, K)
            ui = U[2] * (float(L) + self.total)                     # the document proposal gets a small phi: neither side accepts it
            dt = int(zdoc[int(ui)]) if ui < float(L) else min(int(((ui - float(L)) / self.total) * K), K - 1)
            if dt != i:
                col[dt] = rng.uniform(1e-3, 2e-3)
            f = frac / K                                            # ps[i] = K * pi[i] / typeNorm for a low cell
            col[i] = float(np.sum(np.delete(col * ALPHA, i))) * f / (1.0 - f) / ALPHA[i]
            row = self._row(d, pos, zdoc) if _ == 0 else self._reuse(row, zdoc)
            row.kind, row.cell = "a", i
            if self._scan(row, col, i, lambda c: self.eval(row, c, ALPHA)[1]["up"], 1e-3):
                return row
        row.kind = "plain"
        row.cols = [col] * (2 * SCAN + 1)
        return row

    def _reuse(self, row, zdoc):
        self.rows.pop()
        return self._row(row.doc, row.pos, zdoc)

    def _aim_e(self, d, L, pos, rng, after):
        U = self.U[int(self.doc_ptr[d]) + pos]
        row = None
        for attempt in range(40):
            topics = rng.permutation(K)[:4]
            zdoc = topics[rng.integers(0, 4, L)]
            col = rng.uniform(0.2, 1.0, K)
            ps, a, _ = SR.alias_table(col * ALPHA)
            wp = SR.alias_sample(ps, a, U[0])
            others = np.bincount(np.delete(zdoc, pos), minlength=K)
            if after:                                               # a topic no fuller than wp's: pi_w >= 1
                cand = [k for k in range(K) if k != wp and others[k] <= others[wp]]
                zdoc[pos] = cand[int(rng.integers(len(cand)))]
            elif attempt % 2:
                zdoc[pos] = wp                                      # no word step at all
            row = self._row(d, pos, zdoc) if row is None else self._reuse(row, zdoc)
            row.kind = "e"
            new, det = self.eval(row, col, ALPHA)
            if det["ratio"] is None or det["acc_w"] != after:
                continue
            row.s, row.dt = det["s"], det["doc"]
            knob = row.dt if (d % 3) else row.s
            ok = False
            for _ in range(8):                                      # the knob moves the table too: until the state holds
                r = det["ratio"]
                col[knob] *= U[3] / r if knob == row.dt else r / U[3]
                new, det = self.eval(row, col, ALPHA)
                if det["ratio"] is None or (det["s"], det["doc"], det["acc_w"]) != (row.s, row.dt, after) or not 1e-3 < col[knob] < 1e3:
                    break
                if abs(det["ratio"] / U[3] - 1.0) < 1e-9:
                    ok = True
                    break
            if ok and self._scan(row, col, knob, lambda c: self.eval(row, c, ALPHA)[1]["acc_d"], 1e-6):
                row.after, row.source = after, dt_source(det["idx"], pos)
                return row
        row.kind = "plain"
        row.cols = [col] * (2 * SCAN + 1)
        return row

    def _classify(self, row):
        """row.tags[j] for the scan values on the edge; a row without a useful flip pair is a plain row"""
        if row.kind == "plain":
            return
        prev, pair = None, False
        for j, col in enumerate(row.cols):
            _, det = self.eval(row, col, ALPHA)
            sd = self.sides(row, det)
            if sd is None or not self.useful(row, col, ALPHA, det):
                prev = None
                continue
            out = self.outcome(row, det)
            pair |= prev is not None and prev != out
            prev = out
            t = tag_of(*sd)
            if t is not None:
                row.tags[j] = t
        if not pair or not row.tags:                                # (a flip whose two sides are both further than a neighbour: not counted)
            row.kind, row.tags = "plain", {}

    def phi(self, j):
        """Phi [K][V] of scan value j in [0, 2 * SCAN]"""
        phi = np.zeros((K, self.V))
        phi[np.arange(K), np.arange(K)] = 1.0
        for row in self.rows:
            phi[:, row.word] = row.cols[j]
        return phi

    def restatement(self, j):
        if j not in self.checked:
            self.checked[j] = self.check_step(self.phi(j), ALPHA, "Phi matrix %d" % j)
        return self.checked[j]

    def label(self, row, j):
        return (row.kind, row.tags.get(j, "-"), getattr(row, "source", "-"))

    def survey(self):
        """counts[(comparison, tag)] and, for e, counts[("e", source, after)]: rows, not (row, scan value) pairs"""
        counts = {}
        for row in self.rows:
            if row.kind == "plain":
                continue
            for t in set(row.tags.values()):
                counts[(row.kind, t)] = counts.get((row.kind, t), 0) + 1
            if row.kind == "e":
                counts[("e", row.source, row.after)] = counts.get(("e", row.source, row.after), 0) + 1
        return counts


class AliasRows(PhiEdges):
    """The a rows alone as one-token documents: what spalias draws through its empty-list path (x = U1, the same table)."""

    def __init__(self, n_docs=60, seed=2):
        rng = np.random.default_rng(seed)
        self._layout(np.ones(n_docs, np.int64))
        self.V = K + n_docs
        self.total = R.alpha_sum(ALPHA, K)
        for d in range(n_docs):
            f = self.U[d][0] * K - int(self.U[d][0] * K)
            row = self._aim_a(d, 1, 0, rng) if 0.5 <= f <= 0.97 else self._plain(d, 1, 0, rng)
            if row.kind == "a":
                self._classify_alias(row)
        self.checked = {}

    def _classify_alias(self, row):
        for j, col in enumerate(row.cols):
            ps, a, _ = SR.alias_table(col * ALPHA)
            t = tag_of(float(ps[row.cell]), row.U[0] * K - row.cell)
            if t is not None:
                row.tags[j] = t

    def spalias_z(self, j):
        """what spalias draws: the alias draw at U1 (the list of a one-token document is empty once the token has left)"""
        phi = self.phi(j)
        z = self.z0.astype(np.int64)
        SR.z_step(self.doc_ptr, self.tokens, z, phi, SR.alias_tables(phi, ALPHA), SEED, ITERATION)
        for row in self.rows:
            ps, a, _ = SR.alias_table(row.cols[j] * ALPHA)
            assert z[row.target] == SR.alias_sample(ps, a, row.U[0])
        return z


class AlphaEdges(_Edges):
    """b, c and d rows: one Phi, N_VECTORS alpha vectors."""
    NB = 16
    nK = K + NB + 1
    SLACK = nK - 1
    # d: the integer m between cells m - 1 and m -- first, two middle ones, last.  v = x * K with x = (ui - len) / alphaSum
    # moves in steps of K * ulp(x); for m = 13 .. 15 at K = 25 (x in [0.5, 1): steps of 25 * 2^-53, doubles at m 2^-49 apart)
    # the step is coarser than the doubles at m and pred(m), m, succ(m) are not all reached: those m are not aimed at
    CELLS = (1, nK // 2, 16, nK - 1)
    WINDOW = 4096

    def __init__(self, n_c=40, n_d=90, seed=3):
        rng = np.random.default_rng(seed)
        nK, NB = self.nK, self.NB
        lens = np.concatenate((rng.integers(4, 9, NB), rng.integers(4, 13, n_c), rng.integers(4, 15, n_d)))
        self._layout(lens)
        self.V = nK + len(lens)
        self.cols = {}
        # b rows: alpha[s_r] for each tag
        self.b_alpha = {t: np.full(nK, 0.1) for t in TAGS}
        for d in range(NB):
            self._aim_b(d, int(lens[d]), rng)
        S = {t: R.alpha_sum(self.b_alpha[t][:nK - 1], nK - 1) for t in TAGS}
        # c and d rows: candidates in document order until four of each carry all three tags
        self.vectors, self.aimed = [], []
        cands = {"c": list(range(NB, NB + n_c)), "d": list(range(NB + n_c, len(lens)))}
        for kind in ("c", "d"):
            for q in range(MIN_ALPHA_ROWS):
                while True:
                    assert cands[kind], "too few candidates for %s rows" % kind
                    d = cands[kind].pop(0)
                    got = self._aim_cd(kind, d, int(lens[d]), rng, S, self.CELLS[q])
                    if got is not None:
                        break
                    self._plain(d, int(lens[d]), rng)
                row, slack = got
                for t in TAGS:
                    vec = self.b_alpha[t].copy()
                    vec[self.SLACK] = slack[t]
                    self.vectors.append(vec)
                    self.aimed.append(row)
        for kind in ("c", "d"):
            for d in cands[kind]:
                self._plain(d, int(lens[d]), rng)
        assert len(self.vectors) == N_VECTORS <= MAX_HANDLES
        self.rows.sort(key=lambda r: r.doc)
        self.phi = np.zeros((nK, self.V))
        self.phi[np.arange(nK), np.arange(nK)] = 1.0
        for row in self.rows:
            self.phi[:, row.word] = self.cols[row.doc]
        for v in range(N_VECTORS):
            self._classify(v)
        for row in self.rows:                                       # a flip pair is mandatory: "above" accepts, the other two do not
            have = set(row.tags.values())
            if row.kind == "b" and not ("above" in have and len(have) > 1):
                row.kind, row.tags = "plain", {}
        self.checked = {}

    def _plain(self, d, L, rng):
        row = self._row(d, int(rng.integers(L)), rng.integers(0, K, L))
        self.cols[d] = rng.uniform(0.2, 1.0, self.nK)
        return row

    def _aim_b(self, d, L, rng):
        """target on its own topic s_r with ns companions, the word proposal t with nt < ns tokens: pi_w runs from
        nt / ns to 1 as alpha[s_r] grows"""
        s_r = K + d
        pick = None
        for p in range(L):                                          # nt == 0 first: alpha[s_r] alone then moves pi_w, in steps of its own ulp
            U2 = self.U[int(self.doc_ptr[d]) + p][1]
            for ns in range(1, L):
                for nt in range(0, min(ns, L - ns)):
                    a0 = (U2 * ns - nt) / (1.0 - U2)
                    if 0.02 <= a0 <= 1.0 and (pick is None or (nt > 0, a0) < (pick[1] > 0, pick[2])):
                        pick = (ns, nt, a0, p)
        pos = pick[3] if pick is not None else 0
        U = self.U[int(self.doc_ptr[d]) + pos]
        t = int(rng.integers(K))
        col = rng.uniform(1e-3, 2e-3, self.nK)
        col[t] = 1.0
        self.cols[d] = col
        if pick is None:
            self._row(d, pos, rng.integers(0, K, L))
            return
        ns, nt, a0, _ = pick
        fill = (t + 1 + int(rng.integers(K - 1))) % K
        zdoc = [s_r] * ns + [t] * nt + [fill] * (L - 1 - ns - nt)
        zdoc = [zdoc[i] for i in rng.permutation(L - 1)]
        zdoc.insert(pos, s_r)
        row = self._row(d, pos, zdoc)
        row.kind, row.t, row.s_r = "b", t, s_r
        pi = lambda a: (a + float(nt)) / (a + float(ns))            # noqa: E731
        lo = _bisect(lambda a: U[1] < pi(a), _bits(a0 * 0.999), _bits(a0 * 1.001))
        if lo is None:
            row.kind = "plain"
            return
        centre = _dbl(lo)
        want = {"below": _next(U[1], False), "tie": U[1], "above": _next(U[1], True)}
        for tg in TAGS:
            self.b_alpha[tg][s_r] = centre
        h = float(np.spacing(centre + float(ns))) / 2.0             # the grid of the two sums, and alpha's own
        for a in [_dbl(lo + j) for j in sorted(range(-2048, 2049), key=abs)] + [centre + j * h for j in sorted(range(-512, 513), key=abs)]:
            for tg in TAGS:
                if pi(a) == want[tg] and self.b_alpha[tg][s_r] == centre:
                    self.b_alpha[tg][s_r] = a

    def _aim_cd(self, kind, d, L, rng, S, m):
        """A target whose U3 puts ui on len (c) or the alpha-branch cell on m (d) at an alphaSum above every vector's
        sum without the slack topic; the slack alpha per tag, or None."""
        nK, fL = self.nK, float(L)
        floor = max(S.values()) + 0.01
        best = None
        for pos in range(L - 1):                                    # not the last token: c's index branch reads z[len - 1]
            U3 = self.U[int(self.doc_ptr[d]) + pos][2]
            A0 = fL * (1.0 - U3) / U3 if kind == "c" else (fL * (1.0 - U3) / (U3 - m / float(nK)) if U3 > m / float(nK) else -1.0)
            if floor < A0 <= 40.0:
                best = (pos, U3, A0)
                break
        if best is None:
            return None
        pos, U3, A0 = best
        if kind == "c":
            val, bound = (lambda A: U3 * (fL + A)), fL
        else:
            val, bound = (lambda A: ((U3 * (fL + A) - fL) / A) * float(nK)), float(m)
        lo = _bisect(lambda A: val(A) < bound, _bits(A0 * 0.999), _bits(A0 * 1.001))
        if lo is None:
            return None
        want = {"below": _next(bound, False), "tie": bound, "above": _next(bound, True)}
        slack = {}
        for tg in TAGS:
            for j in sorted(range(-self.WINDOW, self.WINDOW + 1), key=abs):
                A = _dbl(lo + j)
                if val(A) != want[tg]:
                    continue
                a = A - S[tg]
                for k in (0, 1, -1, 2, -2):                         # the k-order sum ends with the slack topic
                    ak = _dbl(_bits(a) + k)
                    if S[tg] + ak == A:
                        slack[tg] = ak
                        break
                if tg in slack:
                    break
            if tg not in slack:
                return None
        # the target's topic has a small phi, the two topics the edge separates a large one: both sides accept
        others = [k for k in range(1, K) if kind == "c" or k not in (m - 1, m)]
        z0 = others.pop(int(rng.integers(len(others))))
        zdoc = [others[int(rng.integers(3))] for _ in range(L)]
        zdoc[pos] = z0
        col = rng.uniform(0.2, 0.5, nK)
        col[z0] = 0.01
        if kind == "c":
            col[0] = col[zdoc[L - 1]] = 1.0
        else:
            col[m - 1] = col[m] = 1.0
        self.cols[d] = col
        row = self._row(d, pos, zdoc)
        row.kind, row.m = kind, m
        return row, slack

    def _classify(self, v):
        alpha = self.vectors[v]
        for row in self.rows:
            if row.kind == "plain" or (row.kind != "b" and row is not self.aimed[v]):
                continue
            col = self.cols[row.doc]
            _, det = self.eval(row, col, alpha)
            sd = self.sides(row, det)
            if sd is None or not self.useful(row, col, alpha, det):
                continue
            t = tag_of(*sd)
            if t is not None:
                row.tags[v] = t

    def restatement(self, v):
        if v not in self.checked:
            self.checked[v] = self.check_step(self.phi, self.vectors[v], "alpha vector %d" % v)
        return self.checked[v]

    def label(self, row, v):
        return (row.kind, row.tags.get(v, "-"), "-")

    def survey(self):
        counts = {}
        for row in self.rows:
            for t in set(row.tags.values()):
                counts[(row.kind, t)] = counts.get((row.kind, t), 0) + 1
        return counts


# ---- the random corpus of tests/test_lightpclda_gpu.py::test_ragged_corpus ------------------------------------------
RAGGED = dict(K=7, V=5, alpha=0.3, beta=0.1, seed=777, zseed=5, sweeps=12)
RAGGED_SOURCES = ("own", "later", "chunk", "earlier", "alpha")


def ragged_corpus():
    """(doc_ptr, tokens): documents of 0 and 1 tokens, 63, 64 and 65 (chunk boundaries), 130 and 700 tokens over V = 5"""
    rng = np.random.default_rng(3)
    lens = np.array([63, 0, 1, 64, 700, 65, 1, 130, 0, 2], np.int64)
    tokens = rng.integers(0, 5, lens.sum()).astype(np.int32)
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens


def ragged_model(z0):
    doc_ptr, tokens = ragged_corpus()
    g = RAGGED
    m = R.Model(g["K"], g["V"], g["alpha"], g["beta"], g["seed"], doc_ptr, tokens, z0)
    m.init_phi()
    return m


def count_dt_sources(m, counts):
    """One z step of the restatement's model m walked token by token (m itself is left alone): counts[(source, after an
    accepted word proposal)] += the tokens whose document proposal came from there.  Returns z after the step."""
    z = m.z.copy()
    alpha = np.broadcast_to(np.asarray(m.alpha, np.float64), (m.K,))
    total = R.alpha_sum(alpha, m.K)
    for d in range(len(m.doc_ptr) - 1):
        b, e = int(m.doc_ptr[d]), int(m.doc_ptr[d + 1])
        zdoc, n = [int(k) for k in z[b:e]], np.bincount(z[b:e], minlength=m.K).tolist()
        for pos in range(e - b):
            det = {}
            w = int(m.tokens[b + pos])
            R.token_step(n, zdoc, pos, m.phi[:, w], alpha, total, m.tables[0][w], m.tables[1][w],
                         R.token_uniforms(m.seed, m.iteration + 1, m.tok_base + b + pos), det)
            idx = det["idx"]
            src = "alpha" if idx is None else "own" if idx == pos else "later" if idx > pos else "chunk" if idx >= pos - pos % 64 else "earlier"
            counts[(src, det["acc_w"])] = counts.get((src, det["acc_w"]), 0) + 1
        z[b:e] = zdoc
    return z


_cache = {}


def edges(name):
    """the builders' results, built once per process: "phi", "alpha", "alias" """
    if name not in _cache:
        _cache[name] = {"phi": PhiEdges, "alpha": AlphaEdges, "alias": AliasRows}[name]()
    return _cache[name]
