"""Knife-edge rows for the doubly sparse z step of scheme=polyaurn_sparse, and a numpy model of the kernel's proposal (a
test helper, not collected; the manner of tests/spalias_knife_edge.py).

A row is a document of its own: a prefix of tokens whose words have one-hot Phi columns (word k: phi[k] = 1: such a token
keeps its topic k on either list and on either branch) and one TARGET token, last, with a word of its own.  The prefix is
simulated with DocState, so the document's list at the target is in the kernel's order; the target's uniform U is known
from the oracle's stream; the target word's Phi column is then solved so that the draw sits on an edge.  The candidates
c_0 .. c_{n-1} are the word's list (WORD rows: nw < nd) or the document's (DOC rows: nw >= nd, ties among them).

  walk rows       ul = U * (tn + sum) - tn lands on cum[b]: the steering entry q (a topic the document does not use: it
                  moves typeNorm only) is bisected on its bit pattern for the flip of ul > cum[b], then the Phi entry of
                  candidate b (its count is 1 or 2) is scanned over 2 * SCAN + 1 neighbouring doubles.  b: first (0),
                  middle, last (n - 2) and, where n > 64, 62, 63, 64: the seam between the first block of 64 candidates and
                  the second.  Per scan value: "tie" (ul == cum[b]), "below" / "above" (ul within two ulps under / over
                  cum[b]) or "far".
  plateau rows    walk rows with zero scores, so that neighbouring running sums are equal.  A WORD row has them at every
                  candidate the document does not use (q itself is one: every WORD row has a plateau somewhere, a plateau
                  row has it right behind b); a DOC row at list topics whose Phi entry is 0.0 (further outside non-zeros
                  keep nw >= nd).  "mid": entries b + 1 (and b + 2) score 0.  "trail": the last one or two candidates
                  score 0 and b is the entry before the last scoring one, so a search that found no i with ul <= cum[i]
                  would fall to a topic of probability zero.  "lead": the first one or two candidates score 0, b is the
                  last of them, cum[b] == 0.0 and the edge ul against 0 is the branch's own edge; q is scanned.  Here
                  "tie" is ul == 0.0 (the draw IS candidate 0, of score zero: what the reference does); "below" is
                  ul < 0 (rare: U >= thr and U * (tn + sum) rounds under tn) or, under the edge proper, a scan value
                  on the alias side within two of one on the walk's side.
  branch rows     U against tn / (tn + sum): q bisected for the flip of the comparison, then scanned.
  ps / cell rows  the alias branch: q bisected for the flip of frac > ps[w][i] with i = (int)ups unchanged (aimed at
                  x = (i + ps[w][i]) / K), or for the change of i (aimed at x = j / K, tn = sum / (j / (U K) - 1)).  The DOC
                  rows of these two kinds have a column that is non-zero in every topic: nw = K, the candidates are the
                  document's list and the draw is spalias's draw formula for formula (asserted at every scan value).
                  In fact every DOC row is: where nw >= nd both schemes walk the document's list (spalias_expect).
  plain rows      the rows whose U does not suit, or whose aim found no flip.

Adjacent scan values on opposite sides of a comparison are "pairs": branch (U < thr), ps (frac > ps[w][i], same i), cell
(i changes).  Right under the branch's edge x can round to 1.0 and i to K: Java would throw, the restatement raises and
the device answers GGS_ERR_INVALID_TOPIC; such a scan value is lost for every row, so each row's scan is centred at a
scan index of its own (row.shift) and the categories count testable scan values only.

Behind the 2 * SCAN + 1 neighbouring doubles the scan goes on in steps of 2^7 .. 2^22 ulps to either side (FAR_OFFSETS):
next to the edge nearly every token is left to the replay, and these are the values at which the proposal starts to decide.

Scan value j of every row goes into Phi matrix j: one set_phi + set_z(z0) + set_iteration + sample_z_given_phi(1) per j.

proposal() restates the kernel's proposal (polyaurn_sparse_wave_kernel, "PROPOSAL"): the per-block running sums in a
chosen association, eps, thr, the alias test with dm, the walk test with delta and the look-back at sel - 1."""
import numpy as np

from oracle import oracle as O
from tests import polyaurn_sparse_restatement as R
from tests import spalias_restatement as SR

ALPHA = 0.1
BETA = 0.01
SEED = 4242
ITERATION = 1
MIN_PER_CATEGORY = 8
WORD, DOC = R.WORD, R.DOC
LIST_NAME = {WORD: "word", DOC: "doc"}
EDGE_CATS = ("tie", "below", "above")
PAIR_KINDS = ("branch", "ps", "cell")
ASSOCIATIONS = ("dpp", "chain", "reversed", "tree")
# beyond the neighbouring doubles: steps of 2^7 .. 2^22 ulps to either side, across the distance at which the proposal's
# margins (eps = (4 n + 64) 2^-53, a few hundred ulps of tn + sum) begin to decide
FAR_OFFSETS = [sign * 2 ** k for k in range(7, 23) for sign in (-1, 1)]


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(b):
    return float(np.int64(b).view(np.float64))


class Row:
    pass


class _NeedTable(Exception):
    pass


class _NoTable:
    """stands for a word's alias table until a draw reads it"""
    def __len__(self):
        raise _NeedTable

    def __getitem__(self, i):
        raise _NeedTable


_NO_TABLE = _NoTable()


class Spec:
    def __init__(self, name, K, scan, n_range, seam, per_walk, per_plateau, per_branch, per_alias, seed):
        self.name, self.K, self.scan, self.n_range, self.seam = name, K, scan, n_range, seam
        self.per_walk, self.per_plateau, self.per_branch, self.per_alias, self.seed = per_walk, per_plateau, per_branch, per_alias, seed


# narrow: spalias's figures (K = 8, lists of 3 to 5).  wide: every walk has more than 64 candidates.
NARROW = Spec("narrow", K=8, scan=100, n_range=(3, 5), seam=False, per_walk=14, per_plateau=14, per_branch=16, per_alias=16, seed=1)
WIDE = Spec("wide", K=160, scan=100, n_range=(70, 120), seam=True, per_walk=6, per_plateau=6, per_branch=6, per_alias=10, seed=2)


class KnifeEdge:
    def __init__(self, spec):
        self.spec, self.K, self.SCAN = spec, spec.K, spec.scan
        K = self.K
        rng = np.random.default_rng(spec.seed)
        positions = ["first", "middle", "last"] + (["b62", "b63", "b64"] if spec.seam else [])
        queue = []
        for lst in (WORD, DOC):
            queue += [(lst, "walk", p) for p in positions for _ in range(spec.per_walk)]
            queue += [(lst, "plateau", p) for p in ("mid", "lead", "trail") for _ in range(spec.per_plateau)]
            queue += [(lst, "branch", "-")] * spec.per_branch
            queue += [(lst, "ps", "-"), (lst, "cell", "-")] * spec.per_alias
        order = rng.permutation(len(queue))
        queue = [queue[i] for i in order]
        U_all = O.uniforms(SEED, ITERATION, R.PURPOSE_Z, 0, (len(queue) * 4 + 64) * (2 * spec.n_range[1] + 4))
        self.rows = []
        doc_ptr, tokens, z0 = [0], [], []
        while queue:
            lst, kind, pos = queue[0]
            row = self._layout(lst, kind, pos, rng)
            row.word = K + len(self.rows)
            lo, hi = (0.12, 0.8) if kind in ("ps", "cell") else (0.25, 0.9)
            start = len(tokens)
            for _ in range(12):
                st = SR.DocState(K, row.prefix + [row.old])
                for k in row.prefix:                                # every prefix token leaves and comes back
                    st.remove(k)
                    st.add(k)
                st.remove(row.old)
                row.U = float(U_all[start + len(row.prefix)])
                if lo <= row.U <= hi:
                    break
                # the uniform does not suit: one more token moves the target to the next one.  A topic that already has
                # two tokens and is not the scanned candidate: neither the list's order nor that candidate's count changes
                keep = (row.cand if lst == WORD else st.list)[row.b] if row.b is not None else -1
                twice = [t for t in st.list if st.cnt[t] >= 2 and t != keep]
                if not twice:
                    break
                row.prefix.append(twice[0])
            row.st = st
            tokens += row.prefix + [row.word]
            z0 += row.prefix + [row.old]
            doc_ptr.append(len(tokens))
            row.target = len(tokens) - 1
            row.shift = int(rng.integers(-self.SCAN // 2, self.SCAN // 2 + 1))
            if lo <= row.U <= hi and self._solve(row, rng):
                queue.pop(0)
            else:
                self._plain(row, rng)
            self.rows.append(row)
            assert len(self.rows) < 4 * len(order) + 64, "too few suitable uniforms"
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int32)
        self.z0 = np.asarray(z0, np.int32)
        self.V = K + len(self.rows)
        self.NEAR = 2 * self.SCAN + 1                               # scan values 0 .. NEAR - 1 are neighbouring doubles,
        self.J = self.NEAR + len(FAR_OFFSETS)                       # the rest step away from the edge: where the proposal decides
        self._survey, self._spalias, self._steps = None, None, {}

    # ---- one row's document ----------------------------------------------------------------------------------------
    def _layout(self, lst, kind, pos, rng):
        """The document and the roles of the candidates: row.n candidates, row.zero the positions that score 0.0, row.b
        the boundary, row.q the steering topic; the candidates themselves follow in _roles, after the simulation."""
        K, spec = self.K, self.spec
        row = Row()
        row.lst, row.kind, row.pos = lst, kind, pos
        r = int(rng.integers(1, 3)) if kind == "plateau" else 0     # the zero run of a plateau row
        lo, hi = spec.n_range
        if lst == WORD and spec.seam:                               # word lists of 67 to nd - 1 entries (65 would do where b is no seam)
            nd = int(rng.integers(lo, hi + 1))
            n = int(rng.integers(67 if pos != "first" else 65, nd))
        elif lst == WORD:                                           # nw < nd, and nd + the outside candidates <= K
            n = int(rng.integers(max(lo, r + 2), hi + 1))
            nd = int(rng.integers(n + 1, K - max(r, 1) + 1))
        else:
            nd = int(rng.integers(max(lo, r + 2), hi + 1))
            n = nd
        row.n, row.nd, row.r = n, nd, r
        row.shared = lst == DOC and kind in ("ps", "cell")
        if kind == "plateau":
            if pos == "mid":
                row.b = int(rng.integers(61, 64)) if spec.seam else int(rng.integers(0, n - r - 1))
                zero = list(range(row.b + 1, row.b + 1 + r))
            elif pos == "lead":
                row.b = r - 1
                zero = list(range(r))
            else:
                row.b = n - r - 2
                zero = list(range(n - r, n))
        else:
            row.b = {"first": 0, "middle": (n - 1) // 2, "last": n - 2, "b62": 62, "b63": 63, "b64": 64, "-": None}[pos]
            zero = []
        if lst == WORD and not zero:                                # q is a candidate of score 0: away from b + 1
            allowed = [p for p in range(n) if row.b is None or p not in (row.b, row.b + 1)]
            zero = [int(rng.choice(allowed))]
        row.zero = sorted(zero)
        ids = [int(t) for t in rng.permutation(K)]
        if lst == WORD:
            cand = sorted(ids[:n])
            row.cand = cand
            outside_c = [cand[p] for p in row.zero]
            in_doc = [c for c in cand if c not in outside_c] + ids[n:n + nd - (n - len(outside_c))]
            row.q = outside_c[-1] if kind != "plateau" or pos != "lead" else outside_c[0]
            row.outside = [t for t in outside_c if t != row.q]
        else:
            in_doc = ids[:nd]
            rest = ids[nd:]
            row.q, rest = rest[0], rest[1:]
            more = len(row.zero) - 1 + int(rng.integers(0, 2)) if row.zero else int(rng.integers(0, 3))
            more = max(0, min(more, len(rest)))                     # len(zero) - 1: a tie, nw == nd
            if kind in ("ps", "cell"):
                more = len(rest)                                    # non-zero in every topic: spalias's draw
            row.outside = rest[:more]
        assert len(in_doc) == nd and len(set(in_doc)) == nd
        in_doc = [int(t) for t in rng.permutation(in_doc)]
        p2 = 0.5 if not spec.seam else 0.08
        counts = [2 if rng.random() < p2 else 1 for _ in in_doc]
        row.prefix = in_doc + [t for t, c in zip(in_doc, counts) for _ in range(c - 1)]
        row.old = in_doc[0]
        return row

    def _roles(self, row):
        st = row.st
        assert len(st.list) == row.nd
        if row.lst == DOC:
            row.cand = list(st.list)
        row.cntv = np.array([st.cnt[k] for k in row.cand], np.float64)
        if row.lst == WORD:                                         # the candidates the document does not use, and only they, score 0
            assert all((row.cntv[p] == 0) == (p in row.zero) for p in range(row.n))
        row.scoring = [p for p in range(row.n) if p not in row.zero]

    def _base_column(self, row, rng):
        col = np.zeros(self.K)
        for p in row.scoring:
            col[row.cand[p]] = rng.uniform(0.1, 1.0)
        if row.lst == WORD:
            col[row.outside] = rng.uniform(0.1, 1.0, len(row.outside))
        else:
            col[row.outside] = rng.uniform(0.001, 0.05, len(row.outside))
        return col

    def _plain(self, row, rng):
        row.kind, row.pos, row.b = "plain", "-", None
        self._roles(row)
        col = self._base_column(row, rng)
        col[row.q] = 0.3
        row.scan_topic, row.centre, row.col = row.q, _bits(0.3), col
        row.fixed_scan = True

    # ---- evaluation ------------------------------------------------------------------------------------------------
    def _eval(self, row, col):
        """(the restatement's draw or None where it raises, its detail).  The word's alias table is built only where the
        draw reads it (the alias branch): detail["tables"] = (ps, a), else None; detail["tn"] = typeNorm either way."""
        tn = float(np.cumsum(col * ALPHA)[-1])                      # alias_table's own typeNorm
        nzw = np.flatnonzero(col != 0.0)
        det = {"tn": tn, "tables": None}
        try:
            new = R.token_draw(row.st, col, nzw, _NO_TABLE, _NO_TABLE, tn, row.U, self.K, det)
        except _NeedTable:
            ps, a, tn2 = SR.alias_table(col * ALPHA)
            assert tn2 == tn
            det = {"tn": tn, "tables": (ps, a)}
            try:
                new = R.token_draw(row.st, col, nzw, ps, a, tn, row.U, self.K, det)
            except R.InvalidTopic:
                new, det["invalid"] = None, True
            if row.shared:                                          # spalias's draw, formula for formula
                sdet = {}
                try:
                    snew = SR.token_draw(row.st, row.old, col, ps, a, tn, row.U, sdet)
                except SR.InvalidTopic:
                    snew = None
                assert snew == new and sdet["prior"] and sdet["sum"] == det["sum"], "the shared alias rows are not spalias's draw"
        return new, det

    def _flip(self, row, col, topic, key, lo, hi):
        """lo such that key differs between the adjacent doubles lo, lo + 1 of col[topic], or None"""
        def k(bits):
            c = col.copy()
            c[topic] = _dbl(bits)
            return key(self._eval(row, c)[1])
        klo = k(lo)
        if klo == k(hi):
            return None
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if k(mid) == klo:
                lo = mid
            else:
                hi = mid
        return lo

    def _solve(self, row, rng):
        self._roles(row)
        K, U, q = self.K, row.U, row.q
        col = self._base_column(row, rng)
        cand = np.asarray(row.cand, np.int64)

        def sums():
            return np.cumsum(row.cntv * col[cand])

        def q_for_tn(tn_target):
            c = col.copy()
            c[q] = 0.0
            return (tn_target - float(np.sum(c * ALPHA))) / ALPHA

        b = row.b
        if row.kind in ("walk", "plateau") and row.pos != "lead":
            cum = sums()
            if cum[b] / cum[-1] > U / 2:                            # room above the boundary: the entries behind b grow
                need = cum[b] * (2.0 / U - 1.0)
                behind = [row.cand[p] for p in row.scoring if p > b]
                col[behind] *= need / (cum[-1] - cum[b])
            cum = sums()
            x0 = q_for_tn((U * cum[-1] - cum[b]) / (1.0 - U))
            key = lambda det: (not det["prior"]) and det["ul"] > float(det["cum"][b])
            width = 2.0
        elif row.kind == "branch" or row.pos == "lead":
            x0 = q_for_tn(U * float(sums()[-1]) / (1.0 - U))
            key = (lambda det: not det["prior"]) if row.kind == "branch" else (lambda det: (not det["prior"]) and det["ul"] > 0.0)
            width = 2.0
        else:
            s = float(sums()[-1])
            lo_cell = int(np.floor(U * K)) + 1                      # x > U: cells above U * K
            if row.kind == "cell":
                if lo_cell > K - 1:
                    return False
                j = int(rng.integers(lo_cell, K))
                x0 = q_for_tn(s / (j / (U * K) - 1.0))
                key = lambda det: det["i"] if det["prior"] else -1
                width = 1.0 + 0.3 / j
            else:
                x0 = None
                for attempt in range(4):                            # ps[w][i] moves with q: a few rounds of aiming
                    c = col.copy()
                    c[q] = x0 if x0 is not None else float(np.mean(col[col > 0]))
                    ps, _, _ = SR.alias_table(c * ALPHA)
                    if attempt == 0:
                        cells = [i for i in range(lo_cell, K) if 0.05 < ps[i] < 0.95]
                        if not cells:
                            return False
                        i = int(rng.choice(cells))
                    x0 = q_for_tn(s / ((i + ps[i]) / (U * K) - 1.0))
                    if not x0 > 0:
                        return False
                key = lambda det: (det["i"], det["frac"] > det["ps_i"]) if det["prior"] and det["i"] < K else -1
                width = 1.0 + 0.2 / (i + 1)
        if not x0 > 0:
            return False
        col[q] = x0
        col /= 1.2 * col.max()                                      # the draw is scale-free in the column
        lo = self._flip(row, col, q, key, _bits(col[q] / width), _bits(col[q] * width))
        if lo is None:
            return False
        if row.kind == "ps":                                        # the flip that was aimed at, not a change of cell
            ka = self._eval(row, self._with(col, q, _dbl(lo)))[1]
            kb = self._eval(row, self._with(col, q, _dbl(lo + 1)))[1]
            if not (ka["prior"] and kb["prior"] and ka["i"] == kb["i"]):
                return False
        col[q] = _dbl(lo + 1)
        if row.kind in ("walk", "plateau") and row.pos != "lead":
            row.scan_topic = row.cand[b]
            row.centre = _bits(col[row.scan_topic])
        else:
            row.scan_topic, row.centre = q, lo
        row.col = col
        row.fixed_scan = False
        return True

    @staticmethod
    def _with(col, topic, value):
        c = col.copy()
        c[topic] = value
        return c

    def column(self, row, j):
        """the target word's Phi column at scan value j in [0, J)"""
        if row.fixed_scan:
            return row.col
        if j >= self.NEAR:
            return self._with(row.col, row.scan_topic, _dbl(row.centre + FAR_OFFSETS[j - self.NEAR]))
        return self._with(row.col, row.scan_topic, _dbl(row.centre + (j - self.SCAN - row.shift)))

    # ---- the scan --------------------------------------------------------------------------------------------------
    def phi(self, j):
        """Phi [K][V] of scan value j."""
        K = self.K
        phi = np.zeros((K, self.V))
        phi[np.arange(K), np.arange(K)] = 1.0
        for row in self.rows:
            phi[:, row.word] = self.column(row, j)
        return phi

    def classify(self, row, j):
        """(category, the topic the builder expects or None, new, det) of row at scan value j.  The expected topic of a
        walk is the candidate at the smallest i with ul <= cum[i], the last one if there is none; of an alias draw the
        restatement's."""
        new, det = self._eval(row, self.column(row, j))
        assert det["kind"] == row.lst and det["cand"] == row.cand, "the row does not walk the list it was built for"
        if det.get("invalid"):
            return "invalid", None, new, det
        if det["prior"]:
            want = new
        else:
            ul, cum = det["ul"], det["cum"]
            first = [i for i in range(row.n) if ul <= float(cum[i])]
            want = row.cand[first[0] if first else row.n - 1]
        if row.kind == "plain":
            return "plain", want, new, det
        if row.kind in ("branch", "ps", "cell"):
            return ("prior" if det["prior"] else "likelihood"), want, new, det
        if det["prior"]:
            return "far", want, new, det
        b = row.b
        ul, cb = det["ul"], float(det["cum"][b])
        if row.pos == "lead":                                       # cum[b] == 0.0; ul moves in steps of typeNorm's spacing
            unit = float(np.spacing(det["tn"]))
            if ul == 0.0:
                return "tie", want, new, det
            if abs(ul) <= 2 * unit:
                return ("below" if ul < 0 else "above"), want, new, det
            return "far", want, new, det
        scoring_before = [p for p in row.scoring if p < b]
        if scoring_before and ul <= float(det["cum"][scoring_before[-1]]):
            return "far", want, new, det
        scoring_after = [p for p in row.scoring if p > b]
        if len(scoring_after) > 1 and ul > float(det["cum"][scoring_after[0]]):
            return "far", want, new, det
        if ul == cb:
            return "tie", want, new, det
        d = _bits(cb) - _bits(ul) if ul > 0 else 10 ** 9            # in ulps of ul (same binade near the edge; else "far")
        if abs(d) <= 2 and np.frexp(ul)[1] == np.frexp(cb)[1]:
            return ("below" if d > 0 else "above"), want, new, det
        return "far", want, new, det

    def survey(self):
        """dict(evals=[row][j] -> (category, want, new, det), invalid=the scan values at which some row raises,
        counts[(list, kind, position, category)] over the testable scan values, pairs[(list, pair kind)],
        ps_ties=exact ties frac == ps[w][i], expect=[(j, target token, topic, row index, category)])."""
        if self._survey is not None:
            return self._survey
        evals = [[self.classify(row, j) for j in range(self.J)] for row in self.rows]
        invalid = sorted({j for ev in evals for j in range(self.J) if ev[j][0] == "invalid"})
        for row, ev in zip(self.rows, evals):                       # lead rows: under the edge the reference takes the alias branch
            if row.pos == "lead":
                walk = [j for j in range(self.NEAR) if ev[j][0] != "invalid" and not ev[j][3]["prior"]]
                for j in range(self.NEAR):
                    if ev[j][0] == "far" and ev[j][3]["prior"] and any(abs(j - k) <= 2 for k in walk):
                        ev[j] = ("below",) + ev[j][1:]
        bad = set(invalid)
        counts, pairs, expect, ps_ties = {}, {}, [], 0
        for r, (row, ev) in enumerate(zip(self.rows, evals)):
            lname = LIST_NAME[row.lst]
            for j in range(self.J):
                cat, want, new, det = ev[j]
                if j in bad:
                    continue
                key = (lname, row.kind, row.pos, cat)
                counts[key] = counts.get(key, 0) + 1
                expect.append((j, row.target, int(want), r, cat))
                if det["prior"] and det["i"] < self.K and det["frac"] == det["ps_i"]:
                    ps_ties += 1
                if j == 0 or j >= self.NEAR or (j - 1) in bad:
                    continue
                pdet = ev[j - 1][3]
                kinds = []
                if pdet["prior"] != det["prior"]:
                    kinds.append("branch")
                elif det["prior"]:
                    if pdet["i"] != det["i"]:
                        kinds.append("cell")
                    elif (pdet["frac"] > pdet["ps_i"]) != (det["frac"] > det["ps_i"]):
                        kinds.append("ps")
                for k in kinds:
                    pairs[(lname, k)] = pairs.get((lname, k), 0) + 1
                    ev[j][3].setdefault("pair", k)
                    pdet.setdefault("pair", k)
        self._survey = dict(evals=evals, invalid=invalid, counts=counts, pairs=pairs, ps_ties=ps_ties, expect=expect)
        return self._survey

    def spalias_expect(self):
        """[J][rows]: the topic spalias's restatement draws for every target (scheme=spalias walks the document's list in
        every row: the DOC rows keep their edges, the WORD rows are plain tokens there), -1 where it raises."""
        if self._spalias is None:
            sv = self.survey()
            out = np.full((self.J, len(self.rows)), -1, np.int64)
            for r, row in enumerate(self.rows):
                for j in range(self.J):
                    det = sv["evals"][r][j][3]
                    col = self.column(row, j)
                    ps, a = det["tables"] if det["tables"] is not None else SR.alias_table(col * ALPHA)[:2] if row.lst == WORD else (None, None)
                    try:                                            # a DOC row off the alias branch: spalias does not read the table either
                        out[j, r] = SR.token_draw(row.st, row.old, col, ps, a, det["tn"], row.U)
                    except SR.InvalidTopic:
                        pass
                    if row.lst == DOC:
                        assert out[j, r] == (-1 if sv["evals"][r][j][2] is None else sv["evals"][r][j][2])
            self._spalias = out
        return self._spalias

    def spalias_z(self, j):
        """z after scheme=spalias's step with Phi matrix j, or None where its restatement raises"""
        z = self.z0.astype(np.int64)
        phi = self.phi(j)
        try:
            SR.z_step(self.doc_ptr, self.tokens, z, phi, SR.alias_tables(phi, ALPHA), SEED, ITERATION)
        except SR.InvalidTopic:
            return None
        return z

    def restatement_z(self, j):
        """z after the step with Phi matrix j and the restatement's counters of that step, or (None, None) where the
        restatement raises what Java would throw."""
        if j not in self._steps:
            self._steps[j] = self._restatement_z(j)
        return self._steps[j]

    def _restatement_z(self, j):
        z = self.z0.astype(np.int64)
        phi = self.phi(j)
        stats = np.zeros(4, np.int64)
        try:
            R.z_step(self.doc_ptr, self.tokens, z, phi, SR.alias_tables(phi, ALPHA), R.word_lists(phi)[1], SEED, ITERATION, stats=stats)
        except R.InvalidTopic:
            return None, None
        return z, stats


_built = {}


def fixture(name):
    """the narrow or the wide fixture, built once per process and left unchanged"""
    if name not in _built:
        _built[name] = KnifeEdge({"narrow": NARROW, "wide": WIDE}[name])
    return _built[name]


def required_categories():
    """every (list, kind, position) whose tie / below / above count must reach MIN_PER_CATEGORY across the two fixtures"""
    out = []
    for lname in LIST_NAME.values():
        out += [(lname, "walk", p) for p in ("first", "middle", "last", "b62", "b63", "b64")]
        out += [(lname, "plateau", p) for p in ("mid", "lead", "trail")]
    return out


# ---- the kernel's proposal ------------------------------------------------------------------------------------------
def _scan_dpp(x):
    """wave_inclusive_scan (csrc/ggs_exact_sum.hpp) on [J][64]: shifts by 1, 2, 4, 8 inside rows of 16 lanes, lane 15 of
    row 0 into row 1 and of row 2 into row 3, lane 31 into rows 2 and 3"""
    x = x.copy()
    lane = np.arange(64) % 16
    for s in (1, 2, 4, 8):
        src = np.zeros_like(x)
        src[:, s:] = x[:, :-s]
        src[:, lane < s] = 0.0
        x = x + src
    x[:, 16:32] = x[:, 16:32] + x[:, 15:16]
    x[:, 48:64] = x[:, 48:64] + x[:, 47:48]
    x[:, 32:64] = x[:, 32:64] + x[:, 31:32]
    return x


def _scan_reversed(x):
    out = np.empty_like(x)
    for i in range(x.shape[1]):
        acc = x[:, i].copy()
        for k in range(i - 1, -1, -1):
            acc = acc + x[:, k]
        out[:, i] = acc
    return out


def _scan_tree(x):
    out = np.empty_like(x)
    for i in range(x.shape[1]):
        m = 1
        while m < i + 1:
            m *= 2
        v = np.zeros((x.shape[0], m))
        v[:, :i + 1] = x[:, :i + 1]
        while v.shape[1] > 1:
            v = v[:, 0::2] + v[:, 1::2]
        out[:, i] = v[:, 0]
    return out


_SCANS = {"dpp": _scan_dpp, "chain": lambda x: np.cumsum(x, axis=1), "reversed": _scan_reversed, "tree": _scan_tree}


def block_sums(scores, assoc="dpp"):
    """the proposal's running sums of scores [J][n]: per block of 64 candidates before + scan(score), before = lane 63"""
    scores = np.atleast_2d(np.asarray(scores, np.float64))
    J, n = scores.shape
    out = np.empty((J, n))
    before = np.zeros((J, 1))
    for base in range(0, n, 64):
        blk = np.zeros((J, 64))
        m = min(64, n - base)
        blk[:, :m] = scores[:, base:base + m]
        sc = before + _SCANS[assoc](blk)
        out[:, base:base + m] = sc[:, :m]
        before = sc[:, 63:64]
    return out, before[:, 0]


def proposal(scores, tn, U, K, ps_w, a_w, cand, eps_scale=1.0, assoc="dpp", sums=None):
    """The topic the kernel's proposal decides for one token, or None where it leaves the token to the replay.
    sums = (running sums [n], their last value) computed ahead with block_sums, else computed here."""
    n = len(cand)
    if sums is None:
        c, s = block_sums(scores, assoc)
        cuml, s_hat = c[0], float(s[0])
    else:
        cuml, s_hat = sums
    tn, U = float(tn), float(U)
    eps = float(4 * n + 64) * 2.0 ** -53 * eps_scale
    den = tn + s_hat
    with np.errstate(invalid="ignore", divide="ignore"):
        thr = float(np.float64(tn) / np.float64(den))
    if U < thr * (1.0 - eps):
        x = U + (s_hat * U) / tn
        ups = x * float(K)
        i = int(ups)
        frac, dm = ups - float(i), float(K) * eps * (x + 1.0)
        if i < K and frac > dm and frac < 1.0 - dm:
            psv = float(ps_w[i])
            if abs(frac - psv) > dm:
                return int(a_w[i]) if frac > psv else i
        return None
    if U > thr * (1.0 + eps):
        ul, delta = U * den - tn, eps * den
        for base in range(0, n, 64):
            m = [e for e in range(base, min(base + 64, n)) if ul - float(cuml[e]) < -delta]
            if m:
                sel = m[0]
                if sel == 0 or ul - float(cuml[sel - 1]) > delta:
                    return int(cand[sel])
                return None
    return None
