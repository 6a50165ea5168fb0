"""Knife-edge rows for the sparse z step of scheme=spalias (a test helper, not collected; the manner of
tests/test_knife_edge_model.py, a builder of its own).

A row is a document of its own: a prefix of tokens whose words have one-hot Phi columns (word k: phi[k] = 1, so such a
token keeps its topic k whatever it draws with) and one TARGET token, last, with a word of its own.  The prefix fixes the
document's list and counts at the target; the target's uniform U is known from the oracle's stream (purpose Z, element =
the token's index); the target word's Phi column is then solved so that the draw sits on an edge:

  boundary rows   ul = U * (tn + sum) - tn lands on cum[b]: a coarse solve of the Phi entry of a topic OUTSIDE the list
                  (it moves typeNorm only; bisection on its bit pattern for the sign change of ul - cum[b]), then a scan of
                  the Phi entry of list entry b itself, 2 * SCAN + 1 neighbouring doubles (its count is 1 or 2, so cum[b]
                  steps through every double near ul).  Per scan value: "tie" (ul == cum[b]), "below" / "above" (ul one
                  or two ulps of ul under / over cum[b]) or "far".  b is the first entry (0), a middle one, or the last
                  boundary there is, nnz - 2: ul <= U * sum < cum[nnz - 1] whenever tn > 0, so cum[last] itself cannot be
                  reached and the last entry is drawn exactly when ul is above cum[nnz - 2].
  branch rows     U against tn / (tn + sum): the outside entry bisected for the flip of the comparison, then scanned; two
                  adjacent scan values with the comparison true for one and false for the other make a "branch" pair.

Scan value j of every row goes into Phi matrix j: one ggs_set_phi + one z step per scan value, from the same z and the same
iteration, so every row keeps its U."""
import numpy as np

from oracle import oracle as O
from tests import spalias_restatement as R

K = 8
ALPHA = 0.1
BETA = 0.01
SEED = 4242
ITERATION = 1
SCAN = 100
POSITIONS = ("first", "middle", "last")
MIN_PER_CATEGORY = 8


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(b):
    return float(np.int64(b).view(np.float64))


def _ulps_apart(a, b):
    return _bits(a) - _bits(b)                                      # both positive


class Row:
    pass


class KnifeEdge:
    def __init__(self, rows_per_position=20, branch_rows=30, seed=1):
        rng = np.random.default_rng(seed)
        n_rows = 3 * rows_per_position + branch_rows
        n_docs = 2 * n_rows                                         # about two thirds have a uniform that suits; the rest are plain rows
        self.rows = []
        doc_ptr, tokens, z0 = [0], [], []
        for r in range(n_docs):
            m = int(rng.integers(3, 6))                             # list entries at the target
            topics = rng.permutation(K)[:m]
            counts = rng.integers(1, 3, m)
            prefix = [int(t) for t in topics] + [int(t) for t, c in zip(topics, counts) for _ in range(c - 1)]
            row = Row()
            row.word = K + r
            row.old = int(topics[0])                                # the target's old topic: in the list with the prefix's count left
            tokens += prefix + [row.word]
            z0 += prefix + [row.old]
            doc_ptr.append(len(tokens))
            row.target = len(tokens) - 1
            st = R.DocState(K, z0[doc_ptr[-2]:doc_ptr[-1]])
            for k in prefix:                                        # every prefix token leaves and comes back
                st.remove(k)
                st.add(k)
            st.remove(row.old)
            row.st = st
            self.rows.append(row)
        self.doc_ptr = np.asarray(doc_ptr, np.int64)
        self.tokens = np.asarray(tokens, np.int32)
        self.z0 = np.asarray(z0, np.int32)
        self.V = K + n_docs
        U = O.uniforms(SEED, ITERATION, R.PURPOSE_Z, 0, len(tokens))
        kinds = [POSITIONS[i % 3] for i in range(3 * rows_per_position)] + ["branch"] * branch_rows
        for row in self.rows:
            row.U = float(U[row.target])
            row.kind = kinds.pop(0) if kinds and 0.25 <= row.U <= 0.9 else "plain"
            self._solve(row, rng)
        assert not kinds, "too few suitable uniforms"

    # ---- one row -------------------------------------------------------------------------------------------------
    def _eval(self, row, col):
        ps, a, tn = R.alias_table(col * ALPHA)
        det = {}
        try:
            new = R.token_draw(row.st, row.old, col, ps, a, tn, row.U, det)
        except R.InvalidTopic:                                      # right under the branch's edge x can round to 1.0: Java would throw
            new, det["invalid"] = None, True
        return new, det

    def _solve(self, row, rng):
        st, U = row.st, row.U
        nnz = len(st.list)
        col = np.zeros(K)
        col[st.list] = rng.uniform(0.1, 1.0, nnz)
        outside = [k for k in range(K) if k not in st.pos]
        q = outside[0]
        if rng.random() < 0.5:
            col[outside[1:]] = rng.uniform(0.001, 0.05, len(outside) - 1)   # else: zeros in the column
        row.q, row.b, row.scan_topic = q, None, q
        if row.kind == "plain":
            col[q] = 0.3
            row.cols = [col.copy() for _ in range(2 * SCAN + 1)]
            return
        n = np.array([st.cnt[k] for k in st.list], np.float64)
        if row.kind != "branch":
            b = {"first": 0, "middle": (nnz - 1) // 2, "last": nnz - 2}[row.kind]
            row.b = b
            cum = np.cumsum(n * col[st.list])
            if cum[b] / cum[-1] > U / 2:                            # room above the boundary: the entries behind b grow
                need = cum[b] * (2.0 / U - 1.0)
                col[st.list[b + 1:]] *= need / (cum[-1] - cum[b])
            cum = np.cumsum(n * col[st.list])
            tn_target = (U * cum[-1] - cum[b]) / (1.0 - U)
        else:
            s = float(np.sum(n * col[st.list]))
            tn_target = U * s / (1.0 - U)
        fixed = float(np.sum(col * ALPHA))
        x0 = (tn_target - fixed) / ALPHA
        assert x0 > 0
        col[q] = x0
        col /= 1.2 * col.max()                                      # the draw is scale-free in the column
        # bisection on the outside entry's bits: `over` is true for small x, false for large x
        def over(x):
            c = col.copy()
            c[q] = x
            _, det = self._eval(row, c)
            return (not det["prior"]) if row.kind == "branch" else (not det["prior"] and det["ul"] > det["cum"][row.b])
        lo, hi = _bits(col[q] * 0.5), _bits(col[q] * 2.0)
        assert over(_dbl(lo)) and not over(_dbl(hi)), "no sign change to bisect"
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if over(_dbl(mid)):
                lo = mid
            else:
                hi = mid
        col[q] = _dbl(hi)
        if row.kind == "branch":
            row.scan_topic, centre = q, lo                          # lo and hi = lo + 1 straddle the flip
        else:
            row.scan_topic = st.list[row.b]
            centre = _bits(col[row.scan_topic])
        row.cols = []
        for j in range(-SCAN, SCAN + 1):
            c = col.copy()
            c[row.scan_topic] = _dbl(centre + j)
            row.cols.append(c)

    # ---- the scan ------------------------------------------------------------------------------------------------
    def phi(self, j):
        """Phi [K][V] of scan value j in [0, 2 * SCAN]."""
        phi = np.zeros((K, self.V))
        phi[np.arange(K), np.arange(K)] = 1.0
        for row in self.rows:
            phi[:, row.word] = row.cols[j]
        return phi

    def classify(self, row, j):
        """(category, the topic the builder expects or None) of row at scan value j."""
        new, det = self._eval(row, row.cols[j])
        if row.kind == "plain":
            return "plain", None, det
        if row.kind == "branch":
            return ("invalid" if det.get("invalid") else "prior" if det["prior"] else "likelihood"), None, det
        if det["prior"]:
            return "far", None, det
        ul, cb = det["ul"], float(det["cum"][row.b])
        want = row.st.list[row.b] if ul <= cb else row.st.list[row.b + 1]
        if row.b > 0 and ul <= float(det["cum"][row.b - 1]):
            return "far", None, det
        if row.b + 1 < len(row.st.list) - 1 and ul > float(det["cum"][row.b + 1]):
            return "far", None, det
        if ul == cb:
            return "tie", want, det
        d = _ulps_apart(cb, ul)                                     # in ulps of ul (same binade near the edge; else "far")
        if abs(d) <= 2 and np.frexp(ul)[1] == np.frexp(cb)[1]:
            return ("below" if d > 0 else "above"), want, det
        return "far", want, det

    def survey(self):
        """counts[(kind, category)], the expectations [(j, target token, topic)] and the branch pairs found."""
        counts, expect, pairs = {}, [], 0
        for row in self.rows:
            prev = None
            for j in range(2 * SCAN + 1):
                cat, want, _ = self.classify(row, j)
                counts[(row.kind, cat)] = counts.get((row.kind, cat), 0) + 1
                if want is not None:
                    expect.append((j, row.target, int(want), row.kind, cat))
                if row.kind == "branch":
                    side = cat == "likelihood"
                    if prev is not None and prev != side:
                        pairs += 1
                    prev = side
        return counts, expect, pairs

    def restatement_z(self, j):
        """z after the step with Phi matrix j, or None where the restatement raises what Java would throw."""
        z = self.z0.astype(np.int64)
        phi = self.phi(j)
        try:
            R.z_step(self.doc_ptr, self.tokens, z, phi, R.alias_tables(phi, ALPHA), SEED, ITERATION)
        except R.InvalidTopic:
            return None
        return z
