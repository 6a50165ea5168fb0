"""The two distance loops of the diagnostics (compute_doc_topic_distances; UPLDA:723-753 "Quantity A", :778-806 "Quantity B"),
restated in numpy for tests/test_min_distances_model.py (CPU) and tests/test_min_distances_gpu.py (the kernels of
csrc/ggs_distances.hpp, bit for bit).

Per pair the reference does  s = 0.0;  for k in index order: s += Math.pow(a[k] - b[k], 2.0);  dist = Math.sqrt(s);  and the
minimum starts at 1e+20 and is replaced only when dist < min.  Here: S = S + T * T with T = A[:, None, k] - B[None, :, k],
element-wise -- every pair keeps its own index order, and numpy rounds the product and the sum separately (two roundings,
no FMA).  Math.pow(x, 2.0) is x * x on HotSpot from JDK 9 on (an assumption for older JVMs and StrictMath).  sqrt is
correctly rounded, hence monotone, so the minimum of the distances is the square root of the minimum of the sums.
"""
import numpy as np

NO_PARTNER = 1e+20          # the reference's initial minimum


def pair_sums(a, b=None, reverse=False):
    """S [n][m]: the in-order sums of squared differences of the rows of a [n][L] against the rows of b [m][L] (None: a)."""
    a = np.ascontiguousarray(a, np.float64)
    b = a if b is None else np.ascontiguousarray(b, np.float64)
    s = np.zeros((a.shape[0], b.shape[0]), np.float64)
    ks = range(a.shape[1] - 1, -1, -1) if reverse else range(a.shape[1])
    with np.errstate(all="ignore"):
        for k in ks:
            t = a[:, None, k] - b[None, :, k]
            s = s + t * t
    return s


def minima(s, skip_diagonal):
    """(min_dist [n], min_sq [n]) of the sums s [n][m]: a NaN sum never replaces a minimum (NaN < x is false), a row without a
    partner keeps 1e+20 (min_sq: +inf), and dist < 1e+20 is the reference's replacement test against its initial value."""
    m = np.where(np.isnan(s), np.inf, s)
    if skip_diagonal:
        m = m.copy()
        np.fill_diagonal(m, np.inf)
    min_sq = m.min(axis=1) if m.shape[1] else np.full(m.shape[0], np.inf)
    with np.errstate(all="ignore"):
        d = np.sqrt(min_sq)
    return np.where(d < NO_PARTNER, d, NO_PARTNER), min_sq


def min_distances(a, b=None):
    """(min_dist, min_sq) per row of a: against the other rows of a (b None, the reference's document loop), or against the
    rows of a foreign block b (no diagonal)."""
    return minima(pair_sums(a, b), skip_diagonal=b is None)


def min_topic_distance(phi):
    """The reference's topic loop over phi [K][V]: min over i > j."""
    return float(min_distances(phi)[0].min()) if len(phi) else NO_PARTNER


def scalar_min_distances(a, b=None):
    """The reference's loops, statement for statement, on Python floats (doubles): the twin that checks the numpy form."""
    a = np.asarray(a, np.float64)
    other = a if b is None else np.asarray(b, np.float64)
    out, out_sq = [], []
    for d in range(a.shape[0]):
        best, best_sq = NO_PARTNER, float("inf")
        for dd in range(other.shape[0]):
            if b is None and d == dd:
                continue
            s = 0.0
            for k in range(a.shape[1]):
                t = float(a[d, k]) - float(other[dd, k])
                s = s + t * t
            dist = float(np.sqrt(np.float64(s)))
            if dist < best:
                best = dist
            if s < best_sq:
                best_sq = s
        out.append(best)
        out_sq.append(best_sq)
    return np.array(out, np.float64), np.array(out_sq, np.float64)


def fma_pair_sums(a):
    """pair_sums(a) as a fused multiply-add would accumulate it: s = round(s + t * t) with ONE rounding, through exact
    rationals.  What the kernels must not compute."""
    from fractions import Fraction
    a = np.asarray(a, np.float64)
    n, length = a.shape
    s = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(n):
            acc = 0.0
            for k in range(length):
                t = float(a[i, k]) - float(a[j, k])
                acc = float(Fraction(acc) + Fraction(t) * Fraction(t))     # float(Fraction) rounds to nearest even
            s[i, j] = acc
    return s


# ---- the inputs of the GPU cases, shared with the CPU power check -----------------------------------------------------
def dirichlet_rows(n, length, seed, conc=0.3):
    """n rows of Dirichlet(conc, ..., conc) of the given length: theta- and Phi-like rows (sparse-ish, summing to 1)."""
    return np.random.default_rng([n, length, seed]).dirichlet(np.full(length, conc), n)


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)
