"""The distance classes of cc/mallet/similarity, the n nearest of tui/LDASimilarity.java:175-183, the length rule of
LDADistancer.java:84-87 and the centroids and query row of classify/KLDivergenceClassifier.java restated in Python, for
tests/test_similarity_model.py (CPU) and tests/test_similarity_gpu.py (the kernels of csrc/ggs_similarity.hpp, bit for bit).

One function per class, a plain scalar loop written from the Java: Python floats are IEEE doubles and every operation below is
rounded on its own, as the JVM rounds it.  Math.pow(x, 2) is x * x; Math.sqrt is math.sqrt (correctly rounded); Math.log is the
oracle's fdlibm log.  calculate(v1, v2) is called with v1 = the training row and v2 = the query row.

cc.mallet.util.Maths.klDivergence is MALLET's and not in the reference tree; `kl` is what this project assumes it to be.

`pairwise(name, A, B)` is the same arithmetic for all pairs at once: the index loop stays a Python loop, so every pair's sums take
their addends in index order, and numpy rounds each element-wise operation on its own.  The model test holds it to the scalar
functions bit for bit; the GPU tests use it where the scalar loops would take minutes."""
import math

import numpy as np

INF = float("inf")
LN2 = float.fromhex("0x1.62e42fefa39efp-1")           # Math.log(2) = 0x3FE62E42FEFA39EF

NAMES = ("ManhattanDistance", "EuclidianDistance", "HellingerDistance", "CosineDistance", "CanberraDistance", "ChebychevDistance",
         "JaccardDistance", "KLDistance", "JensenShannonDistance", "UberDistance", "StatisticalDistance", "BhattacharyyaDistance")


def _log_array(x):
    from oracle import oracle as O
    O.build()
    x = np.ascontiguousarray(x, np.float64)
    return O.log(x.reshape(-1)).reshape(x.shape) if x.size else x.copy()


def log(x):
    return float(_log_array(np.array([x], np.float64))[0])


def _div(a, b):
    """Java's a / b on doubles: no exception, IEEE results"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _sqrt(x):
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(x)))


def java_max(a, b):
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, a) < 0:
        return b
    return a if a >= b else b


def java_min(a, b):
    if a != a:
        return a
    if a == 0.0 and b == 0.0 and math.copysign(1.0, b) < 0:
        return b
    return a if a <= b else b


def kl(p1, p2):
    kl_div = 0.0
    for i in range(len(p1)):
        if p1[i] == 0:
            continue
        if p2[i] == 0:
            return INF
        kl_div += p1[i] * log(_div(p1[i], p2[i]))
    return kl_div / LN2


def manhattan(v1, v2):
    s = 0.0
    for i in range(len(v1)):
        s += abs(v1[i] - v2[i])
    return s


def euclidian(v1, v2):
    s = 0.0
    for i in range(len(v1)):
        dp = v1[i] - v2[i]
        s += dp * dp
    return _sqrt(s)


def hellinger(v1, v2):
    s = 0.0
    for i in range(len(v1)):
        dp = _sqrt(v1[i]) - _sqrt(v2[i])
        s += dp * dp
    return s


def cosine(v1, v2):
    dot = norm_a = norm_b = 0.0
    for i in range(len(v1)):
        dot += v1[i] * v2[i]
        norm_a += v1[i] * v1[i]
        norm_b += v2[i] * v2[i]
    return 1 + (-(_div(dot, _sqrt(norm_a) * _sqrt(norm_b))))


def canberra(v1, v2):
    s = 0.0
    for i in range(len(v1)):
        num = abs(v1[i] - v2[i])
        denom = abs(v1[i]) + abs(v2[i])
        s += 0.0 if denom == 0.0 else _div(num, denom)
    return s


def chebychev(v1, v2):
    m = 0.0
    for i in range(len(v1)):
        m = java_max(m, abs(v1[i] - v2[i]))
    return m


def jaccard(v1, v2):
    inter = union = 0.0
    for i in range(len(v1)):
        inter += java_min(v1[i], v2[i])
        union += java_max(v1[i], v2[i])
    return 1 - _div(inter, union) if inter > 0.0 else 0.0


def kl_distance(v1, v2):
    return (kl(v1, v2) + kl(v2, v1)) / 2


def jensen_shannon(v1, v2):
    avg = [0.0] * len(v1)
    for i in range(len(v1)):
        avg[i] += (v1[i] + v2[i]) / 2.0
    return (kl_distance(v1, avg) + kl_distance(v2, avg)) / 2


def uber(v1, v2):
    s = 0.0
    for f in (canberra, chebychev, cosine, euclidian, jaccard, kl_distance, manhattan):
        s += f(v1, v2)
    return s / 7


def mean(v):
    s = 0.0
    for x in v:
        s += x
    return _div(s, len(v))


def variance(v):
    m = mean(v)
    var = 0.0
    for a in v:
        var += (m - a) * (m - a)
    return _div(var, len(v))


def covariance(v1, v2):
    result = 0.0
    m1, m2 = mean(v1), mean(v2)
    for i in range(len(v1)):
        d1 = v1[i] - m1
        d2 = v2[i] - m2
        result += (d1 * d2 - result) / (i + 1)
    return result


def statistical(v1, v2):
    correlation = _div(covariance(v1, v2), _sqrt(variance(v1) * variance(v2)))
    return -(correlation - 1)


def bhattacharyya(v1, v2):
    of = 1.0 / 4.0
    var1, var2, mean1, mean2 = variance(v1), variance(v2), mean(v1), mean(v2)
    t1 = log(of * (_div(var1, var2) + _div(var2, var2) + 2))
    t2 = _div((mean1 - mean2) * (mean1 - mean2), var1 + var2)
    return of * t1 + of * t2


SCALAR = dict(zip(NAMES, (manhattan, euclidian, hellinger, cosine, canberra, chebychev, jaccard, kl_distance, jensen_shannon, uber,
                          statistical, bhattacharyya)))


def calculate(name, v1, v2):
    """Distance.calculate of the class `name` on two sequences of floats"""
    return SCALAR[name]([float(x) for x in v1], [float(x) for x in v2])


# ---- all pairs at once: out[q][d] = calculate(A[d], B[q]) ---------------------------------------------------------------
def _jmax(a, b):
    r = np.where(a >= b, a, b)                          # a NaN b comes through: a >= NaN is false
    r = np.where((a == 0.0) & (b == 0.0) & np.signbit(a), b, r)
    return np.where(a != a, a, r)


def _jmin(a, b):
    r = np.where(a <= b, a, b)
    r = np.where((a == 0.0) & (b == 0.0) & np.signbit(b), b, r)
    return np.where(a != a, a, r)


class _Kl:
    """klDivergence for all pairs: the sum and the latched early return"""

    def __init__(self, shape):
        self.s = np.zeros(shape)
        self.inf = np.zeros(shape, bool)

    def step(self, p1, p2):
        live = p1 != 0
        self.inf |= live & (p2 == 0)
        add = live & (p2 != 0)                          # a NaN p2 is not 0: its addend is NaN, as in the loop
        if add.any():
            term = np.zeros(self.s.shape)
            term[add] = p1[add] * _log_array(p1[add] / p2[add])
            self.s = np.where(add, self.s + term, self.s)

    def value(self):
        return np.where(self.inf, INF, self.s / LN2)


def _row_moments(M):
    n = M.shape[1]
    s = np.zeros(M.shape[0])
    for i in range(n):
        s = s + M[:, i]
    m = s / n
    var = np.zeros(M.shape[0])
    for i in range(n):
        var = var + (m - M[:, i]) * (m - M[:, i])
    return m, var / n


def pairwise(name, A, B):
    A, B = np.ascontiguousarray(A, np.float64), np.ascontiguousarray(B, np.float64)
    n, m, length = A.shape[0], B.shape[0], A.shape[1]
    shape = (m, n)
    with np.errstate(all="ignore"):
        def cols(i):
            return np.broadcast_to(A[None, :, i], shape), np.broadcast_to(B[:, None, i], shape)
        z = lambda: np.zeros(shape)   # noqa: E731
        manh, eucl, canb, cheb, dot, inter, union, hell, cov = z(), z(), z(), z(), z(), z(), z(), z(), z()
        k_ab, k_ba = _Kl(shape), _Kl(shape)
        js = [_Kl(shape) for _ in range(4)]
        want = {name} if name != "UberDistance" else {"CanberraDistance", "ChebychevDistance", "CosineDistance", "EuclidianDistance", "JaccardDistance",
                                                      "KLDistance", "ManhattanDistance"}
        if name in ("StatisticalDistance", "BhattacharyyaDistance"):
            ma, va = _row_moments(A)
            mb, vb = _row_moments(B)
        if "CosineDistance" in want:
            na, nb = np.zeros(n), np.zeros(m)
            for i in range(length):
                na = na + A[:, i] * A[:, i]
                nb = nb + B[:, i] * B[:, i]
        for i in range(length if name != "BhattacharyyaDistance" else 0):
            a, b = cols(i)
            if "ManhattanDistance" in want:
                manh = manh + np.abs(a - b)
            if "EuclidianDistance" in want:
                eucl = eucl + (a - b) * (a - b)
            if "HellingerDistance" in want:
                dp = np.sqrt(a) - np.sqrt(b)
                hell = hell + dp * dp
            if "CosineDistance" in want:
                dot = dot + a * b
            if "CanberraDistance" in want:
                num, den = np.abs(a - b), np.abs(a) + np.abs(b)
                canb = canb + np.where(den == 0.0, 0.0, num / np.where(den == 0.0, 1.0, den))
            if "ChebychevDistance" in want:
                cheb = _jmax(cheb, np.abs(a - b))
            if "JaccardDistance" in want:
                inter, union = inter + _jmin(a, b), union + _jmax(a, b)
            if "KLDistance" in want:
                k_ab.step(a, b)
                k_ba.step(b, a)
            if "JensenShannonDistance" in want:
                avg = 0.0 + (a + b) / 2.0
                js[0].step(a, avg), js[1].step(avg, a), js[2].step(b, avg), js[3].step(avg, b)
            if "StatisticalDistance" in want:
                cov = cov + ((a - ma[None, :]) * (b - mb[:, None]) - cov) / (i + 1)
        v = {}
        v["ManhattanDistance"] = manh
        v["EuclidianDistance"] = np.sqrt(eucl)
        v["HellingerDistance"] = hell
        v["CanberraDistance"] = canb
        v["ChebychevDistance"] = cheb
        if "CosineDistance" in want:
            v["CosineDistance"] = 1 + (-(dot / (np.sqrt(na)[None, :] * np.sqrt(nb)[:, None])))
        v["JaccardDistance"] = np.where(inter > 0.0, 1 - (inter / union), 0.0)
        v["KLDistance"] = (k_ab.value() + k_ba.value()) / 2
        if name == "JensenShannonDistance":
            return ((js[0].value() + js[1].value()) / 2 + (js[2].value() + js[3].value()) / 2) / 2
        if name == "StatisticalDistance":
            return -(cov / np.sqrt(va[None, :] * vb[:, None]) - 1)
        if name == "BhattacharyyaDistance":
            of = 1.0 / 4.0
            v1, v2, m1, m2 = (np.broadcast_to(x, shape) for x in (va[None, :], vb[:, None], ma[None, :], mb[:, None]))
            t1 = _log_array(of * (v1 / v2 + v2 / v2 + 2))
            t2 = ((m1 - m2) * (m1 - m2)) / (v1 + v2)
            return of * t1 + of * t2
        if name == "UberDistance":
            s = np.zeros(shape)
            for part in ("CanberraDistance", "ChebychevDistance", "CosineDistance", "EuclidianDistance", "JaccardDistance", "KLDistance", "ManhattanDistance"):
                s = s + v[part]
            return s / 7
        return np.array(v[name])


def apply_length_rule(dist, train_len, query_len):
    """LDADistancer.java:84-87 on dist [Q][D]: both documents empty 0.0, exactly one +Infinity"""
    out = np.array(dist, np.float64)
    te = np.asarray(train_len)[None, :] == 0
    qe = (np.asarray(query_len)[:, None] == 0) if query_len is not None else np.zeros((out.shape[0], 1), bool)
    out[te | qe] = INF
    out[te & qe] = 0.0
    return out


# ---- the n nearest ---------------------------------------------------------------------------------------------------------
def nearest(dist_rows, n, base=0):
    """(idx [Q][n], dist [Q][n]) ordered by (distance rising by value, index rising); only a distance < +Infinity is a candidate;
    unfilled places hold -1 and +Infinity."""
    dist_rows = np.asarray(dist_rows, np.float64)
    idx = np.full((dist_rows.shape[0], n), -1, np.int64)
    out = np.full((dist_rows.shape[0], n), INF)
    for q, row in enumerate(dist_rows):
        cand = [(float(d) + 0.0, i) for i, d in enumerate(row) if d < INF]      # -0.0 + 0.0 = 0.0: by value
        cand.sort()
        for r, (_, i) in enumerate(cand[:n]):
            idx[q, r], out[q, r] = base + i, row[i]
    return idx, out


def java_nearest_one(row):
    """tui/LDASimilarity.java:175-183: minDist = +Infinity, minIdx = -1; strict minDist > d"""
    min_dist, min_idx = INF, -1
    for i, d in enumerate(row):
        if min_dist > d:
            min_dist, min_idx = d, i
    return min_idx, min_dist


# ---- KLDivergenceClassifier --------------------------------------------------------------------------------------------------
def centroids(zbar, labels, alpha):
    """calculateCentroids (:154-186): per class, in order of first appearance, the z-bar rows summed in document order, then
    (sum + alpha) / count.  Returns (class names, [C][K])."""
    names, sums, counts = [], {}, {}
    for d, name in enumerate(labels):
        if name not in sums:
            names.append(name)
            sums[name] = [0.0] * len(zbar[d])
            counts[name] = 0
        counts[name] += 1
        for k in range(len(zbar[d])):
            sums[name][k] += float(zbar[d][k])
    return names, np.array([[_div(sums[c][k] + alpha, float(counts[c])) for k in range(len(sums[c]))] for c in names])


def classifier_query_row(zbar_row, alpha):
    """classify (:57-64): sum = MatrixOps.sum(row), taken as the sequential sum; row[i] = (row[i] + alpha) / sum"""
    s = 0.0
    for x in zbar_row:
        s += float(x)
    return np.array([_div(float(x) + alpha, s) for x in zbar_row])


def first_maximum(scores):
    """the label of a score vector: max = values[0], a later value wins only when it is > max (a NaN never is)"""
    best = 0
    for c in range(1, len(scores)):
        if scores[c] > scores[best]:
            best = c
    return best


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)
