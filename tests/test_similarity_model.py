"""The restated distance classes (tests/similarity_restatement.py) against what the reference itself asserts and against values
worked by hand; the all-pairs form the GPU tests compare the kernels with against the scalar loops, bit for bit; the order of
the n nearest; merge_nearest; and the metric ids of the header, the ctypes table and the registry.  No GPU."""
import itertools
import json
import math
import os
import re

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import _lib
from tests import similarity_restatement as R

HERE = os.path.dirname(os.path.abspath(__file__))
INF, NAN = float("inf"), float("nan")


def jbits(x):
    x = np.ascontiguousarray(x, np.float64)
    b = x.view(np.int64).copy()
    b[np.isnan(x)] = 0x7ff8000000000000
    return b


# ---- the reference's own (ignored) SimilarityTest ----------------------------------------------------------------------------
GOLDEN = json.load(open(os.path.join(HERE, "golden", "similarity_vectors.json")))


@pytest.mark.parametrize("name", GOLDEN["classes"])
def test_the_reference_tests_three_assertions(name):
    assert name in R.NAMES
    v1, v2, one = GOLDEN["v1"], GOLDEN["not_same"], GOLDEN["vs_one"]
    same = R.calculate(name, v1, v1)
    assert same < GOLDEN["same_below"]
    assert R.calculate(name, v1, v2) > same
    assert R.calculate(name, v1, one) > same
    if name == "KLDistance":
        assert R.calculate(name, v1, one) == INF


# ---- hand-worked values --------------------------------------------------------------------------------------------------------
def test_hand_worked_values():
    a, b = [0.5, 0.5], [0.25, 0.75]
    assert R.manhattan(a, b) == 0.5
    want = (0.5 * R.log(0.5 / 0.25) + 0.5 * R.log(0.5 / 0.75)) / R.LN2
    assert R.kl(a, b) == want and abs(want - (0.5 * 1.0 + 0.5 * math.log2(2.0 / 3.0))) < 1e-15
    assert R.LN2.hex() == "0x1.62e42fefa39efp-1" and np.float64(R.LN2).view(np.int64) == 0x3FE62E42FEFA39EF
    assert R.kl_distance(a, b) == (R.kl(a, b) + R.kl(b, a)) / 2
    # Hellinger is the sum itself: no root, no 1/2
    assert R.hellinger([0.25, 0.0], [1.0, 0.0]) == 0.25 and R.hellinger([0.0, 1.0], [1.0, 0.0]) == 2.0
    # Bhattacharyya keeps var2 / var2: with var1 == var2 the log term is log(1/4 * (1 + 1 + 2)) = 0 and the mean term stays
    v1, v2 = [0.0, 2.0], [1.0, 3.0]                                  # means 1 and 2, variances 1 and 1
    assert R.bhattacharyya(v1, v2) == 0.25 * R.log(1.0) + 0.25 * (1.0 / 2.0) == 0.125
    assert math.isnan(R.bhattacharyya(v1, [2.0, 2.0]))               # var2 == 0: 0 / 0
    assert R.euclidian([0.0, 3.0], [4.0, 0.0]) == 5.0
    assert R.chebychev([0.1, 0.9], [0.4, 0.5]) == abs(0.9 - 0.5)
    assert R.canberra([0.0, 1.0], [0.0, 3.0]) == 0.5                  # the 0 / 0 term is 0.0
    assert R.jaccard([1.0, 2.0], [2.0, 1.0]) == 1 - 2.0 / 4.0 and R.jaccard([0.0, 0.0], [1.0, 1.0]) == 0.0
    assert abs(R.cosine([1.0, 0.0], [0.0, 1.0]) - 1.0) == 0.0 and abs(R.cosine([1.0, 2.0], [2.0, 4.0])) < 1e-15
    assert abs(R.statistical([1.0, 2.0, 3.0], [2.0, 4.0, 6.0])) < 1e-15 and abs(R.statistical([1.0, 2.0, 3.0], [3.0, 2.0, 1.0]) - 2.0) < 1e-15
    x, y = [0.2, 0.3, 0.5], [0.1, 0.6, 0.3]
    parts = [R.canberra(x, y), R.chebychev(x, y), R.cosine(x, y), R.euclidian(x, y), R.jaccard(x, y), R.kl_distance(x, y), R.manhattan(x, y)]
    s = 0.0
    for p in parts:
        s += p
    assert R.uber(x, y) == s / 7
    avg = [(p + q) / 2.0 for p, q in zip(x, y)]
    assert R.jensen_shannon(x, y) == (R.kl_distance(x, avg) + R.kl_distance(y, avg)) / 2


# ---- edge cases ----------------------------------------------------------------------------------------------------------------
def test_kl_early_return_and_skip():
    assert R.kl([0.5, NAN, 0.5], [0.5, 0.5, 0.0]) == INF               # at the first p2 == 0, even after a NaN addend
    assert R.kl([0.5, 0.5, NAN], [0.0, 0.5, 0.5]) == INF               # ... and whatever comes after
    assert R.kl([0.0, 1.0], [0.0, 1.0]) == 0.0                          # p1 == 0 is skipped before p2 is looked at
    assert R.kl([0.0, 1.0], [0.7, 1.0]) == 0.0
    assert math.isnan(R.kl([0.5, 0.5], [NAN, 0.5]))                     # a NaN p2 is not 0
    assert R.kl([-0.0, 1.0], [0.0, 1.0]) == 0.0


def test_java_max_and_min():
    assert math.isnan(R.java_max(NAN, 1.0)) and math.isnan(R.java_max(1.0, NAN)) and math.isnan(R.java_min(NAN, 1.0)) and math.isnan(R.java_min(1.0, NAN))
    assert math.copysign(1.0, R.java_max(-0.0, 0.0)) == 1.0 and math.copysign(1.0, R.java_max(0.0, -0.0)) == 1.0
    assert math.copysign(1.0, R.java_min(-0.0, 0.0)) == -1.0 and math.copysign(1.0, R.java_min(0.0, -0.0)) == -1.0
    assert R.java_max(1.0, 2.0) == 2.0 and R.java_min(1.0, 2.0) == 1.0
    assert math.isnan(R.chebychev([0.1, NAN, 0.3], [0.1, 0.2, 0.9])) and math.isnan(R.chebychev([0.1, 0.2], [NAN, 0.2]))
    assert R.jaccard([0.1, NAN, 0.3], [0.1, 0.2, 0.9]) == 0.0           # a NaN intersection is not > 0.0


# ---- the all-pairs form is the scalar loops -------------------------------------------------------------------------------------
def special_rows():
    rng = np.random.default_rng(5)
    a, b = rng.dirichlet(np.full(9, 0.3), 12), rng.dirichlet(np.full(9, 0.3), 10)
    b[9] = a[2]
    a[1] = 0.0
    b[1] = 0.0
    a[3, [1, 4]] = 0.0
    b[3, [0, 4]] = 0.0
    a[4] = 5e-324
    b[4, :5] = 5e-324
    a[5] = NAN
    b[5, 6] = NAN
    a[6] = 1.0 / 9
    b[6] = 0.25
    a[7, 2] = -0.0
    b[7] = -0.0
    return a, b


@pytest.mark.parametrize("name", R.NAMES)
def test_pairwise_is_the_scalar_loops(name):
    a, b = special_rows()
    got = R.pairwise(name, a, b)
    want = np.array([[R.calculate(name, a[d], b[q]) for d in range(len(a))] for q in range(len(b))])
    bad = np.argwhere(jbits(got) != jbits(want))
    assert bad.size == 0, "%s: first at %s: %r vs %r" % (name, bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def test_length_rule():
    d = np.arange(6.0).reshape(2, 3)
    out = R.apply_length_rule(d, [3, 0, 2], [0, 4])
    assert out.tolist() == [[INF, 0.0, INF], [3.0, INF, 5.0]]
    assert R.apply_length_rule(d, [3, 0, 2], None).tolist() == [[0.0, INF, 2.0], [3.0, INF, 5.0]]


# ---- the n nearest --------------------------------------------------------------------------------------------------------------
def test_nearest_order_and_padding():
    rows = np.array([[0.5, 0.25, 0.25, INF, NAN, 0.0, -0.0, 0.75],
                     [INF, NAN, INF, NAN, INF, NAN, INF, NAN]])
    idx, dist = R.nearest(rows, 5)
    assert idx[0].tolist() == [5, 6, 1, 2, 0] and math.copysign(1.0, dist[0, 0]) == 1.0 and math.copysign(1.0, dist[0, 1]) == -1.0
    assert dist[0, 2:].tolist() == [0.25, 0.25, 0.5]
    assert idx[1].tolist() == [-1] * 5 and dist[1].tolist() == [INF] * 5
    idx, dist = R.nearest(rows[:1, :3], 5, base=100)
    assert idx[0].tolist() == [101, 102, 100, -1, -1] and dist[0].tolist() == [0.25, 0.25, 0.5, INF, INF]


def test_nearest_one_is_the_java_loop():
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 4, (50, 9)).astype(np.float64)             # many ties
    rows[rng.random(rows.shape) < 0.2] = INF
    rows[rng.random(rows.shape) < 0.1] = NAN
    rows[7] = INF
    idx, dist = R.nearest(rows, 1)
    for q, row in enumerate(rows):
        i, d = R.java_nearest_one(row)
        assert idx[q, 0] == i and jbits(dist[q, 0]) == jbits(d)


def test_merge_nearest_over_any_split_is_nearest_over_the_whole():
    from ldagroupedgibbssampler_amd.similarity import merge_nearest
    rng = np.random.default_rng(2)
    rows = rng.integers(0, 5, (6, 23)).astype(np.float64)
    rows[rng.random(rows.shape) < 0.15] = INF
    rows[rng.random(rows.shape) < 0.1] = NAN
    rows[0, 3], rows[0, 11] = 0.0, -0.0
    rows[5] = NAN
    for n in (1, 4, 16):
        want = R.nearest(rows, n)
        for cuts in itertools.chain([(0, 23)], [(0, c, 23) for c in (1, 7, 22)], [(0, 5, 5, 9, 23), (0, 2, 11, 12, 23)]):
            parts = [R.nearest(rows[:, lo:hi], n, base=lo) for lo, hi in zip(cuts, cuts[1:])]
            for order in (parts, parts[::-1]):
                idx, dist = merge_nearest(order, n)
                assert np.array_equal(idx, want[0]) and np.array_equal(jbits(dist), jbits(want[1])), (n, cuts)


def test_centroids_and_query_row():
    zbar = np.array([[0.5, 0.5], [1.0, 0.0], [0.25, 0.75], [0.0, 0.0]])
    names, cent = R.centroids(zbar, ["b", "a", "b", "a"], 0.1)
    assert names == ["b", "a"]
    assert cent.tolist() == [[(0.5 + 0.25 + 0.1) / 2.0, (0.5 + 0.75 + 0.1) / 2.0], [(1.0 + 0.0 + 0.1) / 2.0, (0.0 + 0.0 + 0.1) / 2.0]]
    assert R.classifier_query_row([0.25, 0.75], 0.1).tolist() == [(0.25 + 0.1) / 1.0, (0.75 + 0.1) / 1.0]
    assert np.isinf(R.classifier_query_row([0.0, 0.0], 0.1)).all()    # an empty document: sum(zbar) == 0
    assert R.first_maximum([NAN, 1.0, 2.0]) == 0 and R.first_maximum([1.0, 3.0, 3.0]) == 1


# ---- ids -----------------------------------------------------------------------------------------------------------------------------
def test_metric_ids_agree_and_the_abi_version_stays():
    from ldagroupedgibbssampler_amd import similarity
    header = open(_lib.HEADER_PATH).read()
    ids = {m.group(2): int(m.group(1)) for m in re.finditer(r"#define GGS_DISTANCE_[A-Z_]+ +(\d+) +/\* (\w+Distance)", header)}
    assert ids == _lib.DISTANCE_IDS == similarity.DISTANCES
    assert [n for n, _ in sorted(ids.items(), key=lambda kv: kv[1])] == list(R.NAMES)
    assert re.search(r"#define GGS_DISTANCE_COUNT +12\b", header) and re.search(r"#define GGS_NEAREST_MAX +16\b", header)
    assert _lib.NEAREST_MAX == 16 and similarity.NEAREST_MAX == 16
    assert re.search(r"#define GGS_ABI_VERSION +6\b", header) and _lib.ABI_VERSION == 6
    kernels = open(os.path.join(_lib.CSRC, "ggs_similarity.hpp")).read()
    r = re.search(r"kSimR\[kSimMetrics\] = \{([^}]*)\}", kernels).group(1)
    edges = [16 * int(x) for x in r.split(",")]
    assert edges == [32 if n in ("KLDistance", "JensenShannonDistance", "UberDistance") else 64 for n in R.NAMES]   # what the GPU tests' shape lists assume
    assert re.search(r"kSimKC = 32;", kernels)
    for name in ("ggs_get_theta_estimate", "ggs_get_zbar", "ggs_nearest_documents", "ggs_document_distances", "ggs_row_distances"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
