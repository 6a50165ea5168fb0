"""The distance family and the n nearest of csrc/ggs_similarity.hpp against the restated Java (tests/similarity_restatement.py),
bit for bit; the device getters of the theta estimate and z-bar against the samplers' host versions; LDADistancer,
KLDivergenceClassifier and ShardedGGS.nearest_documents end to end.

"Bit for bit" is Double.doubleToLongBits: a NaN compares as NaN (Java has one canonical NaN; the payload and sign a device or
a host gives 0.0 / 0.0 are not part of the reference's result), every other value by its 64 bits, -0.0 apart from 0.0.

Tile edges: 16 * kSimR[metric] rows (64, and 32 for KL, Jensen-Shannon and Uber); the index runs in chunks of kSimKC = 32.
The reference of a shape list is computed once, for the largest block, and sliced: the rows of a smaller block are a prefix."""
import functools
import os

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus
from ldagroupedgibbssampler_amd.sampler import calc_theta_estimate
from tests import min_distances_restatement as MR
from tests import similarity_restatement as R
from tests.ranks import Transport, assert_bit_equal, run_ranks

pytestmark = pytest.mark.gpu

KC = 32
TILE = {name: 32 if name in ("KLDistance", "JensenShannonDistance", "UberDistance") else 64 for name in R.NAMES}
LENS = [1, 2, 3, 7, 100, KC - 1, KC, KC + 1, 1030]
MIN_VALUE = 5e-324
SEED, ZSEED = 17, 23


def sizes(T):
    return [1, 2, T - 1, T, T + 1, 2 * T + 1]


def jbits(x):
    """Double.doubleToLongBits"""
    x = np.ascontiguousarray(x, np.float64)
    b = x.view(np.int64).copy()
    b[np.isnan(x)] = 0x7ff8000000000000
    return b


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shapes %s and %s" % (what, got.shape, want.shape)
    bad = jbits(got) != jbits(want)
    if bad.any():
        first = np.unravel_index(np.flatnonzero(bad)[0], got.shape)
        raise AssertionError("%s: %d of %d differ, first at %s: %r vs %r" % (what, bad.sum(), bad.size, [int(i) for i in first], got[first], want[first]))


@functools.lru_cache(maxsize=None)
def block(name, length):
    """(A, B, the reference [m][n]) of the largest block of a metric at a row length"""
    n = 2 * TILE[name] + 1
    a, b = MR.dirichlet_rows(n, length, 1), MR.dirichlet_rows(n, length, 2)
    want = R.pairwise(name, a, b)
    want.setflags(write=False)
    return a, b, want


# ---- shapes, through ggs_row_distances --------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", LENS)
@pytest.mark.parametrize("name", ["ManhattanDistance", "KLDistance"])
def test_every_shape(native, name, length):
    a, b, want = block(name, length)
    for n in sizes(TILE[name]):
        for m in sizes(TILE[name]):
            assert_same(native.row_distances(a[:n], b[:m], name), want[:m, :n], "%s n=%d m=%d len=%d" % (name, n, m, length))


@pytest.mark.parametrize("name", [x for x in R.NAMES if x not in ("ManhattanDistance", "KLDistance")])
def test_a_diagonal_of_the_shapes(native, name):
    ns = sizes(TILE[name])
    for i, length in enumerate(LENS):
        n, m = ns[i % 6], ns[(i + 2) % 6]
        a, b = MR.dirichlet_rows(n, length, 3), MR.dirichlet_rows(m, length, 4)
        assert_same(native.row_distances(a, b, name), R.pairwise(name, a, b), "%s n=%d m=%d len=%d" % (name, n, m, length))


# ---- built rows, every metric -----------------------------------------------------------------------------------------------
def built_rows():
    a, b = MR.dirichlet_rows(140, 12, 5), MR.dirichlet_rows(70, 12, 6)
    b[69] = a[2]                                       # identical rows, in different tiles of either edge
    b[3] = a[139]
    a[10] = 0.0                                        # an all-zero row on either side
    b[11] = 0.0
    a[20, [1, 4]] = 0.0                                # exact zeros in v1 only, ...
    b[21, [0, 7]] = 0.0                                # ... in v2 only, ...
    a[22, 5] = b[22, 5] = 0.0                          # ... and at the same index in both (rows 22 meet)
    a[23, :3] = b[23, :3] = 0.0
    a[30][a[30] < 0.05] = MIN_VALUE                    # Double.MIN_VALUE entries
    b[31][b[31] < 0.05] = MIN_VALUE
    a[32] = MIN_VALUE
    b[32] = MIN_VALUE
    b[33] = 2 * MIN_VALUE
    a[40] = np.nan                                     # a NaN row, and a single NaN element
    b[41, 6] = np.nan
    a[42, 0] = np.nan
    a[50] = 1.0 / 12                                   # a constant row: variance 0
    b[51] = 0.25
    a[52] = -0.0
    b[52, 3] = -0.0
    return a, b


@pytest.mark.parametrize("name", R.NAMES)
def test_built_rows(native, name):
    a, b = built_rows()
    got = native.row_distances(a, b, name)
    want = R.pairwise(name, a, b)
    assert_same(got, want, name)
    if name in ("ManhattanDistance", "EuclidianDistance", "HellingerDistance", "KLDistance", "JensenShannonDistance"):
        assert got[69, 2] == 0.0 and got[3, 139] == 0.0                  # the identical rows
    if name == "ChebychevDistance":
        assert np.isnan(got[:, 40]).all() and np.isnan(got[41]).all()
    if name == "JaccardDistance":
        assert (got[:, 40] == 0.0).all() and (got[41] == 0.0).all()
    if name == "KLDistance":
        assert np.isinf(got[5, 20]) and np.isinf(got[21, 5]) and np.isfinite(got[22, 22])


def test_row_distances_bad_arguments(native):
    L, p = native._lib.load(), native._dp
    a, out = np.zeros((4, 3)), np.zeros(16)
    assert L.ggs_row_distances(0, 12, p(a), p(a), 4, 4, 3, p(out)) == native.ERR_BAD_ARG
    assert L.ggs_row_distances(0, -1, p(a), p(a), 4, 4, 3, p(out)) == native.ERR_BAD_ARG
    assert L.ggs_row_distances(0, 0, p(a), p(a), -1, 4, 3, p(out)) == native.ERR_BAD_ARG
    assert L.ggs_row_distances(0, 0, p(a), p(a), 4, 4, 0, p(out)) == native.ERR_BAD_ARG
    assert L.ggs_row_distances(0, 0, p(a), p(a), 4, 4, 3, None) == native.ERR_BAD_ARG
    assert L.ggs_row_distances(0, 0, p(a), p(a), 0, 4, 3, p(out)) == 0


# ---- selection, through ggs_nearest_documents -------------------------------------------------------------------------------
def corpus_with_z(D, K, seed, empty=(), same=()):
    """(corpus, z): D documents of 1 .. 40 tokens over 50 types with a random z; `empty` documents have no token; `same` lists
    (i, j): document j gets document i's length and z, hence its theta estimate"""
    rng = np.random.default_rng([D, K, seed])
    lens = rng.integers(1, 41, D)
    lens[list(empty)] = 0
    for i, j in same:
        lens[j] = lens[i]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = rng.integers(0, 50, int(ptr[-1])).astype(np.int32)
    z = rng.integers(0, K, int(ptr[-1])).astype(np.int32)
    for i, j in same:
        z[ptr[j]:ptr[j + 1]] = z[ptr[i]:ptr[i + 1]]
    return Corpus(ptr, tokens, 50), z


def handle_of(native, corpus, z, K, alpha=0.1, scheme="spalias", doc_base=0):
    h = native.GGSHandle(K, corpus.num_types, alpha, 0.01, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens, doc_base)
    h.set_z(z, redraw_phi=False)
    return h


def theta_rows(corpus, z, K, alpha):
    p = corpus.doc_ptr
    return np.stack([calc_theta_estimate(K, alpha, z[p[d]:p[d + 1]]) for d in range(corpus.num_docs)])


def expected(name, corpus, z, K, alpha, query, query_len=None):
    return R.apply_length_rule(R.pairwise(name, theta_rows(corpus, z, K, alpha), query), np.diff(corpus.doc_ptr), query_len)


def check_nearest(h, name, want_dist, query, n, query_len=None, base=0, what=""):
    idx, dist = h.nearest_documents(query, n, name, query_len)
    want_idx, want = R.nearest(want_dist, n, base)
    assert np.array_equal(idx, want_idx), "%s %s n=%d: indices\n%r\n%r" % (what, name, n, idx, want_idx)
    assert_same(dist, want, "%s %s n=%d" % (what, name, n))
    return idx, dist


@pytest.mark.parametrize("name", ["ManhattanDistance", "KLDistance"])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 257])
def test_nearest_sizes_and_padding(native, name, D):
    K = 7
    corpus, z = corpus_with_z(D, K, 1)
    h = handle_of(native, corpus, z, K)
    query = MR.dirichlet_rows(70, K, 9)
    want = expected(name, corpus, z, K, 0.1, query)
    for n in (1, 2, 16):
        idx, _ = check_nearest(h, name, want, query, n, what="D=%d" % D)
        if n > D:
            assert (idx[:, D:] == -1).all()
    one = [R.java_nearest_one(row) for row in want]                  # n = 1 is the loop of LDASimilarity.java:175-183
    idx, dist = h.nearest_documents(query, 1, name)
    assert idx[:, 0].tolist() == [i for i, _ in one]
    assert_same(dist[:, 0], np.array([d for _, d in one]), "the Java loop")
    h.close()


@pytest.mark.parametrize("name", ["ManhattanDistance", "KLDistance", "UberDistance", "CosineDistance"])
def test_ties_go_to_the_lower_index_across_tiles_and_segments(native, name, monkeypatch):
    K, D = 6, 300
    same = [(3, 70), (3, 299), (3, 131), (40, 41), (200, 100)]
    corpus, z = corpus_with_z(D, K, 2, same=same)
    query = theta_rows(corpus, z, K, 0.1)[[3, 40, 200, 7]] * (1 + 2.0 ** -40)   # next to the duplicated documents
    want = expected(name, corpus, z, K, 0.1, query)
    outs = []
    for segs in ("1", "1000000", None):
        if segs is None:
            monkeypatch.delenv("GGS_DEBUG_SIM_SEGMENTS", raising=False)
        else:
            monkeypatch.setenv("GGS_DEBUG_SIM_SEGMENTS", segs)
        h = handle_of(native, corpus, z, K)
        outs.append(check_nearest(h, name, want, query, 5, what="segments=%s" % segs))
        h.close()
    idx = outs[0][0]
    assert idx[0, :4].tolist() == [3, 70, 131, 299] and idx[1, :2].tolist() == [40, 41] and idx[2, :2].tolist() == [100, 200]
    for o in outs[1:]:
        assert np.array_equal(o[0], idx) and np.array_equal(jbits(o[1]), jbits(outs[0][1]))


@pytest.mark.parametrize("name", R.NAMES)
def test_segment_independence(native, name, monkeypatch):
    """the same call with the segment count forced to 1 and to its maximum: identical output, and the restatement's"""
    K, D = 9, 200
    corpus, z = corpus_with_z(D, K, 3, empty=(0, 77, 199))
    query = MR.dirichlet_rows(40, K, 11)
    query[5, 2] = 0.0
    qlen = np.full(40, 3, np.int64)
    qlen[[1, 39]] = 0
    want = expected(name, corpus, z, K, 0.1, query, qlen)
    got = []
    for segs in ("1", "1000000"):
        monkeypatch.setenv("GGS_DEBUG_SIM_SEGMENTS", segs)
        h = handle_of(native, corpus, z, K)
        got.append(check_nearest(h, name, want, query, 16, qlen, what="segments=%s" % segs))
        assert_same(h.document_distances(query, name, qlen), want, "%s dense, segments=%s" % (name, segs))
        h.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(jbits(got[0][1]), jbits(got[1][1]))


def test_nearest_in_the_last_row_of_a_ragged_tile(native):
    K, D = 8, 2 * 64 + 3
    corpus, z = corpus_with_z(D, K, 4)
    rows = theta_rows(corpus, z, K, 0.1)
    query = rows[[D - 1]] * (1 - 2.0 ** -30)
    for name in ("ManhattanDistance", "KLDistance"):
        h = handle_of(native, corpus, z, K)
        idx, _ = check_nearest(h, name, expected(name, corpus, z, K, 0.1, query), query, 3)
        assert idx[0, 0] == D - 1
        h.close()


def test_a_query_without_a_finite_distance_finds_nothing(native):
    K, D = 5, 70
    corpus, z = corpus_with_z(D, K, 5)
    query = MR.dirichlet_rows(3, K, 1)
    query[1, 2] = 0.0                                  # kl(v1, v2) returns +Infinity against every training row (all > 0)
    h = handle_of(native, corpus, z, K)
    idx, dist = check_nearest(h, "KLDistance", expected("KLDistance", corpus, z, K, 0.1, query), query, 4)
    assert (idx[1] == -1).all() and np.isinf(dist[1]).all() and (idx[[0, 2]] >= 0).all()
    h.close()


def test_empty_documents_on_either_side_and_on_both(native):
    K, D = 5, 70
    corpus, z = corpus_with_z(D, K, 6, empty=(4, 66))
    query = MR.dirichlet_rows(4, K, 2)
    qlen = np.array([5, 0, 9, 0], np.int64)
    h = handle_of(native, corpus, z, K)
    for name in ("ManhattanDistance", "KLDistance", "BhattacharyyaDistance"):
        want = expected(name, corpus, z, K, 0.1, query, qlen)
        assert (want[1, [4, 66]] == 0.0).all() and np.isinf(np.delete(want[1], [4, 66])).all() and np.isinf(want[0, [4, 66]]).all()
        assert_same(h.document_distances(query, name, qlen), want, name)
        idx, dist = check_nearest(h, name, want, query, 3, qlen)
        assert idx[1].tolist() == [4, 66, -1] and dist[1].tolist() == [0.0, 0.0, np.inf] and 4 not in idx[0] and 66 not in idx[0]
    h.close()


def test_global_indices_and_pieces(native, monkeypatch):
    """doc_base enters the indices; training rows, queries and the [Q][D] output in several pieces change nothing"""
    K, D = 6, 150
    corpus, z = corpus_with_z(D, K, 7, empty=(9,))
    query = MR.dirichlet_rows(90, K, 3)
    want = expected("KLDistance", corpus, z, K, 0.1, query)
    monkeypatch.setenv("GGS_DEBUG_SIM_PIECE_BYTES", str(12 * K * 40))           # 40 documents, 60 queries (dense: 1) a piece
    h = handle_of(native, corpus, z, K, doc_base=1000)
    check_nearest(h, "KLDistance", want, query, 16, base=1000)
    assert_same(h.document_distances(query, "KLDistance"), want, "dense in pieces")
    assert_same(h.theta_estimate(), theta_rows(corpus, z, K, 0.1), "theta estimate in pieces")
    h.close()


def test_state_and_argument_errors(native):
    corpus, z = corpus_with_z(20, 4, 8)
    h = native.GGSHandle(4, corpus.num_types, 0.1, 0.01, SEED)
    L, dp, lp = native._lib.load(), native._dp, native._lp
    q, idx, dist, rows = np.full((2, 4), 0.25), np.zeros((2, 16), np.int64), np.zeros((2, 20)), np.zeros((20, 4))
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 2, 1, lp(idx), dp(dist)) == native.ERR_STATE
    assert L.ggs_document_distances(h._h, 0, dp(q), None, 2, dp(dist)) == native.ERR_STATE
    assert L.ggs_get_theta_estimate(h._h, 0, 20, dp(rows)) == native.ERR_STATE
    assert L.ggs_get_zbar(h._h, 0, 20, dp(rows)) == native.ERR_STATE
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 2, 1, lp(idx), dp(dist)) == native.ERR_STATE      # a corpus, no z yet
    assert L.ggs_document_distances(h._h, 0, dp(q), None, 2, dp(dist)) == native.ERR_STATE
    assert L.ggs_get_theta_estimate(h._h, 0, 20, dp(rows)) == native.ERR_STATE
    assert L.ggs_get_zbar(h._h, 0, 20, dp(rows)) == native.ERR_STATE
    h.set_z(z, redraw_phi=False)
    bad = native.ERR_BAD_ARG
    assert L.ggs_nearest_documents(h._h, 12, dp(q), None, 2, 1, lp(idx), dp(dist)) == bad
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 2, 0, lp(idx), dp(dist)) == bad
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 2, 17, lp(idx), dp(dist)) == bad
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, -1, 1, lp(idx), dp(dist)) == bad
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 2, 1, None, dp(dist)) == bad
    assert L.ggs_nearest_documents(h._h, 0, None, None, 2, 1, lp(idx), dp(dist)) == bad
    assert L.ggs_document_distances(h._h, 0, dp(q), None, 2, None) == bad
    assert L.ggs_get_theta_estimate(h._h, 0, 21, dp(rows)) == bad
    assert L.ggs_get_zbar(h._h, 0, 20, None) == bad
    assert L.ggs_nearest_documents(h._h, 0, dp(q), None, 0, 1, lp(idx), dp(dist)) == 0
    h.close()
    empty = native.GGSHandle(4, 10, 0.1, 0.01, SEED)
    empty.set_corpus(np.zeros(1, np.int64), np.zeros(0, np.int32))
    i, d = empty.nearest_documents(q, 3, "ManhattanDistance")
    assert (i == -1).all() and np.isinf(d).all()
    empty.close()


# ---- handle level -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 100, 1024])
@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "spalias", "collapsed", "adlda"])
def test_device_getters_equal_the_samplers(native, scheme, K):
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    from ldagroupedgibbssampler_amd.sampler import ADLDA, SimpleLDAConfiguration, create_model
    corpus = random_corpus(130, 300, 40, seed=31, empty_every=13)
    cfg = SimpleLDAConfiguration(scheme=scheme, topics=K, alpha=0.1, beta=0.01, seed=SEED, exec_time=None, iterations=2)
    m = ADLDA(cfg) if scheme == "adlda" else create_model(cfg)        # create_model does not know the name adlda
    m.setRandomSeed(SEED)
    m.addInstances(corpus)
    m.sample(2)
    assert (np.diff(corpus.doc_ptr) == 0).any()
    assert_bit_equal(m._h.theta_estimate(), m.getThetaEstimate(), "theta estimate")
    assert_bit_equal(m._h.zbar(), m.getZbar(), "z-bar")
    m.alpha[:] = np.random.default_rng(K).uniform(0.01, 2.0, K)     # a per-topic alpha
    m._h.set_hyperparameters(m.alpha, m.beta, m.betaSum)
    assert_bit_equal(m._h.theta_estimate(), m.getThetaEstimate(), "theta estimate after set_hyperparameters")
    assert_bit_equal(m._h.zbar(), m.getZbar(), "z-bar after set_hyperparameters")
    assert_bit_equal(m._h.theta_estimate(5, 40), m.getThetaEstimate()[5:40], "a range")
    m._h.close()


@pytest.mark.parametrize("name", ["ManhattanDistance", "KLDistance", "JensenShannonDistance", "StatisticalDistance"])
def test_document_distances_equal_the_restatement_on_z(native, cats, name):
    K = 5
    h = native.GGSHandle(K, cats.num_types, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS["spalias"])
    h.set_corpus(cats.doc_ptr, cats.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    h.sweep(3)
    query = MR.dirichlet_rows(10, K, 5)
    assert_same(h.document_distances(query, name), expected(name, cats, h.get_z(), K, 0.1, query), name)
    h.close()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def cats_halves():
    from ldagroupedgibbssampler_amd import frontend
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "datasets", "cats.txt")
    ds = frontend.load_dataset(path, stoplist=None)
    half = ds.corpus.num_docs // 2
    train, _, _ = ds.corpus.shard(0, half)
    test, _, _ = ds.corpus.shard(half, ds.corpus.num_docs)
    return train, test, ds.labels[:half].tolist(), ds.labels[half:].tolist()


def config(K=5):
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration
    return SimpleLDAConfiguration(scheme="spalias", topics=K, alpha=0.1, beta=0.01, seed=SEED, exec_time=None, iterations=20)


@pytest.mark.parametrize("name", ["ManhattanDistance", "KLDistance"])
def test_lda_distancer(native, name):
    from ldagroupedgibbssampler_amd.similarity import LDADistancer
    train, test, _, _ = cats_halves()
    d = LDADistancer(config())
    d.setDist(name)
    d.train(train)
    dist = d.distance(test, fold_in_sweeps=10)
    trained_z, folded_z = d.getTrainedSampler()._h.get_z(), d.folded._h.get_z()
    query = theta_rows(test, folded_z, 5, 0.1)
    assert_same(d.getSampledTestTopics(), query, "sampledTestTopics")
    want = expected(name, train, trained_z, 5, 0.1, query, np.diff(test.doc_ptr))
    assert_same(dist, want, "distance")
    idx, near = d.nearest(test, 3, fold_in_sweeps=10)                # the same seed: the same fold-in
    assert np.array_equal(d.folded._h.get_z(), folded_z)
    want_idx, want_near = R.nearest(want, 3)
    assert np.array_equal(idx, want_idx)
    assert_same(near, want_near, "nearest")


def test_kl_divergence_classifier(native):
    from ldagroupedgibbssampler_amd.similarity import KLDivergenceClassifier
    train, test, train_labels, _ = cats_halves()
    c = KLDivergenceClassifier(config())
    c.train(train, train_labels)
    names, cent = R.centroids(c.getTrainedSampler().getZbar(), train_labels, 0.1)     # the sampler's host z-bar
    assert names == c.classes == c.centroidClasses
    assert_same(c.classCentroids, cent, "centroids")
    scores, labels = c.classify(test, fold_in_sweeps=10)
    zbar = c.folded.getZbar()
    rows = np.stack([R.classifier_query_row(r, 0.1) for r in zbar])
    with np.errstate(all="ignore"):
        want = 1.0 / R.pairwise("KLDistance", cent, rows)
    assert_same(scores, want, "scores")
    assert labels == [names[R.first_maximum(r)] for r in want]
    # with the target alphabet the columns are its indices; a class without a training document keeps Java's 0.0
    alphabet = ["never seen"] + sorted(set(train_labels)) + ["nor this"]
    a = KLDivergenceClassifier(config())
    a.train(train, [alphabet.index(x) for x in train_labels], alphabet)
    assert a.classes == alphabet and a.centroidClasses == alphabet[1:-1]
    scores_a, labels_a = a.classify(test, fold_in_sweeps=10)                     # the same seed: the same chains
    cols = [alphabet.index(x) for x in names]
    assert_same(scores_a[:, cols], want, "scores by alphabet index")
    assert (scores_a[:, [0, len(alphabet) - 1]] == 0.0).all()
    padded = np.zeros_like(scores_a)
    padded[:, cols] = want
    assert labels_a == [alphabet[R.first_maximum(r)] for r in padded]


def run_dataset_example(tmp_path, *extra):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = os.path.join(root, "tests", "golden", "datasets")
    out = str(tmp_path / "run")
    cmd = [sys.executable, os.path.join(root, "examples", "run_dataset.py"), os.path.join(data, "cats.txt"), "--scheme", "spalias", "--topics", "5",
           "--iterations", "20", "--similarity", os.path.join(data, "SmallTexts.txt"), "--fold-in", "10", "--out", out] + list(extra)
    return subprocess.run(cmd, capture_output=True, text=True, timeout=120), out, data


def test_run_dataset_similarity_writes_the_nearest_documents(native, tmp_path):
    """the example end to end: the test file against the training alphabet, nearest_documents.csv in --out"""
    from ldagroupedgibbssampler_amd import frontend
    run, out, data = run_dataset_example(tmp_path, "--distance", "ManhattanDistance", "--nearest", "3")
    assert run.returncode == 0, run.stderr[-2000:]
    train = frontend.load_dataset(os.path.join(data, "cats.txt"), stoplist=None)
    test = frontend.load_dataset(os.path.join(data, "SmallTexts.txt"), stoplist=None, alphabet=tuple(train.corpus.vocab))
    assert test.corpus.num_types == train.corpus.num_types
    lines = [l.split(",") for l in open(os.path.join(out, "nearest_documents.csv")).read().splitlines()]
    assert lines and all(len(l) == 4 for l in lines)
    by_query = {}
    for q, rank, name, d in lines:
        assert name in train.names
        by_query.setdefault(q, []).append((int(rank), float(d)))
    lens = dict(zip(test.names, np.diff(test.corpus.doc_ptr)))
    assert set(by_query) <= set(test.names)
    for q, rows in by_query.items():
        assert [r for r, _ in rows] == list(range(len(rows))) and len(rows) <= 3
        assert all(a[1] <= b[1] for a, b in zip(rows, rows[1:])) and all(np.isfinite(d) for _, d in rows)
        assert lens[q] > 0 and len(rows) == 3                        # no training document of cats.txt is empty: a non-empty query finds three
    assert all(lens[q] == 0 for q in set(test.names) - set(by_query))   # an empty query has no finite distance and no line
    assert by_query and len(by_query) < len(test.names)              # SmallTexts.txt against this alphabet has both kinds


def test_run_dataset_similarity_refuses_a_scheme_without_phi(native, tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cats = os.path.join(root, "tests", "golden", "datasets", "cats.txt")
    run = subprocess.run([sys.executable, os.path.join(root, "examples", "run_dataset.py"), cats, "--scheme", "collapsed", "--similarity", cats,
                          "--out", str(tmp_path / "run")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 2 and "has none" in run.stderr


def test_two_shards_equal_one_handle(native):
    from ldagroupedgibbssampler_amd.sharded import NativeExchange, ShardedGGS
    K = 6
    whole, z = corpus_with_z(150, K, 10, empty=(3, 149), same=[(5, 120)])
    query = theta_rows(whole, z, K, 0.1)[[5, 80]] * (1 + 2.0 ** -40)
    qlen = np.array([4, 4], np.int64)
    side, sharded = Transport(2), {}

    def through(h, attach, rank):
        def exchange_factory(engine):
            attach(engine)
            return NativeExchange()
        sharded[rank] = ShardedGGS(h, exchange_factory, whole, rank, 2)

    def body(h, rank, sub, tok_base):
        sh = sharded[rank]
        sh.set_z_global(z)
        return {name: sh.nearest_documents(query, 7, name, qlen, gather=lambda a: side.exchange(rank, a)) for name in ("ManhattanDistance", "KLDistance")}

    out = run_ranks(2, whole, lambda rank: native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS["spalias"]), body, through=through)
    one = handle_of(native, whole, z, K)
    for name in ("ManhattanDistance", "KLDistance"):
        idx, dist = check_nearest(one, name, expected(name, whole, z, K, 0.1, query, qlen), query, 7, qlen)
        assert idx[0, :2].tolist() == [5, 120]
        for r in range(2):
            assert np.array_equal(out[r][name][0], idx) and np.array_equal(jbits(out[r][name][1]), jbits(dist)), (name, r)
    one.close()
