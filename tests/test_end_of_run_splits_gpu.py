"""The end-of-run kernels on their second piece, group, band and trip.

The min distances (csrc/ggs_distances.hpp), the top words and the topic diagnostics (csrc/ggs_topic_diagnostics.hpp) split
their work on the host side, in ggs_host_end_of_run.hpp: documents in pieces, topics in groups, tiles in bands, a foreign block in pieces,
and grids that are capped so that a workgroup loops.  The constants are sized for the benchmark corpus; at test shapes none of
these loops runs twice.  Here each of them does, either at a shape that reaches the built-in constant (the document pass on
8 492 documents, td_wtc_kernel on 16 389 words, td_mirror_kernel on 540 672 cells, two groups of topics at V = 70 000) or under
one of three knobs that can only make pieces smaller (GGS_DEBUG_TD_PIECE_BYTES, GGS_DEBUG_DIST_PIECE_BYTES,
GGS_DEBUG_DIST_BAND_TILES).  tests/end_of_run_splits.py holds the arithmetic and the inputs,
tests/test_end_of_run_splits_model.py proves without a device that every case reaches what it claims; every case here
asserts the same counts before it compares anything.

  loop of ggs_host_end_of_run.hpp                          its second round is reached by
  td_docs_kernel, grid min(nd, 4096)                    test_document_pass_second_and_third_trip
  TdDocPlan::piece                                      test_document_pieces_of_256, test_document_pieces_through_a_handle
  TdScorePlan::group, td_sorted_kernel with k0 > 0      test_topic_groups_of_g, test_topic_groups_through_a_handle,
                                                        test_two_built_in_groups_of_topics
  td_wtc_kernel, grid min(V, 8192)                      test_word_totals_third_trip
  td_mirror_kernel, grid_for's 2048 x 256 cells         test_mirror_second_trip
  dist_band_rows (both launchers)                       test_row_bands_against_itself, test_row_bands_against_a_foreign_block,
                                                        test_topic_bands
  ggs_min_doc_distances, pieces of the foreign block    test_foreign_block_in_pieces

Every comparison is bit for bit (integers equal, doubles by bit pattern, NaN as NaN), through the helpers of
tests/test_topic_diagnostics_gpu.py and tests/test_min_distances_gpu.py against the numpy restatements; every knobbed result
is also compared with the same call without the knob."""
import numpy as np
import pytest

from tests import end_of_run_splits as S
from tests import min_distances_restatement as MR
from tests import topic_diagnostics_restatement as R
from tests.test_min_distances_gpu import check as check_dist
from tests.test_min_distances_gpu import make as dist_handle
from tests.test_min_distances_gpu import synthetic
from tests.test_topic_diagnostics_gpu import check_docs, check_scores, handle_on, random_statistics

pytestmark = pytest.mark.gpu


def same_docs(a, b, tag):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and R.same_doubles(a[2], b[2]), tag


def same_scores(a, b, tag):
    assert R.same_doubles(a[0], b[0]) and R.same_doubles(a[1], b[1]), tag


# ---- the document pass: second and third trip (no knob) -----------------------------------------------------------------------
def test_document_pass_second_and_third_trip(native):
    """D = 2 x 4096 + 300, K = 130 (three rounds of topics, the third of 2), n = 128 (four mask words), non-uniform alpha: a
    workgroup of td_docs_kernel takes a long document, an empty one and a one-token one in turn (every other workgroup the
    other way round), clearing its histogram and masks as it reads them.  Workgroup 150's three documents are built by hand:
    every mask bit of topic 129 set on trip 1, one top word of that topic on trip 2, two on trip 3."""
    most, groups = S.trips(S.TRIP_D, S.DOCS_GRID)
    assert most == 3 and 0 < groups < S.DOCS_GRID and S.doc_pieces(S.TRIP_D, S.TRIP_K) == [S.TRIP_D]
    doc_ptr, tokens, z, counts, idx = S.trip_corpus()
    codoc, stats, _ = check_docs(native, doc_ptr, tokens, z, S.TRIP_V, S.TRIP_K, S.TRIP_ALPHA, S.TRIP_N, idx)
    want, (p1, p2, p3) = S.triple_codoc(idx)
    k = S.TRIP_TOPIC
    assert np.array_equal(codoc[k], want), np.argwhere(codoc[k] != want)[:5]
    assert codoc[k][p1, p1] == 2 and codoc[k][p2, p3] == 2 and codoc[k][0, 127] == 1
    assert stats[k, 0] == 3 and stats[k, 1] == 2                      # in three documents, rank 1 in the first and the third


# ---- pieces of documents ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [False, True], ids=["from zero", "from clogc_in"])
@pytest.mark.parametrize("K", S.PIECE_KS)
def test_document_pieces_of_256(native, monkeypatch, K, start):
    """GGS_DEBUG_TD_PIECE_BYTES = 12 K 256: rank1 / maxtopic by the piece's local document, the thresholds by doc_ptr[d0 + dl],
    the clogc chain across the pieces"""
    clogc_in = np.linspace(0.5, 40.0, K) if start else None
    for D in S.PIECE_DS:
        pieces = S.doc_pieces(D, K, S.piece_knob(K))
        assert pieces == S.cut(D, S.SEG) and S.doc_pieces(D, K) == [D]
        doc_ptr, tokens, z, counts = S.piece_case(D, K)
        idx = R.top_words(counts, S.PIECE_N)
        with S.knob(monkeypatch, S.KNOB_TD, S.piece_knob(K)):
            got = check_docs(native, doc_ptr, tokens, z, S.PIECE_V, K, np.linspace(0.05, 0.7, K), S.PIECE_N, idx, clogc_in, tag="%d pieces" % len(pieces))
        plain = native.debug_topic_doc_statistics(doc_ptr, tokens, z, S.PIECE_V, K, np.linspace(0.05, 0.7, K), S.PIECE_N, idx, clogc_in)
        same_docs(got, plain, ("knob against no knob", D, K))


def test_document_pieces_through_a_handle(native, monkeypatch):
    from ldagroupedgibbssampler_amd.corpus import Corpus
    D, K = 769, 65
    assert S.doc_pieces(D, K, S.piece_knob(K)) == [256, 256, 256, 1]
    doc_ptr, tokens, z, counts = S.piece_case(D, K)
    h = handle_on(native, Corpus(doc_ptr, tokens, S.PIECE_V), K, z)
    idx = R.top_words(counts, S.PIECE_N)
    start = np.linspace(0.5, 40.0, K)
    with S.knob(monkeypatch, S.KNOB_TD, S.piece_knob(K)):              # the knobbed call first: the scratch holds no earlier answer
        got = h.topic_doc_statistics(S.PIECE_N, idx, start)
        own = h.topic_doc_statistics(S.PIECE_N)                       # idx = None: the handle's own top words
    same_docs(got, h.topic_doc_statistics(S.PIECE_N, idx, start), "the handle: knob against no knob")
    same_docs(got, R.doc_statistics(doc_ptr, tokens, z, S.PIECE_V, K, np.full(K, 0.1), S.PIECE_N, idx, start), "the handle against the restatement")
    same_docs(own, R.doc_statistics(doc_ptr, tokens, z, S.PIECE_V, K, np.full(K, 0.1), S.PIECE_N, idx), "the handle's own top words")
    h.close()


# ---- groups of topics ---------------------------------------------------------------------------------------------------------
def assert_built_columns(ts, where, V):
    """rows 3, 4, 5: uniform_dist, corpus_dist, eff_num_words"""
    for kind, k in where.items():
        if kind == S.DENSE:
            assert np.isfinite(ts[3:6, k]).all(), (kind, k)
        if kind == S.HOLED:
            assert np.isnan(ts[3, k]) and np.isnan(ts[4, k]) and np.isfinite(ts[5, k]), (kind, k)
        if kind == S.EMPTY_COL:
            assert np.isnan(ts[3:6, k]).all() and ts[0, k] == 0.0, (kind, k)
        if kind == S.THIRD_DIGIT:
            assert np.isnan(ts[3, k]) and np.isfinite(ts[5, k]) and ts[0, k] > 65536 + 70000, (kind, k)


@pytest.mark.parametrize("V,g,K", S.GROUP_CASES)
def test_topic_groups_of_g(native, monkeypatch, V, g, K):
    """GGS_DEBUG_TD_PIECE_BYTES = 16 V g: td_sorted_kernel launched per group of g topics with k0 > 0, its sort buffers indexed by
    blockIdx.x and its outputs by k0 + blockIdx.x"""
    groups = S.topic_groups(V, K, S.group_knob(V, g))
    assert groups == S.cut(K, g) and S.topic_groups(V, K) == [K]
    counts, where = S.group_counts(V, g, K)
    assert S.columns_differ(counts) and (len(groups) == 1 or all(k >= g for k in where.values()))
    n = 20
    idx, stat = R.top_words(counts, n), random_statistics(K, n, V)
    with S.knob(monkeypatch, S.KNOB_TD, S.group_knob(V, g)):
        got = check_scores(native, counts, 0.01, n, idx, *stat, tag="groups %r" % (groups,))
    assert_built_columns(got[0], where, V)
    same_scores(got, native.debug_topic_scores(counts, 0.01, n, idx, *stat)[:2], "knob against no knob")


def test_topic_groups_through_a_handle(native, monkeypatch):
    from ldagroupedgibbssampler_amd.corpus import Corpus
    D, K, n = 257, 5, S.PIECE_N
    doc_ptr, tokens, z, counts = S.piece_case(D, K)
    assert S.topic_groups(S.PIECE_V, K, S.group_knob(S.PIECE_V, 2)) == [2, 2, 1]
    h = handle_on(native, Corpus(doc_ptr, tokens, S.PIECE_V), K, z)
    idx, stat = R.top_words(counts, n), random_statistics(K, n, 4)
    # the knobbed call first, on a fresh handle: a topic that a later launch failed to write must not find the answer of an
    # earlier call in the scratch
    with S.knob(monkeypatch, S.KNOB_TD, S.group_knob(S.PIECE_V, 2)):
        got = h.topic_scores(n, idx, *stat, word_scores=True)
    same_scores(got, R.scores(counts, 0.01, n, idx, *stat)[:2], "the handle against the restatement")
    same_scores(got, h.topic_scores(n, idx, *stat, word_scores=True), "the handle: knob against no knob")
    h.close()


def test_two_built_in_groups_of_topics(native):
    """no knob: V = 70 000 gives 64 MiB / (16 V) = 59 topics per launch, K = 61 a second launch of 2"""
    assert S.topic_groups(S.BIG_V, S.BIG_K) == [59, 2]
    counts = S.big_counts()
    n, K = S.BIG_N, S.BIG_K
    ts, _ = check_scores(native, counts, 0.01, n, R.top_words(counts, n), *random_statistics(K, n, 7))
    assert np.isfinite(ts[3:6, 0]).all() and np.isnan(ts[3, K - 1]) and np.isnan(ts[4, K - 1]) and np.isfinite(ts[5, K - 1])


# ---- td_wtc_kernel and td_mirror_kernel on their later trips (no knob) --------------------------------------------------------
@pytest.mark.parametrize("K", S.WTC_KS)
def test_word_totals_third_trip(native, K):
    """V = 2 x 8192 + 5: five workgroups of td_wtc_kernel take a third word; the dense column 0 reads wtc of every word in its
    corpus_dist chain"""
    assert S.trips(S.WTC_V, S.WTC_GRID) == (3, 5) and S.topic_groups(S.WTC_V, K) == [K]
    counts = S.sparse_tied_counts(S.WTC_V, K, 1)
    assert (counts[:, 0] > 0).all()
    n = 20
    ts, _ = check_scores(native, counts, 0.5, n, R.top_words(counts, n), *random_statistics(K, n, 8))
    assert np.isfinite(ts[3:6, 0]).all()


def test_mirror_second_trip(native):
    """K = 33, n = 128: 540 672 cells of codoc on td_mirror_kernel's 2048 x 256 threads"""
    assert S.mirror_trips(S.MIRROR_K, S.MIRROR_N) == (2, 16384)
    doc_ptr, tokens, z, counts = R.random_case(S.MIRROR_D, S.MIRROR_V, S.MIRROR_K, 3, mean_len=40)
    codoc, _, _ = check_docs(native, doc_ptr, tokens, z, S.MIRROR_V, S.MIRROR_K, 0.1, S.MIRROR_N, R.top_words(counts, S.MIRROR_N))
    assert np.array_equal(codoc, np.transpose(codoc, (0, 2, 1))) and codoc[S.MIRROR_K - 1].any() and np.triu(codoc[S.MIRROR_K - 1], 1).any()


# ---- bands of distance tiles --------------------------------------------------------------------------------------------------
def banded(native, monkeypatch, a, b, tile, element_major, diag_rows=True):
    n, m = len(a), len(a) if b is None else len(b)
    dev_in = np.ascontiguousarray(a.T) if element_major else a
    plain = native.debug_min_distances(dev_in, b, element_major=element_major)
    for v in S.band_knobs(m, tile):
        bands = S.dist_bands(n, m, tile, v)
        assert len(bands) >= 2 and S.dist_bands(n, m, tile) == [sum(bands)]
        if b is None:
            assert S.band_of(n - 1, n, m, tile, v) != S.band_of(S.NEAR, n, m, tile, v)
        with S.knob(monkeypatch, S.KNOB_DIST_BAND, v):
            dist, sq = check_dist(native, a, b, element_major=element_major, tag="bands %r" % (bands,))
        assert np.array_equal(MR.bits(dist), MR.bits(plain[0])) and np.array_equal(MR.bits(sq), MR.bits(plain[1])), ("knob against no knob", v)
        assert dist[S.TWIN] == 0.0 and sq[S.TWIN] == 0.0
        if b is None:
            d5 = MR.pair_sums(a[S.NEAR:S.NEAR + 1], a)[0]
            assert dist[n - 2] == 0.0 and dist[S.NEAR] == dist[n - 1] == np.sqrt(d5[n - 1]) and sq[n - 1] == np.delete(d5, S.NEAR).min()
        else:
            d5 = MR.pair_sums(a[S.NEAR:S.NEAR + 1], b)[0]
            assert int(np.argmin(d5)) == m - 1 and sq[S.NEAR] == d5[m - 1] and dist[n - 2] == 0.0


@pytest.mark.parametrize("n", S.BAND_ROW_SELF)
def test_row_bands_against_itself(native, monkeypatch, n):
    """one tile row per launch (the floor and the exact fit) and two with a ragged last band; the nearest partner of row 5 is
    the last row, identical rows lie in the first and the last but one tile row"""
    banded(native, monkeypatch, S.band_rows(n, S.BAND_ROW_LEN, 1), None, S.ROW_TILE, False)


def test_row_bands_against_a_foreign_block(native, monkeypatch):
    n, m = S.BAND_ROW_FOREIGN
    a = S.band_rows(n, S.BAND_ROW_LEN, 2)
    banded(native, monkeypatch, a, S.foreign_rows(a, m, 3), S.ROW_TILE, False)


@pytest.mark.parametrize("n,length", S.BAND_TOPIC)
def test_topic_bands(native, monkeypatch, n, length):
    banded(native, monkeypatch, S.band_rows(n, length, 4), None, S.TOPIC_TILE, True)


# ---- pieces of the foreign block, through a handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_foreign_block_in_pieces(native, monkeypatch, scheme):
    """GGS_DEBUG_DIST_PIECE_BYTES = 8 K r: the block travels r rows at a time, atomicMin merges across the pieces, and the stream
    is synchronised before a piece is overwritten.  One document's nearest partner is the last row of the last piece, another's
    the first row of the first; a row of the middle piece is NaN."""
    K = 7
    h = dist_handle(native, scheme, synthetic(), K)
    h.min_doc_distances()                                             # pcgs: the diagnostic theta of this iteration
    theta = h.get_theta()
    for r in S.FOREIGN_RS:
        for n_other in S.foreign_sizes(r):
            pieces = S.dist_pieces(n_other, K, S.foreign_knob(K, r))
            assert pieces == S.cut(n_other, min(r, n_other)) and S.dist_pieces(n_other, K) == [n_other]
            other = S.foreign_block(theta, n_other, r, r)
            want = MR.min_distances(theta, other)[0]
            sums = MR.pair_sums(theta[[S.LAST_DOC, S.FIRST_DOC]], other)
            assert int(np.nanargmin(sums[0])) == n_other - 1 and (n_other == 1 or int(np.nanargmin(sums[1])) == 0)
            if n_other == 2 * r + 1:
                assert len(pieces) == 3 and np.isnan(other[S.nan_row(n_other, r)]).all()
            with S.knob(monkeypatch, S.KNOB_DIST_PIECE, S.foreign_knob(K, r)):
                got = h.min_doc_distances(other)
            assert np.array_equal(MR.bits(got), MR.bits(want)), (scheme, r, n_other, pieces)
            assert np.array_equal(MR.bits(got), MR.bits(h.min_doc_distances(other))), ("knob against no knob", r, n_other)
            assert np.array_equal(MR.bits(h.get_theta()), MR.bits(theta))
    h.close()
