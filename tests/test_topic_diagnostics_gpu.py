"""The topic-diagnostics kernels (csrc/ggs_topic_diagnostics.hpp) against topics/TopicModelDiagnosticsPlain.java restated
(tests/topic_diagnostics_restatement.py): integers equal, doubles bit for bit, NaN as NaN.

The document pass takes a wave (64 lanes) per document and keeps 128-bit masks; the column statistics take SEG documents per
wave and 64 topics per workgroup; the sort takes 8-bit digits and 64 cells per step; a piece of documents holds at most
PIECE_BYTES / (12 K) documents: every list of shapes holds those edges -1, +0, +1."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import topic_diagnostics_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP, MAX_TOPICS, SEG, PIECE_BYTES = 128, 3072, 256, 64 << 20     # kTdMaxWords, kTdMaxTopics, kTdSegDocs, kTdPieceBytes
SEED, ZSEED = 17, 23


def check_docs(native, doc_ptr, tokens, z, V, K, alpha, n, idx, clogc_in=None, tag=""):
    got = native.debug_topic_doc_statistics(doc_ptr, tokens, z, V, K, alpha, n, idx, clogc_in)
    want = R.doc_statistics(doc_ptr, tokens, z, V, K, np.broadcast_to(np.asarray(alpha, np.float64), (K,)), n, idx, clogc_in)
    what = (tag, len(doc_ptr) - 1, V, K, n)
    bad = np.argwhere(got[0] != want[0])
    assert bad.size == 0, ("codoc differs in %d cells, first (k, i, j) %r: %d vs %d" % (len(bad), bad[0], got[0][tuple(bad[0])], want[0][tuple(bad[0])]),) + what
    assert np.array_equal(got[0], np.transpose(got[0], (0, 2, 1))), ("codoc is not symmetric",) + what
    assert np.array_equal(got[1], want[1]), ("doc_stats", got[1][(got[1] != want[1]).any(1)][:3], want[1][(got[1] != want[1]).any(1)][:3]) + what
    assert R.same_doubles(got[2], want[2]), ("clogc", got[2], want[2]) + what
    return got


def check_scores(native, counts, beta, n, idx, codoc, stats, clogc, tag=""):
    ts, ws, head = native.debug_topic_scores(counts, beta, n, idx, codoc, stats, clogc)
    wts, wws, whead = R.scores(counts, beta, n, idx, codoc, stats, clogc)
    what = (tag, counts.shape, beta, n)
    for i, name in enumerate(R.SCORE_ROWS):
        assert R.same_doubles(ts[i], wts[i]), (name, ts[i][:4], wts[i][:4]) + what
    for i, name in enumerate(R.WORD_ROWS):
        assert R.same_doubles(ws[i], wws[i]), (name,) + what
    assert np.array_equal(head, whead), ("sorted ids",) + what
    top = native.debug_topic_summaries(counts, beta, "top", n)["idx"]
    assert np.array_equal(np.where(head >= 0, top, -1), head), ("the first n sorted cells are not ggs_top_words' ids",) + what
    return ts, ws


def ns_of(V):
    return sorted({x for x in (1, 2, 20, 63, 64, 65, min(V, CAP)) if x <= V})


DS, VS, KS = [1, 2, 3, 65, 257], [1, 2, 64, 65, 300], [1, 2, 63, 64, 65, 130]


# ---- document statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", KS)
def test_document_statistics_shapes(native, K):
    """every D x V at this K; n walks through every value of {1, 2, 20, 63, 64, 65, min(V, 128)} that V allows"""
    turn = KS.index(K)
    for D in DS:
        for V in VS:
            ns = ns_of(V)
            n = ns[(turn + DS.index(D) + VS.index(V)) % len(ns)]
            doc_ptr, tokens, z, counts = R.random_case(D, V, K, 1, mean_len=30)
            alpha = 0.1 if (turn + D) % 2 else np.linspace(0.02, 0.9, K)
            check_docs(native, doc_ptr, tokens, z, V, K, alpha, n, R.top_words(counts, n))


@pytest.mark.parametrize("n", [1, 2, 20, 63, 64, 65, 128])
def test_every_list_length_with_all_document_lengths(native, n):
    """documents of 0, 1, 63, 64, 65 and 1 000 tokens in one corpus; short lists and lists of more than 64 and of 128 words"""
    lengths = [0, 1, 63, 64, 65, 1000, 0, 64, 1000, 2, 0]
    V, K = 300, 5
    doc_ptr, tokens, z, counts = R.random_case(len(lengths), V, K, n, lengths=lengths)
    check_docs(native, doc_ptr, tokens, z, V, K, np.array([0.1, 0.5, 0.02, 1.0, 0.3]), n, R.top_words(counts, n))


def test_built_rows(native):
    doc_ptr, tokens, z, counts, V, K, n = R.edge_case()
    idx = R.top_words(counts, n)
    codoc, stats, _ = check_docs(native, doc_ptr, tokens, z, V, K, 0.1, n, idx)
    assert (codoc[0] >= 1).all() and codoc[0][0, 0] == 2 and not codoc[4].any() and stats[4].tolist() == [0] * 9
    assert (codoc[3][2:] == 0).all() and stats[:, 1].tolist() == [5, 0, 1, 0, 0]
    check_docs(native, doc_ptr, tokens, z, V, K, np.array([0.3, 0.01, 2.0, 0.1, 0.7]), n, idx, tag="non-uniform alpha")


def test_rank_one_ties(native):
    """two topics tie, all topics tie, the tie sits beyond lane 63: the lowest topic wins"""
    K, V = 130, 3
    docs = [[5, 5, 9, 9], list(range(K)), [129, 70, 70, 129], [64, 0], [128, 65, 128, 65, 3]]
    doc_ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    z = np.array([k for d in docs for k in d], np.int32)
    tokens = (np.arange(len(z)) % V).astype(np.int32)
    _, stats, _ = check_docs(native, doc_ptr, tokens, z, V, K, 0.1, 1, np.zeros((K, 1), np.int32))
    assert stats[:, 1].nonzero()[0].tolist() == [0, 5, 65, 70] and stats[0, 1] == 2


@pytest.mark.parametrize("K,c,length,target", [(2, 1, 2, 0.5), (10, 1, 10, 0.1), (5, 1, 5, 0.2)])
def test_proportion_at_a_threshold_and_its_neighbours(native, K, c, length, target):
    cases = R.threshold_cases(K, c, length, target)
    assert set(cases) == {"at", "below", "above"}
    i = R.PROPORTIONS.tolist().index(target)
    for name, (alpha, doc_ptr, tokens, z) in cases.items():
        _, st, _ = check_docs(native, doc_ptr, tokens, z, 2, K, alpha, 1, np.zeros((K, 1), np.int32), tag=name)
        assert int(st[0, 2:].sum()) == i + (name != "below"), name


# ---- the clogc chain ----------------------------------------------------------------------------------------------------------
def growing_corpus(D=5000):
    """topic 0: counts growing from 1 to D / 10 over the documents (the running sum crosses some twenty binades); topic 1: one
    token in every document (every addend +0.0); topic 2: random"""
    rng = np.random.default_rng(3)
    c = np.stack([1 + np.arange(D) // 10, np.ones(D, np.int64), rng.integers(0, 6, D)], axis=1)
    lens = c.sum(1)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    z = np.repeat(np.tile(np.arange(3), D), c.reshape(-1)).astype(np.int32)
    tokens = rng.integers(0, 40, len(z)).astype(np.int32)
    return doc_ptr, tokens, z


def test_long_chain_across_binades_and_a_start_value(native):
    doc_ptr, tokens, z = growing_corpus()
    idx = np.tile(np.arange(5, dtype=np.int32), (3, 1))
    _, _, clogc = check_docs(native, doc_ptr, tokens, z, 40, 3, 0.1, 5, idx)
    first = 2 * np.log(2.0)
    assert clogc[1] == 0.0 and not np.signbit(clogc[1]) and np.log2(clogc[0] / first) >= 20
    start = np.array([0.1, 3.7, 1e-3])
    _, _, again = check_docs(native, doc_ptr, tokens, z, 40, 3, 0.1, 5, idx, clogc_in=start)
    assert again[1] == 3.7 and again[0] != clogc[0]


def test_second_piece_of_documents_at_the_largest_k(native):
    """K = 3072, the LDS limit: a piece holds 64 MiB / (12 K) documents rounded down to whole waves of 256; this corpus has more"""
    K, V, n = MAX_TOPICS, 50, 2
    piece = PIECE_BYTES // (12 * K) // SEG * SEG
    D = piece + SEG + 7
    doc_ptr, tokens, z, counts = R.random_case(D, V, K, 5, mean_len=4)
    check_docs(native, doc_ptr, tokens, z, V, K, 0.1, n, R.top_words(counts, n))
    with pytest.raises(native.GGSError) as e:
        native.debug_topic_doc_statistics(doc_ptr[:3], tokens[:doc_ptr[2]], z[:doc_ptr[2]], V, K + 1, 0.1, n, np.zeros((K + 1, n), np.int32))
    assert e.value.code == native.ERR_UNSUPPORTED


def handle_on(native, corpus, K, z, scheme="pcgs", alpha=0.1, beta=0.01):
    h = native.GGSHandle(K, corpus.num_types, alpha, beta, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.set_z(np.ascontiguousarray(z, np.int32), redraw_phi=True)
    return h


@pytest.mark.parametrize("cuts", [(37,), (1, 100), (64, 65)])
def test_handles_over_an_unevenly_split_corpus_chain_to_one(native, cuts):
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    c = random_corpus(130, 300, 40, seed=31, empty_every=13)
    K, n = 7, 6
    z = np.random.default_rng(2).integers(0, K, c.num_tokens).astype(np.int32)
    one = handle_on(native, c, K, z)
    idx = one.top_words("top", n)
    want = one.topic_doc_statistics(n)                                # idx=None: the handle's own top words
    assert np.array_equal(want[0], one.topic_doc_statistics(n, idx)[0])
    one.close()
    bounds = [0] + list(cuts) + [c.num_docs]
    codoc, stats, chain = 0, 0, None
    for a, b in zip(bounds[:-1], bounds[1:]):
        sub, _, tok_base = c.shard(a, b)
        h = handle_on(native, sub, K, z[tok_base:tok_base + sub.num_tokens])
        cd, st, chain = h.topic_doc_statistics(n, idx, chain)
        codoc, stats = codoc + cd.astype(np.int64), stats + st.astype(np.int64)
        h.close()
    assert np.array_equal(codoc, want[0]) and np.array_equal(stats, want[1]) and R.same_doubles(chain, want[2])


# ---- the sorted chains and the small scores -----------------------------------------------------------------------------------
def random_statistics(K, n, seed):
    rng = np.random.default_rng([K, n, seed])
    a = rng.integers(0, 6, (K, n, n))
    codoc = np.minimum(a, np.transpose(a, (0, 2, 1)))
    codoc[:, np.arange(n), np.arange(n)] += rng.integers(0, 9, (K, n))
    stats = np.sort(rng.integers(0, 50, (K, 9)), axis=1)[:, ::-1].copy()
    return codoc.astype(np.int32), stats.astype(np.int32), rng.random(K) * 100


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 5000])
def test_sorted_chains_shapes(native, V):
    """sparse counts with many ties (the ties' wtc differ: their order changes corpus_dist's bits where the column is dense)"""
    for K in (1, 64, 65, 100):
        rng = np.random.default_rng([V, K])
        counts = (rng.integers(0, 4, (V, K)) * (rng.random((V, K)) < 0.4)).astype(np.int32)
        counts[:, 0] = rng.integers(1, 4, V)                        # a column without zeros: finite distances
        if K > 1:
            counts[:, K - 1] = counts[:, 0]
            counts[V // 2, K - 1] = 0                               # the same column with exactly one zero cell
        n = min(V, 20)
        beta = (0.01, 0.5)[(K + V) % 2]
        ts, _ = check_scores(native, counts, beta, n, R.top_words(counts, n), *random_statistics(K, n, V))
        assert np.isfinite(ts[3:6, 0]).all()
        if K > 1:
            assert np.isnan(ts[3, K - 1]) and np.isnan(ts[4, K - 1]) and np.isfinite(ts[5, K - 1]) == (V > 1)      # V == 1: n_k == 0


def test_one_zero_cell_leaves_eff_num_words(native):
    V, K, n = 300, 3, 10
    rng = np.random.default_rng(8)
    counts = rng.integers(1, 50, (V, K)).astype(np.int32)
    stat = random_statistics(K, n, 1)
    full, _ = check_scores(native, counts, 0.01, n, R.top_words(counts, n), *stat)
    holed = counts.copy()
    w = int(np.argmin(counts[:, 1]))
    # the cell leaves n_k too: compare against the column where the cell's tokens never were
    holed[w, 1] = 0
    got, _ = check_scores(native, holed, 0.01, n, R.top_words(holed, n), *stat)
    assert np.isfinite(full[3:5]).all() and np.isnan(got[3:5, 1]).all() and np.isfinite(got[3:5, [0, 2]]).all()
    rest = np.delete(holed, w, axis=0)
    assert R.bits(got[5])[1] == R.bits(R.scores(rest, 0.01, n, R.top_words(rest, n), *stat)[0][5])[1]


def test_counts_at_the_digit_seams(native):
    V, K, n = 600, 4, 64
    rng = np.random.default_rng(9)
    counts = np.zeros((V, K), np.int32)
    seams = [254, 255, 256, 257, 65535, 65536, 65537, 1 << 24, (1 << 24) + 1, 1, 2]
    counts[:, 0] = rng.choice(seams, V)                              # dense, three digit passes and a fourth
    counts[:, 1] = rng.choice(seams[:4] + [0], V)                    # two passes
    counts[:, 2] = rng.choice([0, 1, 255], V)                        # one pass
    counts[:, 3] = rng.choice(seams[4:7], V)                         # dense, ties across the 16-bit seam
    check_scores(native, counts, 0.01, n, R.top_words(counts, n), *random_statistics(K, n, 2))
    check_scores(native, counts, 0.5, CAP, R.top_words(counts, CAP), *random_statistics(K, CAP, 3))


def test_empty_topic_and_empty_statistics(native):
    """n_k == 0 and nonzero == 0: the NaNs and infinities IEEE gives"""
    counts = np.array([[2, 0, 1], [0, 0, 1], [5, 0, 1]], np.int32)
    codoc, stats, clogc = np.zeros((3, 2, 2), np.int32), np.zeros((3, 9), np.int32), np.zeros(3)
    ts, _ = check_scores(native, counts, 0.01, 2, R.top_words(counts, 2), codoc, stats, clogc)
    assert np.isnan(ts[5, 1]) and np.isnan(ts[7]).all() and ts[0].tolist() == [7.0, 0.0, 3.0]


# ---- handles ------------------------------------------------------------------------------------------------------------------
def make(native, scheme, corpus, K, sweeps=3):
    h = native.GGSHandle(K, corpus.num_types, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    if sweeps:
        h.sweep(sweeps)
    return h


def same_as_restatement(d, want):
    assert np.array_equal(d.idx, want["idx"]) and np.array_equal(d.codoc, want["codoc"]) and np.array_equal(d.doc_stats, want["doc_stats"])
    assert R.same_doubles(d.clogc, want["clogc"])
    for i, name in enumerate(R.SCORE_ROWS):
        assert R.same_doubles(d.scores[name], want["topic_scores"][i]), name
    for i, name in enumerate(R.WORD_ROWS):
        assert R.same_doubles(d.word_scores[name], want["word_scores"][i]), name


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "collapsed", "adlda"])
def test_handle_answers_for_its_z_and_counts(native, cats, scheme):
    for K in (3, 20):
        h = make(native, scheme, cats, K)
        d = h.topic_diagnostics(8)
        same_as_restatement(d, R.diagnostics(cats.doc_ptr, cats.tokens, h.get_z(), h.get_type_topic_counts(), 0.1, 0.01, 8))
        assert d.names == R.SCORE_ROWS and np.array_equal(d.codocument_matrix(1), d.codoc[1])
        h.close()


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "collapsed", "adlda"])
def test_diagnostics_leave_the_chain_alone(native, cats, scheme):
    plain, probed = make(native, scheme, cats, 6, sweeps=1), make(native, scheme, cats, 6, sweeps=1)
    probed.topic_diagnostics(8)
    probed.topic_diagnostics_phases(8)
    plain.sweep(1)
    probed.sweep(1)
    for what in ("get_z", "get_type_topic_counts") + (("get_phi",) if scheme not in ("collapsed", "adlda") else ()):
        a, b = getattr(plain, what)(), getattr(probed, what)()
        assert np.array_equal(a.view(np.int64 if what == "get_phi" else np.int32), b.view(np.int64 if what == "get_phi" else np.int32)), what
    plain.close()
    probed.close()


def test_phase_times_of_a_call(native, cats):
    h = make(native, "ggs", cats, 5)
    ms = h.topic_diagnostics_phases(8)
    assert list(ms) == ["membership", "document_pass", "column_statistics", "clogc_chain", "totals", "sort_and_sorted_chains", "small_scores"]
    assert all(0.0 < v < 1000.0 for v in ms.values()), ms
    h.close()


def test_error_codes(native, cats):
    L, ip, dp = native._lib.load(), native._ip, native._dp
    K, V = 4, cats.num_types
    idx, codoc, stats, clogc = np.zeros((K, CAP + 1), np.int32), np.zeros((K, CAP + 1, CAP + 1), np.int32), np.zeros((K, 9), np.int32), np.zeros(K)
    ts = np.zeros((10, K))
    h = native.GGSHandle(K, V, 0.1, 0.01, SEED)
    assert L.ggs_topic_doc_statistics(h._h, 8, None, None, ip(codoc), ip(stats), dp(clogc)) == native.ERR_STATE
    assert L.ggs_topic_scores(h._h, 8, None, ip(codoc), ip(stats), dp(clogc), dp(ts), None) == native.ERR_STATE
    h.set_corpus(cats.doc_ptr, cats.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    assert L.ggs_topic_doc_statistics(h._h, 8, None, None, None, ip(stats), dp(clogc)) == native.ERR_BAD_ARG
    assert L.ggs_topic_doc_statistics(h._h, 8, None, None, ip(codoc), None, dp(clogc)) == native.ERR_BAD_ARG
    assert L.ggs_topic_doc_statistics(h._h, 8, None, None, ip(codoc), ip(stats), None) == native.ERR_BAD_ARG
    for n in (0, -1, V + 1):
        assert L.ggs_topic_doc_statistics(h._h, n, None, None, ip(codoc), ip(stats), dp(clogc)) == native.ERR_BAD_ARG
        assert L.ggs_topic_scores(h._h, n, None, ip(codoc), ip(stats), dp(clogc), dp(ts), None) == native.ERR_BAD_ARG
    if V > CAP:
        assert L.ggs_topic_doc_statistics(h._h, CAP + 1, None, None, ip(codoc), ip(stats), dp(clogc)) == native.ERR_UNSUPPORTED
        assert L.ggs_topic_scores(h._h, CAP + 1, None, ip(codoc), ip(stats), dp(clogc), dp(ts), None) == native.ERR_UNSUPPORTED
    bad = np.zeros((K, 8), np.int32)
    bad[1, 3] = V
    assert L.ggs_topic_doc_statistics(h._h, 8, ip(bad), None, ip(codoc), ip(stats), dp(clogc)) == native.ERR_BAD_ARG
    for args in ((None, ip(stats), dp(clogc), dp(ts)), (ip(codoc), None, dp(clogc), dp(ts)), (ip(codoc), ip(stats), None, dp(ts)), (ip(codoc), ip(stats), dp(clogc), None)):
        assert L.ggs_topic_scores(h._h, 8, None, *args, None) == native.ERR_BAD_ARG
    assert L.ggs_topic_doc_statistics(h._h, 8, None, None, ip(codoc), ip(stats), dp(clogc)) == 0
    assert L.ggs_topic_scores(h._h, 8, None, ip(codoc), ip(stats), dp(clogc), dp(ts), None) == 0
    with pytest.raises(native.GGSError) as e:
        h.topic_diagnostics(V + 1)
    assert e.value.code == native.ERR_BAD_ARG and "Asked for more words" in str(e.value)
    h.close()
    big = native.GGSHandle(MAX_TOPICS + 1, V, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS["pcgs"])
    big.set_corpus(cats.doc_ptr, cats.tokens)
    with pytest.raises(native.GGSError) as e:
        big.topic_doc_statistics(2, np.zeros((MAX_TOPICS + 1, 2), np.int32))
    assert e.value.code == native.ERR_UNSUPPORTED and "at most %d topics" % MAX_TOPICS in str(e.value)
    big.close()
    z = np.zeros(3, np.int32)
    with pytest.raises(native.GGSError) as e:                                                    # a z outside [0, K)
        native.debug_topic_doc_statistics(np.array([0, 3]), z, z + 2, 2, 2, 0.1, 1, np.zeros((2, 1), np.int32))
    assert e.value.code == native.ERR_BAD_ARG


# ---- the samplers, the sharded run and the example ----------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", ["ggs", "lightpclda", "spalias"])
def test_sampler_getter(native, scheme):
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    c = load_dataset(os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt"), stoplist=None).corpus
    cfg = SimpleLDAConfiguration(scheme=scheme, topics=6, alpha=0.1, beta=0.01, seed=SEED, exec_time=None, iterations=3, nr_top_words=7)
    m = create_model(cfg)
    m.setRandomSeed(SEED)
    m.addInstances(c)
    m.sample(3)
    d = m.getTopicModelDiagnostics()
    assert d.n == 7 and d.names == R.NAMES
    want = R.diagnostics(c.doc_ptr, c.tokens, m._h.get_z(), np.asarray(m.getTypeTopicMatrix()), 0.1, 0.01, 7)
    same_as_restatement(d, want)
    assert R.same_doubles(d.scores["word-length"], R.word_length(c.vocab, want["idx"]))
    assert d.topics_to_csv().splitlines()[0] == "Topic," + ",".join(R.NAMES) and len(d.topics_to_csv().splitlines()) == 7
    with pytest.raises(ValueError, match="more words"):
        m.getTopicModelDiagnostics(c.num_types + 1)


def test_three_sharded_ranks_equal_one(native):
    torch = pytest.importorskip("torch")
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    from ldagroupedgibbssampler_amd.sharded import ShardedGGS, java_lcg_initial_z, wrap_device_int32
    from tests.test_min_distances_gpu import _Lockstep
    c = random_corpus(130, 300, 40, seed=31, empty_every=13)
    K, n, world = 7, 9, 3
    z0 = java_lcg_initial_z(c.num_tokens, K, ZSEED)
    one = native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS["pcgs"])
    one.set_corpus(c.doc_ptr, c.tokens)
    one.set_z(z0, redraw_phi=False)
    one.init_phi()
    one.sweep(2)
    want = one.topic_diagnostics(n)
    one.close()
    ranks = [ShardedGGS(native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=native.SCHEME_FLAGS["pcgs"]), _Lockstep, c, r, world) for r in range(world)]

    def allreduce():
        counts = [wrap_device_int32(*s.engine.counts_device_ptr()) for s in ranks]
        tot = torch.stack(counts).sum(0, dtype=torch.int32)
        for t in counts:
            t.copy_(tot)
        torch.cuda.synchronize()

    for s in ranks:
        s.engine.set_z(z0[s.tok_base:s.tok_base + s.local.num_tokens], redraw_phi=False)
    allreduce()
    for s in ranks:
        s.engine.init_phi()
    for _ in range(2):
        for s in ranks:
            s.engine.sweep_begin()
        allreduce()
        for s in ranks:
            s.engine.sweep_end()
    # the call is collective: one thread per rank, `gather` meets at a barrier
    barrier, slots, got, errors = threading.Barrier(world, timeout=60), [None] * world, [None] * world, []

    def run(r):
        def gather(a):
            slots[r] = a
            barrier.wait()
            out = list(slots)
            barrier.wait()
            return out
        try:
            got[r] = ranks[r].topic_diagnostics(n, gather=gather)
        except Exception as e:                                        # noqa: BLE001
            errors.append(e)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    assert not errors, errors
    ref = dict(idx=want.idx, codoc=want.codoc, doc_stats=want.doc_stats, clogc=want.clogc,
               topic_scores=[want.scores[x] for x in R.SCORE_ROWS], word_scores=[want.word_scores[x] for x in R.WORD_ROWS])
    for d in got:
        same_as_restatement(d, ref)
    for s in ranks:
        s.engine.close()


def test_run_dataset_writes_the_diagnostics_file(tmp_path):
    from ldagroupedgibbssampler_amd import formats as F
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    out = tmp_path / "run"
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--topics", "5", "--iterations", "10", "--seed", "4711",
                        "--top-words", "6", "--topic-diagnostics", "diag.csv", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = (out / "diag.csv").read_bytes().decode()
    lines = text.split("\n")
    assert lines[0] == "Topic," + ",".join(R.NAMES) and len(lines) == 8 and lines[-2:] == ["", ""]       # topicsToCsv's last "\n" and println's
    # the same run in this process (the chain is deterministic): the file is the formatter's bytes on its scores
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    c = load_dataset(ds, stoplist=None, rare_threshold=0).corpus
    cfg = SimpleLDAConfiguration(scheme="ggs", topics=5, alpha=0.1, beta=0.01, iterations=10, seed=4711, exec_time=None, nr_top_words=6)
    m = create_model(cfg)
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(c)
    m.sample(10)
    d = m.getTopicModelDiagnostics(6)
    assert text == F.format_topic_diagnostics_csv(d.names, [d.scores[x] for x in d.names]) + os.linesep
    same_as_restatement(d, R.diagnostics(c.doc_ptr, c.tokens, m._h.get_z(), np.asarray(m.getTypeTopicMatrix()), 0.1, 0.01, 6))
    printed = [line for line in r.stdout.splitlines() if line.startswith("coherence: ")]
    assert len(printed) == 1 and printed[0].split()[1:] == ["%d:%s" % (k, F.java_format_fixed(v, 4)) for k, v in enumerate(d.scores["coherence"])]
