"""The topic-summary kernels (csrc/ggs_topic_summaries.hpp) against LDAUtils.java:566-911 restated
(tests/topic_summaries_restatement.py): the three normalisers and every score bit for bit, the ranking index for index.

The selection kernel takes SEG words per segment and BLOCK topics per workgroup; lists of up to LDS_WORDS words live in LDS,
longer ones (up to CAP) in global memory: every shape list holds the edges -1, +0, +1 and more than one segment / block."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import topic_summaries_restatement as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG, BLOCK, CAP, LDS_WORDS = 256, 64, 128, 64       # kTsSegWords, kTsTopics, kTsMaxWords, kTsLdsWords
BETAS, LAMBDAS = (0.01, 0.5), (0.0, 0.3, 0.6, 1.0)
SEED, ZSEED = 17, 23


def bits1(x):
    return int(np.float64(x).view(np.int64))


def check(native, counts, beta, kind, n, lam=0.6, tag="", want=None):
    """one debug call == the restatement: normalisers, all scores, the ranking, the returned scores"""
    got = native.debug_topic_summaries(counts, beta, kind, n, lam)
    mass, rowsum, total = R.normalisers(counts, beta)
    what = (tag, counts.shape, beta, kind, n, lam)
    assert np.array_equal(R.bits(got["mass_k"]), R.bits(mass)), ("mass_k",) + what
    assert np.array_equal(R.bits(got["rowsum_w"]), R.bits(rowsum)), ("rowsum_w",) + what
    assert bits1(got["total"]) == bits1(total), ("total", got["total"], total) + what
    a = R.scores(counts, beta, kind, lam) if want is None else want
    bad = np.argwhere(R.bits(got["all_scores"]) != R.bits(a))
    assert bad.size == 0, ("all_scores differ in %d cells, first %r: %r vs %r" % (len(bad), bad[0], got["all_scores"][tuple(bad[0])], a[tuple(bad[0])]),) + what
    idx = R.rank(a, n)
    bad = np.argwhere(got["idx"] != idx)
    assert bad.size == 0, ("idx differs in %d places, first (topic, rank) %r: %d vs %d" % (len(bad), bad[0], got["idx"][tuple(bad[0])], idx[tuple(bad[0])]),) + what
    assert np.array_equal(R.bits(got["score"]), R.bits(a[idx, np.arange(a.shape[1])[:, None]])), ("score",) + what
    return got


def ns_of(V):
    return sorted({1, min(20, V), min(V, CAP)})


VS = [1, 2, 63, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 1, 5000]
KS = [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 100, 130]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("V", VS)
def test_shapes(native, V, K):
    """every kind at every n of {1, 20, min(V, cap)}; beta and lambda rotate through their lists with the case, and the
    relevance ranking takes every lambda once more at n = min(20, V)"""
    counts = R.zipf_counts(V, K, 0)
    assert V < 64 or K < 8 or (counts == 0).mean() > 0.5             # sparse: most cells zero
    turn = VS.index(V) + KS.index(K)
    for i, kind in enumerate(R.KINDS):
        beta, lam = BETAS[(turn + i) % 2], LAMBDAS[(turn + i) % 4]
        want = R.scores(counts, beta, kind, lam)
        for n in ns_of(V):
            check(native, counts, beta, kind, n, lam, want=want)
    for lam in LAMBDAS:
        check(native, counts, BETAS[(turn + 1) % 2], "relevance", min(20, V), lam)


@pytest.mark.parametrize("n", [LDS_WORDS - 1, LDS_WORDS, LDS_WORDS + 1])
def test_list_moves_from_lds_to_global_memory(native, n):
    counts = R.zipf_counts(2 * SEG + 9, BLOCK + 3, 1)
    for kind in R.KINDS:
        check(native, counts, 0.01, kind, n)


# ---- ties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", R.KINDS)
def test_all_zero_matrix_lists_the_ids_downwards(native, kind):
    V, K = 2 * SEG + 5, 3
    for n in (1, 20, CAP):
        got = check(native, np.zeros((V, K), np.int32), 0.01, kind, n)
        assert got["idx"].tolist() == [list(range(V - 1, V - 1 - n, -1))] * K


@pytest.mark.parametrize("kind", R.KINDS)
def test_all_cells_equal(native, kind):
    V, K = SEG + 40, BLOCK + 1
    got = check(native, np.full((V, K), 3, np.int32), 0.5, kind, 20)
    assert got["idx"][0].tolist() == list(range(V - 1, V - 21, -1))


def test_topic_with_fewer_words_than_asked_for(native):
    V, K, n = 2 * SEG + 30, 4, 20
    counts = np.zeros((V, K), np.int32)
    counts[[5, SEG + 1, 2 * SEG + 7], 1] = [4, 9, 4]                 # topic 1: three words, two of them tied across segments
    counts[:, 2] = R.zipf_counts(V, 1, 3)[:, 0]
    got = check(native, counts, 0.01, "top", n)
    assert got["idx"][1].tolist() == [SEG + 1, 2 * SEG + 7, 5] + list(range(V - 1, V - 18, -1))
    for kind in R.KINDS[1:]:
        check(native, counts, 0.01, kind, n)


def test_same_best_weight_in_two_segments(native):
    V, K = 3 * SEG, 2
    counts = R.zipf_counts(V, K, 4)
    top = int(counts.max()) + 7
    counts[10, 0] = counts[2 * SEG + 10, 0] = top
    got = check(native, counts, 0.01, "top", 5)
    assert got["idx"][0, :2].tolist() == [2 * SEG + 10, 10]          # the higher id first


@pytest.mark.parametrize("kind", R.KINDS)
def test_identical_rows_tie_in_every_kind(native, kind):
    V, K = SEG + 70, 5
    counts = R.zipf_counts(V, K, 5, density=0.5)
    counts[SEG + 3] = counts[17] = counts.max(axis=0) + 1              # the two best words of every topic, in two segments
    got = check(native, counts, 0.01, kind, 20)
    assert np.array_equal(R.bits(got["all_scores"][17]), R.bits(got["all_scores"][SEG + 3]))
    if kind == "top":
        assert got["idx"][:, :2].tolist() == [[SEG + 3, 17]] * K
    for row in got["idx"].tolist():                                   # wherever the pair ranks: side by side, the higher id first
        if SEG + 3 in row[:-1]:
            assert row[row.index(SEG + 3) + 1] == 17


# ---- positions -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["last ragged segment", "first segment", "one per segment"])
def test_where_the_winners_sit(native, where):
    n, K = 20, 3
    V = (n - 1) * SEG + 37 if where == "one per segment" else 3 * SEG + 37
    counts = (R.zipf_counts(V, K, 6) > 0).astype(np.int32)
    rng = np.random.default_rng(7)
    for k in range(K):
        if where == "last ragged segment":
            ids = 3 * SEG + rng.permutation(37)[:n]
        elif where == "first segment":
            ids = rng.permutation(SEG)[:n]
        else:
            ids = np.arange(n) * SEG + rng.integers(0, 37, n)
        counts[ids, k] = 100 + rng.permutation(n)
    got = check(native, counts, 0.01, "top", n)
    seg = got["idx"] // SEG
    if where == "one per segment":
        assert all(sorted(row) == list(range(n)) for row in seg.tolist())
    else:
        assert (seg == (3 if where.startswith("last") else 0)).all()
    for kind in R.KINDS[1:]:
        check(native, counts, 0.5, kind, n)


# ---- chains ----------------------------------------------------------------------------------------------------------------
def test_addends_on_half_ulp_ties(native):
    """beta = 2^-30 under running sums in [2^23, 2^24): their ulp is 2^-29, so every later addend 0 + beta is a half-ulp tie
    of mass_0, rowsum_0 and total, which round to even and stay where they are; a second case ends the regime half-way"""
    V, K, beta = 300, 5, 2.0 ** -30
    for big_rows in (1, 2):
        counts = np.zeros((V, K), np.int32)
        counts[0, 0] = 2 ** 23
        if big_rows == 2:
            counts[150, :] = 2 ** 23                                 # the sums leave the binade here
        counts[2::7, 1] = 1
        mass, rowsum, total = R.normalisers(counts, beta)
        if big_rows == 1:
            assert mass[0] == 2.0 ** 23 and rowsum[0] == 2.0 ** 23 and total == 2.0 ** 23 + counts[:, 1].sum()    # every beta was rounded away
        for kind in R.KINDS:
            check(native, counts, beta, kind, 20)


@pytest.mark.parametrize("beta", [0.5, 0.25, 2.0])
def test_dyadic_beta_sums_are_exact(native, beta):
    counts = R.zipf_counts(SEG + 9, BLOCK + 2, 8)
    got = check(native, counts, beta, "relevance", 20)
    assert got["total"] == float(counts.sum(dtype=np.int64)) + beta * counts.size
    for kind in ("distinctive", "salient", "k1"):
        check(native, counts, beta, kind, 20)


def test_long_total_chain_across_twenty_binades(native):
    V, K, beta = 5000, 100, 0.01
    counts = R.zipf_counts(V, K, 9, density=0.3)
    counts[V - 40:, :] += 200
    _, _, total = R.normalisers(counts, beta)
    assert V * K >= 500000 and np.log2(total) - np.log2(beta) >= 20
    check(native, counts, beta, "relevance", 20)
    check(native, counts, beta, "salient", 20)


def test_element_by_element_sums_agree(native, monkeypatch):
    """GGS_DEBUG_CHAIN=1: both column sums walked one element at a time"""
    monkeypatch.setenv("GGS_DEBUG_CHAIN", "1")
    check(native, R.zipf_counts(SEG + 9, 11, 10), 0.01, "distinctive", 20)


# ---- handle level ----------------------------------------------------------------------------------------------------------
def synthetic():
    return random_corpus(130, 300, 40, seed=31, empty_every=13)


def make(native, scheme, corpus, K, sweeps=2, beta=0.01):
    h = native.GGSHandle(K, corpus.num_types, 0.1, beta, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    if sweeps:
        h.sweep(sweeps)
    return h


def check_handle(h, beta, n=20, lam=0.3):
    counts = h.get_type_topic_counts()
    for kind in R.KINDS:
        idx, sc, _ = R.top_words(counts, beta, kind, n, lam)
        got_idx, got_sc = h.top_words(kind, n, lam, scores=True)
        assert np.array_equal(got_idx, idx), kind
        assert np.array_equal(R.bits(got_sc), R.bits(sc)), kind
        assert np.array_equal(h.top_words(kind, n, lam), idx), kind


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "collapsed", "adlda"])
def test_handle_answers_for_its_counts(native, cats, scheme):
    for corpus, K in ((cats, 20), (synthetic(), 7)):
        h = make(native, scheme, corpus, K, sweeps=3)
        check_handle(h, 0.01)
        h.close()


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "collapsed"])
def test_summaries_leave_the_chain_alone(native, scheme):
    c = synthetic()
    plain, probed = make(native, scheme, c, 7, sweeps=0), make(native, scheme, c, 7, sweeps=0)
    for _ in range(3):
        for kind in R.KINDS:
            probed.top_words(kind, 20)
        plain.sweep(1)
        probed.sweep(1)
    for what in ("get_z", "get_type_topic_counts") + (("get_phi",) if scheme != "collapsed" else ()):
        a, b = getattr(plain, what)(), getattr(probed, what)()
        assert np.array_equal(a.view(np.int64 if what == "get_phi" else np.int32), b.view(np.int64 if what == "get_phi" else np.int32)), what
    plain.close()
    probed.close()


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_two_exchanging_handles_equal_one(native, scheme):
    from ldagroupedgibbssampler_amd.sharded import even_split, java_lcg_initial_z
    from tests.test_native_exchange_gpu import OneThreadTransport
    c = random_corpus(170, 300, 70, seed=12, empty_every=7)
    K, n = 13, 2
    z0 = java_lcg_initial_z(c.num_tokens, K, 5)
    one = native.GGSHandle(K, c.num_types, 0.1, 0.01, 606, flags=native.SCHEME_FLAGS[scheme])
    one.set_corpus(c.doc_ptr, c.tokens)
    one.set_z(z0, redraw_phi=True)
    one.sweep(3)
    want = {kind: one.top_words(kind, 20, 0.6, scores=True) for kind in R.KINDS}
    one.close()
    tr = OneThreadTransport(n)
    bounds = even_split(c.num_docs, n)
    hs, zs = [], []
    for r in range(n):
        h = native.GGSHandle(K, c.num_types, 0.1, 0.01, 606, flags=native.SCHEME_FLAGS[scheme])
        h.attach_exchange(r, n, *tr.callbacks(r))
        sub, doc_base, tok_base = c.shard(bounds[r], bounds[r + 1])
        h.set_corpus(sub.doc_ptr, sub.tokens, doc_base, tok_base)
        h.set_global_token_count(c.num_tokens)
        zs.append(z0[tok_base:tok_base + sub.num_tokens])
        hs.append(h)
    g = native.GGSGroup.adopt(hs)
    g.set_z(zs, redraw_phi=True)
    g.sweep(3)
    g.gather_counts()                                                 # the collective part, for both handles at once
    for h in hs:
        for kind in R.KINDS:
            idx, sc = h.top_words(kind, 20, 0.6, scores=True)
            assert np.array_equal(idx, want[kind][0]) and np.array_equal(R.bits(sc), R.bits(want[kind][1])), kind
    g.close()
    for h in hs:
        h.close()


def test_phase_times_of_a_call(native):
    """ggs_debug_top_words_phases: what scripts/time_topic_summaries.py reports; the call changes nothing a later one reads"""
    h = make(native, "pcgs", synthetic(), 7)
    before = h.top_words("relevance", 20, scores=True)
    for chain in (False, True):
        ms = h.top_words_phases("relevance", 20, element_chain=chain)
        assert list(ms) == ["mass_k", "total", "words", "select_merge"] and all(0.0 < v < 1000.0 for v in ms.values())
    after = h.top_words("relevance", 20, scores=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(R.bits(before[1]), R.bits(after[1]))
    assert h.top_words_phases("top", 20)["select_merge"] > 0.0
    L = native._lib.load()
    assert L.ggs_debug_top_words_phases(h._h, 1, 20, 0.6, 0, None) == native.ERR_BAD_ARG
    h.close()


def test_error_codes(native):
    c = synthetic()
    V = c.num_types
    L, ip, dp = native._lib.load(), native._ip, native._dp
    idx, sc = np.zeros((5, CAP + 1), np.int32), np.zeros((5, CAP + 1), np.float64)
    h = native.GGSHandle(5, V, 0.1, 0.01, SEED)
    assert L.ggs_top_words(h._h, 0, 20, 0.6, ip(idx), None) == native.ERR_STATE                 # no corpus
    h.set_corpus(c.doc_ptr, c.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    assert L.ggs_top_words(h._h, 0, 20, 0.6, None, None) == native.ERR_BAD_ARG
    assert L.ggs_top_words(h._h, 0, 0, 0.6, ip(idx), None) == native.ERR_BAD_ARG
    assert L.ggs_top_words(h._h, 0, V + 1, 0.6, ip(idx), None) == native.ERR_BAD_ARG
    assert L.ggs_top_words(h._h, 5, 20, 0.6, ip(idx), None) == native.ERR_BAD_ARG
    assert L.ggs_top_words(h._h, -1, 20, 0.6, ip(idx), None) == native.ERR_BAD_ARG
    for lam in (np.nan, np.inf, -np.inf):
        assert L.ggs_top_words(h._h, 1, 20, lam, ip(idx), None) == native.ERR_BAD_ARG
    assert L.ggs_top_words(h._h, 1, CAP + 1, 0.6, ip(idx), None) == native.ERR_UNSUPPORTED
    assert L.ggs_top_words(h._h, 1, CAP, 0.6, ip(idx), dp(sc)) == 0
    with pytest.raises(native.GGSError) as e:
        h.top_words("top", V + 1)
    assert e.value.code == native.ERR_BAD_ARG and "Asked for more words (%d) than there are types" % (V + 1) in str(e.value)
    with pytest.raises(ValueError):
        h.top_words("best", 3)
    h.close()
    counts = np.ones((10, 3), np.int32)
    for kind in R.KINDS[1:]:                                                                   # beta == 0: NaN scores
        with pytest.raises(native.GGSError) as e:
            native.debug_topic_summaries(counts, 0.0, kind, 3)
        assert e.value.code == native.ERR_BAD_ARG
    assert native.debug_topic_summaries(counts, 0.0, "top", 3)["idx"].tolist() == [[9, 8, 7]] * 3
    with pytest.raises(native.GGSError) as e:
        native.debug_topic_summaries(counts, 0.01, "top", 11)
    assert e.value.code == native.ERR_BAD_ARG
    assert L.ggs_debug_topic_summaries(0, 10, 3, None, 0.01, 0.6, 0, 3, ip(idx), None, None, None, None, None) == native.ERR_BAD_ARG


# ---- the samplers and the example ------------------------------------------------------------------------------------------
def test_sampler_methods(native, cats):
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    ds = load_dataset(os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt"), stoplist=None)
    c = ds.corpus
    cfg = SimpleLDAConfiguration(scheme="pcgs", topics=6, alpha=0.1, beta=0.01, seed=SEED, exec_time=None, iterations=3, **{"lambda": 0.3})
    m = create_model(cfg)
    m.setRandomSeed(SEED)
    m.addInstances(c)
    m.sample(3)
    counts = np.asarray(m.getTypeTopicMatrix())
    n = cfg.nr_top_words
    words = lambda idx: [[c.vocab[i] for i in row] for row in idx.tolist()]      # noqa: E731
    assert np.array_equal(m.getTopWordIndices(n), R.top_words(counts, 0.01, "top", n)[0])
    assert m.getTopWords(n) == words(R.top_words(counts, 0.01, "top", n)[0])
    assert m.getTopRelevanceWords(n) == words(R.top_words(counts, 0.01, "relevance", n, 0.3)[0])       # the configuration's lambda
    assert m.getTopRelevanceWords(n, 1.0) == words(R.top_words(counts, 0.01, "relevance", n, 1.0)[0])
    assert m.getTopDistinctiveWords(n) == words(R.top_words(counts, 0.01, "distinctive", n)[0])
    assert m.getTopSalientWords(n) == words(R.top_words(counts, 0.01, "salient", n)[0])
    assert m.getK1ReWeightedWords(n) == words(R.top_words(counts, 0.01, "k1", n)[0])
    with pytest.raises(ValueError, match=r"Asked for more words \(%d\) than there are types \(unique words = noTypes = %d\)\." % (c.num_types + 1, c.num_types)):
        m.getTopWords(c.num_types + 1)


def test_run_dataset_writes_top_and_relevance_words(tmp_path):
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    out = tmp_path / "run"
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--topics", "20", "--iterations", "10", "--seed", "4711",
                        "--top-words", "12", "--lambda", "0.3", "--out", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.count("topic ") == 20
    vocab = load_dataset(ds, stoplist=None).corpus.vocab
    counts = np.loadtxt(out / "type_topic_counts.csv", delimiter=",", dtype=np.int64).T            # the file is [K][V]
    for name, kind in (("TopWords.txt", "top"), ("RelevanceWords.txt", "relevance")):
        text = (out / name).read_text()
        assert text.endswith("\n") and not text.endswith("\n\n")
        rows = [line.split(",") for line in text.splitlines()]
        assert len(rows) == 20 and all(len(row) == 12 and set(row) <= set(vocab) for row in rows)
        want = R.top_words(counts, 0.01, kind, 12, 0.3)[0]
        assert rows == [[vocab[i] for i in row] for row in want.tolist()], name
    printed = [line.split(": ", 1)[1].split() for line in r.stdout.splitlines() if line.startswith("topic ")]
    assert printed == [line.split(",") for line in (out / "TopWords.txt").read_text().splitlines()]
