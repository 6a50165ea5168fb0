"""topics/TopicModelDiagnosticsPlain.java restated (tests/topic_diagnostics_restatement.py), without a GPU: the numpy form
against the literal transcription (Python sets for the TIntHashSets, a full IDSorter sort of all V words), a corpus worked by
hand, the exact bytes of the CSV writers, and the sampler's getter refusing n > V."""
import math
import os
import subprocess

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import formats as F
from tests import topic_diagnostics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compare(doc_ptr, tokens, z, counts, alpha, beta, n):
    V, K = counts.shape
    got = R.diagnostics(doc_ptr, tokens, z, counts, alpha, beta, n)
    lit = R.literal(doc_ptr, tokens, z, counts, alpha, beta, n)
    assert got["idx"].tolist() == lit["idx"]
    assert got["codoc"].tolist() == lit["codoc"]
    assert got["doc_stats"][:, 0].tolist() == lit["nonzero"] and got["doc_stats"][:, 1].tolist() == lit["rank1"]
    assert got["doc_stats"][:, 2:].tolist() == lit["at_prop"]
    assert R.same_doubles(got["clogc"], lit["clogc"])
    for i, name in enumerate(R.SCORE_ROWS):
        assert R.same_doubles(got["topic_scores"][i], lit["scores"][name][0]), (name, got["topic_scores"][i], lit["scores"][name][0])
    for i, name in enumerate(R.WORD_ROWS):
        assert R.same_doubles(got["word_scores"][i], lit["scores"][name][1]), (name, got["word_scores"][i], lit["scores"][name][1])
    return got


@pytest.mark.parametrize("D,V,K,n,seed", [(1, 1, 1, 1, 0), (3, 2, 2, 2, 1), (40, 30, 4, 5, 2), (25, 12, 7, 12, 3), (60, 9, 3, 4, 4)])
def test_numpy_form_equals_the_literal_transcription(D, V, K, n, seed):
    doc_ptr, tokens, z, counts = R.random_case(D, V, K, seed)
    for alpha, beta in ((0.1, 0.01), (np.linspace(0.05, 1.5, K), 0.5)):
        compare(doc_ptr, tokens, z, counts, alpha, beta, n)


def test_dense_columns_have_finite_distances():
    """every word under every topic: uniform_dist and corpus_dist are the in-order chains, ties (by falling id) included"""
    doc_ptr, tokens, z, counts = R.random_case(50, 6, 2, 7, mean_len=40)
    assert (counts > 0).all()
    got = compare(doc_ptr, tokens, z, counts, 0.1, 0.01, 3)
    assert np.isfinite(got["topic_scores"][3:5]).all()
    counts2 = counts.copy()
    counts2[2, 1] = 0                                              # one zero cell: NaN, eff_num_words as if the cell were skipped
    ts2 = R.scores(counts2, 0.01, 3, R.top_words(counts2, 3), got["codoc"], got["doc_stats"], got["clogc"])[0]
    assert np.isnan(ts2[3, 1]) and np.isnan(ts2[4, 1]) and np.isfinite(ts2[3, 0]) and np.isfinite(ts2[5, 1])


def test_edge_rows():
    doc_ptr, tokens, z, counts, V, K, n = R.edge_case()
    got = compare(doc_ptr, tokens, z, counts, 0.1, 0.01, n)
    assert got["idx"][:3].tolist() == [[0, 3, 2, 1], [0, 7, 3, 2], [7, 3, 2, 1]]
    assert (got["codoc"][0] >= 1).all() and got["codoc"][0][0, 0] == 2                          # document 0: the full block; word 0 thrice counts once
    assert got["doc_stats"][4].tolist() == [0] * 9 and not got["codoc"][4].any()                 # the topic without tokens
    assert np.isnan(got["topic_scores"][1, 4]) and np.isnan(got["topic_scores"][5, 4])
    assert (got["codoc"][3][2:] == 0).all() and (got["codoc"][3][:, 2:] == 0).all()             # zero-count words of a short list
    assert got["doc_stats"][:, 1].sum() == 6                                                     # every non-empty document has one rank-1 topic


@pytest.mark.parametrize("K,c,length,target", [(2, 1, 2, 0.5), (10, 1, 10, 0.1), (5, 1, 5, 0.2)])
def test_proportion_at_a_threshold_and_its_neighbours(K, c, length, target):
    cases = R.threshold_cases(K, c, length, target)
    assert set(cases) == {"at", "below", "above"}
    i = R.PROPORTIONS.tolist().index(target)
    for name, (alpha, doc_ptr, tokens, z) in cases.items():
        idx = np.zeros((K, 1), np.int32)
        _, st, _ = R.doc_statistics(doc_ptr, tokens, z, 2, K, alpha, 1, idx)
        assert st[0, 2:].tolist() == [1] * (i + (name != "below")) + [0] * (7 - i - (name != "below")), name
        counts = np.zeros((2, K), np.int32)
        np.add.at(counts, (tokens, z), 1)
        compare(doc_ptr, tokens, z, counts, alpha, 0.01, 1)


def test_worked_by_hand():
    """Three documents, two topics, V = 4, n = 2, alpha = 0.5 each (alphaSum = 1), beta = 1; tokens as (word, topic):
      d0: (0,0) (1,0) (0,0) (2,1)      d1: (0,0) (2,1) (3,1)      d2: (1,0) (1,1) (3,1)
    n_wk = [[3,0],[2,1],[0,2],[0,2]]: T_0 = [0, 1]; T_1 = [3, 2] (2 = 2: the higher id first; word 1's single token loses).
    Topic 0: d0 has words 0 and 1 under it (word 0 twice counts once) -> the whole block; d1 has word 0; d2 has word 1 (its second
    word 1 is under topic 1 and does not count): codoc_0 = [[2,1],[1,2]].  Topic 1: d0 has word 2 (position 1), d1 both, d2 word 3
    (position 0; word 1 is no top word): codoc_1 = [[2,1],[1,2]].  Coherence of both: log((1 + 1) / (2 + 1)) = log(2/3), the word
    scores 0.0 and log(2/3).
    c_dk = [[3,1],[1,2],[1,2]]: nonzero = [3,3]; rank1 = [1,2]; clogc = [3 log 3, 2 log 2 + 2 log 2].
    prop: d0 (3.5/5 = 0.7, 1.5/5 = 0.3: not < 0.3, < 0.5), d1 and d2 (1.5/4 = 0.375, 2.5/4 = 0.625):
    at_prop_0 = [3,3,3,3,3,3,1], at_prop_1 = [3,3,3,3,3,3,2].  rank_1_docs = [1/3, 2/3], allocation_ratio = [1/3, 2/3],
    allocation_count = [1, 1].  eff_num_words = [1 / (0.36 + 0.16), 1 / (0.16 + 0.16 + 0.04)].  Both columns have zero cells:
    uniform_dist and corpus_dist are NaN.  token-doc-diff of topic 0: p = [0.6, 0.4], q = [0.5, 0.5]."""
    docs = [[(0, 0), (1, 0), (0, 0), (2, 1)], [(0, 0), (2, 1), (3, 1)], [(1, 0), (1, 1), (3, 1)]]
    doc_ptr = np.array([0, 4, 7, 10], np.int64)
    tokens = np.array([w for d in docs for w, _ in d], np.int32)
    z = np.array([k for d in docs for _, k in d], np.int32)
    counts = np.zeros((4, 2), np.int32)
    np.add.at(counts, (tokens, z), 1)
    assert counts.tolist() == [[3, 0], [2, 1], [0, 2], [0, 2]]
    got = R.diagnostics(doc_ptr, tokens, z, counts, 0.5, 1.0, 2)
    assert got["idx"].tolist() == [[0, 1], [3, 2]]
    assert got["codoc"].tolist() == [[[2, 1], [1, 2]], [[2, 1], [1, 2]]]
    assert got["doc_stats"].tolist() == [[3, 1, 3, 3, 3, 3, 3, 3, 1], [3, 2, 3, 3, 3, 3, 3, 3, 2]]
    ln = math.log
    assert np.allclose(got["clogc"], [3 * ln(3), 4 * ln(2)], rtol=1e-15, atol=0)
    ts = dict(zip(R.SCORE_ROWS, got["topic_scores"]))
    ws = dict(zip(R.WORD_ROWS, got["word_scores"]))
    assert ts["tokens"].tolist() == [5.0, 5.0]
    assert np.allclose(ts["document_entropy"], [-3 * ln(3) / 5 + ln(5), -4 * ln(2) / 5 + ln(5)], rtol=1e-14, atol=0)
    assert np.allclose(ts["coherence"], [ln(2 / 3)] * 2, rtol=1e-15, atol=0)
    assert np.allclose(ws["coherence"], [[0.0, ln(2 / 3)]] * 2, rtol=1e-15, atol=0)
    assert np.isnan(ts["uniform_dist"]).all() and np.isnan(ts["corpus_dist"]).all()
    assert np.allclose(ts["eff_num_words"], [1 / 0.52, 1 / 0.36], rtol=1e-14, atol=0)
    diff0 = [0.5 * p * ln(p / m) + 0.5 * q * ln(q / m) for p, q, m in ((0.6, 0.5, 0.55), (0.4, 0.5, 0.45))]
    assert np.allclose(ws["token-doc-diff"][0], diff0, rtol=1e-12, atol=0) and np.allclose(ts["token-doc-diff"][0], sum(diff0), rtol=1e-12, atol=0)
    assert np.allclose(ts["rank_1_docs"], [1 / 3, 2 / 3]) and np.allclose(ts["allocation_ratio"], [1 / 3, 2 / 3])
    assert ts["allocation_count"].tolist() == [1.0, 1.0]
    # the word scores of the distances exist for a non-zero cell even where the topic score is NaN
    assert np.allclose(ws["uniform_dist"][0], [0.6 * ln(3 * 4 / 5), 0.4 * ln(2 * 4 / 5)], rtol=1e-14, atol=0)
    assert np.allclose(ws["corpus_dist"][0], [0.6 * ln(2.0 * 3 / 3), 0.4 * ln(2.0 * 2 / 3)], rtol=1e-14, atol=0)
    assert R.word_length(["ab", "c", "d\U0001F600", "efg"], got["idx"]).tolist() == [1.5, 3.0]     # the emoji is two UTF-16 code units


NAMES = ("tokens", "coherence", "eff_num_words")
COLUMNS = [[5.0, float("nan")], [-0.00004, float("inf")], [0.00005, -float("inf")]]
CSV = "Topic,tokens,coherence,eff_num_words\n0,5.0000,-0.0000,0.0001\n1,NaN,Infinity,-Infinity\n"


def test_csv_bytes(tmp_path):
    """NaN, the infinities, a negative value that rounds to zero keeps its sign, 0.00005 rounds HALF_UP"""
    assert F.format_topic_diagnostics_csv(NAMES, COLUMNS) == CSV
    assert F.format_topic_diagnostics_csv(("tokens",), [[]]) == "Topic,tokens\n"
    assert F.format_topic_diagnostics_csv(("tokens",), [[0.125, 0.00015]]) == "Topic,tokens\n0,0.1250\n1,0.0002\n"     # HALF_UP on the shortest digits
    fn = str(tmp_path / "diag.csv")
    F.write_topic_diagnostics(NAMES, COLUMNS, fn)
    assert open(fn, "rb").read() == (CSV + os.linesep).encode()


def test_cpp_writer_equals_the_python_one(tmp_path):
    exe = str(tmp_path / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "topic_diagnostics_formats_driver.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    cols = [list(c) for c in COLUMNS] + [rng.normal(0, 50, 2).tolist(), [0.12345, 1e9 + 0.00005]]
    names = list(NAMES) + ["token-doc-diff", "rank_1_docs"]
    py, cpp = str(tmp_path / "py.csv"), str(tmp_path / "cpp.csv")
    F.write_topic_diagnostics(names, cols, py)
    text = " ".join(names) + "\n" + "\n".join(" ".join(float(v).hex() if math.isfinite(v) else repr(float(v)) for v in c) for c in cols) + "\n"
    subprocess.run([exe, cpp], input=text, text=True, check=True)
    assert open(cpp, "rb").read() == open(py, "rb").read()


def test_names_are_the_csv_columns_of_the_java_class():
    from ldagroupedgibbssampler_amd import native
    assert native.TOPIC_DIAGNOSTIC_NAMES == R.NAMES and native.TOPIC_SCORE_ROWS == R.SCORE_ROWS and native.TOPIC_WORD_SCORE_ROWS == R.WORD_ROWS
    d = native.TopicDiagnostics(np.array([[1, 0]], np.int32), np.zeros((1, 2, 2), np.int32), np.zeros((1, 9), np.int32), np.zeros(1), np.arange(10.0)[:, None],
                                np.zeros((4, 1, 2)))
    assert d.names == R.SCORE_ROWS and d.topics_to_csv().startswith("Topic,tokens,document_entropy,coherence,")    # no alphabet: no word-length
    d = native.TopicDiagnostics(np.array([[1, 0]], np.int32), np.zeros((1, 2, 2), np.int32), np.zeros((1, 9), np.int32), np.zeros(1), np.arange(10.0)[:, None],
                                np.zeros((4, 1, 2)), ["abc", "d"])
    assert d.names == R.NAMES and d.scores["word-length"].tolist() == [2.0]
    assert d.topics_to_csv() == "Topic," + ",".join(R.NAMES) + "\n0,0.0000,1.0000,2.0000,2.0000,3.0000,4.0000,5.0000,6.0000,7.0000,8.0000,9.0000\n"


def test_abi_declares_the_entry_points():
    from ldagroupedgibbssampler_amd import _lib
    for name in ("ggs_topic_doc_statistics", "ggs_topic_scores", "ggs_debug_topic_doc_statistics", "ggs_debug_topic_scores"):
        assert name in _lib.SIGNATURES
        assert name in open(os.path.join(ROOT, "include", "ggs_hip.h")).read()


def test_configuration_keys():
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration
    cfg = SimpleLDAConfiguration()
    assert cfg.save_doc_topic_diagnostics is False and cfg.doc_topic_diagnostics_filename is None
    cfg = SimpleLDAConfiguration(save_doc_topic_diagnostics=True, doc_topic_diagnostics_filename="d.csv")
    assert cfg.save_doc_topic_diagnostics is True and cfg.doc_topic_diagnostics_filename == "d.csv"


def test_getter_refuses_more_words_than_types():
    """the Java reads word 0 for the positions beyond V; here the request is refused before anything is launched"""
    from ldagroupedgibbssampler_amd.sampler import LDAGroupedGibbsSampler, SimpleLDAConfiguration

    class Corpus:
        num_types, vocab = 3, ["a", "b", "c"]

    class Handle:
        def topic_diagnostics(self, n, alphabet):
            return ("called", n, alphabet)

    m = LDAGroupedGibbsSampler.__new__(LDAGroupedGibbsSampler)
    m.config, m._corpus, m._h = SimpleLDAConfiguration(nr_top_words=2), Corpus(), Handle()
    with pytest.raises(ValueError, match="more words"):
        m.getTopicModelDiagnostics(4)
    assert m.getTopicModelDiagnostics() == ("called", 2, ["a", "b", "c"])          # n defaults to nr_top_words
    m._h = None
    with pytest.raises(RuntimeError):
        m.getTopicModelDiagnostics(1)
