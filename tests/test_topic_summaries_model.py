"""The topic summaries of LDAUtils.java:566-911 restated (tests/topic_summaries_restatement.py), without a GPU: the numpy form
against a literal transcription that sorts IDSorter objects with MALLET's comparator, the tie rule against
frontend.tfidf_ranks, a V = 3, K = 2 case worked by hand for each kind, and the exact bytes of the CSV writers."""
import math
import os
import subprocess

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import formats as F
from ldagroupedgibbssampler_amd.frontend import tfidf_ranks
from tests import topic_summaries_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tied_counts(V, K, seed):
    """few distinct values, whole rows repeated: ties in every kind"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 3, (V, K)).astype(np.int32)
    c[V // 2] = c[0]
    c[V - 1] = c[1]
    return c


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("make", [lambda: R.zipf_counts(37, 5, 2, density=0.4), lambda: tied_counts(23, 4, 3), lambda: np.zeros((9, 3), np.int32),
                                  lambda: np.full((7, 2), 4, np.int32)], ids=["random", "tied", "zero", "equal"])
def test_numpy_form_equals_the_literal_transcription(kind, make):
    c = make()
    for beta, lam in ((0.01, 0.6), (0.5, 0.0), (0.5, 1.0)):
        idx, _, a = R.top_words(c, beta, kind, c.shape[0], lam)
        lit_idx, lit_a = R.literal(c, beta, kind, c.shape[0], lam)
        assert np.array_equal(R.bits(np.array(lit_a) + 0.0), R.bits(a + 0.0)), (kind, beta, lam)
        assert idx.tolist() == lit_idx, (kind, beta, lam)


def test_tie_rule_is_that_of_tfidf_ranks():
    tf, df = [0, 3, 0, 3, 1, 0], [1, 2, 1, 2, 1, 1]
    ranks, w = tfidf_ranks(tf, df, 4)
    assert R.rank(np.array(w)[:, None], len(w))[0].tolist() == ranks
    assert R.rank(np.zeros((5, 1)), 5)[0].tolist() == [4, 3, 2, 1, 0]
    assert R.rank(np.array([[0.0], [-0.0], [0.0]]), 3)[0].tolist() == [2, 1, 0]      # the zeros are equal


def test_worked_by_hand():
    """V = 3, K = 2, beta = 0.5 (every sum below is exact): counts rows [2, 0], [0, 1], [1, 1]."""
    c = np.array([[2, 0], [0, 1], [1, 1]], np.int32)
    beta, lam = 0.5, 0.25
    mass, rowsum, total = R.normalisers(c, beta)
    assert mass.tolist() == [4.5, 3.5] and rowsum.tolist() == [3.0, 2.0, 3.0] and total == 8.0
    assert R.rank(R.scores(c, beta, "top"), 3).tolist() == [[0, 2, 1], [2, 1, 0]]      # topic 1: the two 1s by falling id
    ln = math.log
    p_wk = [[2.5 / 4.5, 0.5 / 3.5], [0.5 / 4.5, 1.5 / 3.5], [1.5 / 4.5, 1.5 / 3.5]]
    p_w = [3.0 / 8.0, 2.0 / 8.0, 3.0 / 8.0]
    rel = [[lam * ln(p_wk[w][k]) + (1 - lam) * (ln(p_wk[w][k]) - ln(p_w[w])) for k in range(2)] for w in range(3)]
    assert np.allclose(R.scores(c, beta, "relevance", lam, log=np.log), rel, rtol=1e-14, atol=0)
    assert R.rank(R.scores(c, beta, "relevance", lam), 3).tolist() == [[0, 2, 1], [1, 2, 0]]
    P = [[p_wk[w][k] * ([4.5, 3.5][k] / 8.0) / p_w[w] for k in range(2)] for w in range(3)]
    dist = [[P[w][k] * ln(P[w][k] / p_w[w]) for k in range(2)] for w in range(3)]
    assert np.allclose(R.scores(c, beta, "distinctive", log=np.log), dist, rtol=1e-13, atol=0)
    assert np.allclose(R.scores(c, beta, "salient", log=np.log), [[p_w[w] * dist[w][k] for k in range(2)] for w in range(3)], rtol=1e-13, atol=0)
    assert np.allclose([sum(r) for r in P], 1.0)                                        # P is p(topic | word)
    assert R.rank(R.scores(c, beta, "distinctive"), 3).tolist() == [[0, 2, 1], [1, 2, 0]]
    assert R.rank(R.scores(c, beta, "salient"), 3).tolist() == [[0, 2, 1], [1, 2, 0]]
    k1 = [[p_wk[w][k] / (p_wk[w][0] + p_wk[w][1]) for k in range(2)] for w in range(3)]
    assert np.allclose(R.scores(c, beta, "k1"), k1, rtol=1e-15, atol=0)
    assert R.rank(R.scores(c, beta, "k1"), 3).tolist() == [[0, 2, 1], [1, 2, 0]]


def test_negative_zero_distinctiveness_becomes_positive_zero():
    """wordDistinctiveness[w][k] += x onto 0.0: a -0.0 product is stored as +0.0"""
    a = 0.0 + np.array([-0.0])
    assert np.signbit(a).tolist() == [False]


ROWS = [["cat", "dog", "fish"], ["a"], ["x", "y"]]


def test_csv_bytes(tmp_path):
    assert F.format_top_words_csv(ROWS) == "cat,dog,fish\na\nx,y"
    assert F.format_top_words_csv([]) == "" and F.format_top_words_csv([["one"]]) == "one"
    fn = str(tmp_path / "TopWords.txt")
    F.write_top_words(ROWS, fn)
    assert open(fn, "rb").read() == ("cat,dog,fish\na\nx,y" + os.linesep).encode()


def test_cpp_writer_equals_the_python_one(tmp_path):
    exe = str(tmp_path / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "topic_summaries_formats_driver.cpp"), "-o", exe])
    rng = np.random.default_rng(5)
    rows = ROWS + [["w%d" % i for i in rng.integers(0, 1000, 20)] for _ in range(6)]
    py, cpp = str(tmp_path / "py.txt"), str(tmp_path / "cpp.txt")
    F.write_top_words(rows, py)
    subprocess.run([exe, cpp], input="\n".join(" ".join(r) for r in rows) + "\n", text=True, check=True)
    assert open(cpp, "rb").read() == open(py, "rb").read()


def test_configuration_keys():
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration
    cfg = SimpleLDAConfiguration()
    assert cfg.nr_top_words == 20 and cfg.lambda_ == 0.6                                # LDAConfiguration.java:38,41
    cfg = SimpleLDAConfiguration(nr_top_words=7, **{"lambda": 0.25})
    assert cfg.nr_top_words == 7 and cfg.lambda_ == 0.25


def test_abi_declares_the_entry_points():
    from ldagroupedgibbssampler_amd import _lib
    assert "ggs_top_words" in _lib.SIGNATURES and "ggs_debug_topic_summaries" in _lib.SIGNATURES
