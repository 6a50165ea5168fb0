"""scheme=spalias_priors without a device: the priors file parser (ldagroupedgibbssampler_amd/priors.py) on the reference's three
fixtures and on its rules one by one, and the properties of the CPU restatement (tests/spalias_priors_restatement.py) that
the device tests then rely on."""
import math
import os

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import priors
from ldagroupedgibbssampler_amd.frontend import load_dataset
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import spalias_priors_restatement as PR
from tests import spalias_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "datasets")
PRIORS = os.path.join(ROOT, "tests", "golden", "priors")
SEED = 777


@pytest.fixture(scope="module")
def small_texts():
    c = load_dataset(os.path.join(DATA, "SmallTexts.txt"), stoplist=os.path.join(DATA, "stoplist.txt")).corpus
    assert (c.num_docs, c.num_types, c.num_tokens) == (5, 20, 23)
    return c


# ---- the parser on the reference's fixtures -----------------------------------------------------------------------------
def test_small_texts_fixture_is_the_reference_tests_matrix(small_texts):
    """SpaliasUncollapsedTestPhiPriors.testSetPriors, its statements on getTopicPriors"""
    v = {w: i for i, w in enumerate(small_texts.vocab)}
    assert [v[w] for w in ("mother", "slip", "disk", "drive")] == [15, 13, 1, 2]
    topics, words = priors.load_zero_cells(os.path.join(PRIORS, "topic_priors_SmallTexts.txt"), 4, small_texts.vocab)
    P = priors.priors_matrix(4, small_texts.num_types, topics, words)
    for w in ("mother", "slip"):
        assert P[0, v[w]] == 1.0 and (P[1:, v[w]] == 0.0).all()
    for w in ("disk", "drive"):
        assert P[3, v[w]] == 1.0 and (P[:3, v[w]] == 0.0).all()
    assert int((P == 0.0).sum()) == 12 == len(topics)
    assert list(zip(topics.tolist(), words.tolist())) == sorted(zip(topics.tolist(), words.tolist()))


@pytest.mark.parametrize("name", ["topic_priors.txt", "main_topic_priors.txt"])
def test_words_outside_the_vocabulary_zero_nothing(small_texts, name):
    """testSetPriorsNoWordsIsInDictionary: every prior stays 1.0; one warning per word, the topic-19 line (>= K) included"""
    assert "java" not in small_texts.vocab and "cell" not in small_texts.vocab
    warnings = []
    topics, words = priors.load_zero_cells(os.path.join(PRIORS, name), 4, small_texts.vocab, warn=warnings.append)
    assert topics.size == 0 and words.size == 0
    named = {"topic_priors.txt": 7, "main_topic_priors.txt": 9}[name]
    assert len(warnings) == named and len(set(warnings)) == named


# ---- the parser's rules -----------------------------------------------------------------------------------------------
VOCAB = ["a", "b", "x", "y", "z"]


def cells(lines, K=3, vocab=VOCAB):
    t, w = priors.zero_cells(lines, K, vocab, warn=lambda m: None)
    return sorted(zip(t.tolist(), w.tolist()))


def test_comment_and_blank_lines_are_skipped():
    want = [(1, 2), (2, 2)]
    assert cells(["0,x"]) == want
    assert cells(["# 1,y", "", "   ", "\t# more", "0,x", " #2,z"]) == want


def test_sets_hold_the_words_untrimmed():
    # "x" is kept in topic 0 and " x" in topic 1: the removal works on the untrimmed strings, so topic 0 still zeroes " x"
    # (the word x) and topic 1 still zeroes "x" -- x ends up zero in every topic, which the consistency check refuses
    with pytest.raises(ValueError, match=r"\[x\]"):
        cells(["0,a,x", "1,b, x"])
    # with the same spelling on both lines the word is kept in both topics and zeroed in the third only
    assert cells(["0,x", "1,x"]) == [(2, 2)]
    # a trimmed lookup: " y " names y
    assert cells(["2, y "]) == [(0, 3), (1, 3)]
    spec = priors.extract_prior_spec(["0,a,x", "1,b, x"], 3)
    assert spec == [[" x", "b"], ["a", "x"], [" x", "a", "b", "x"]]


def test_a_topic_beyond_K_zeroes_its_words_everywhere():
    assert priors.extract_prior_spec(["7,y"], 3) == [["y"], ["y"], ["y"]]
    with pytest.raises(ValueError, match=r"\[y\]"):
        cells(["7,y"])
    assert cells(["7,y", "1,y"]) == [(0, 3), (2, 3)]                 # kept where a line with a topic below K names it
    assert cells(["-1,q"]) == []                                     # parses; the word is not in the vocabulary


@pytest.mark.parametrize("line", [" 3,x", "3 ,x", "three,x", ",x", "1.0,x", "99999999999,x"])
def test_an_unparsable_topic_raises(line):
    with pytest.raises(ValueError):
        cells([line])


def test_a_topic_with_every_word_zero_raises():
    with pytest.raises(ValueError, match="one topic has all Zero priors"):
        cells(["0,a,b,x,y,z"], K=2)
    assert len(cells(["0,a,b,x,y"], K=2)) == 4


def test_read_lines_ends_lines_as_java_does(tmp_path):
    p = tmp_path / "p.txt"
    p.write_bytes(b"0, a\r\n1,b\n\n2,x")
    assert priors.read_lines(str(p)) == ["0, a", "1,b", "", "2,x"]
    assert priors.read_lines(os.path.join(PRIORS, "topic_priors_SmallTexts.txt")) == ["0, mother, slip", "3, disk, drive"]


# ---- the restatement's properties -------------------------------------------------------------------------------------
def row_sums(phi):
    return np.asarray([math.fsum(row) for row in phi.tolist()])      # exact: nothing of the measurement in the figure


def corpora(small_texts, cats):
    rng = np.random.default_rng(1)
    yield "SmallTexts", small_texts, 4, priors.load_zero_cells(os.path.join(PRIORS, "topic_priors_SmallTexts.txt"), 4, small_texts.vocab)
    yield "cats", cats, 5, PR.random_cells(rng, 5, cats.num_types, 10, 20, np.bincount(cats.tokens, minlength=cats.num_types))


def test_masked_cells_stay_zero_and_rows_keep_their_mass(oracle, small_texts, cats):
    for name, c, K, zc in corpora(small_texts, cats):
        z0 = java_lcg_initial_z(c.num_tokens, K, 5)
        m = PR.Model(K, c.num_types, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, z0, cells=zc)
        m.init_phi()
        masked = m.P == 0.0
        assert masked.sum() == len(set(zip(zc[0].tolist(), zc[1].tolist())))
        assert (m.phi[masked] == 0.0).all() and not np.signbit(m.phi[masked]).any() and (m.phi[~masked] > 0.0).all()
        mass0 = row_sums(m.phi)
        assert (mass0 < 1.0).any()                                   # rows are not renormalised
        n, worst = c.num_types, 0.0
        for s in range(20):
            m.sweep(1)
            assert (m.phi[masked] == 0.0).all() and not np.signbit(m.phi[masked]).any(), "%s sweep %d" % (name, s + 1)
            rel = np.abs(row_sums(m.phi) - mass0) / mass0
            worst = max(worst, float(rel.max()))
            assert (rel <= n * 2.0 ** -52).all(), "%s sweep %d: %s" % (name, s + 1, rel)
        print("%s: rows drift by at most %.3g relative in 20 sweeps (bound %.3g)" % (name, worst, n * 2.0 ** -52))


def test_the_literal_prior_factor_changes_no_bit_of_z(oracle, small_texts, cats):
    """cnt * phi * prior == cnt * phi while Phi is exactly zero wherever the prior is: spalias's z step on the same Phi"""
    for name, c, K, zc in corpora(small_texts, cats):
        z0 = java_lcg_initial_z(c.num_tokens, K, 5)
        m = PR.Model(K, c.num_types, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, z0, cells=zc)
        m.init_phi()
        for s in range(20):
            plain = m.z.copy()
            R.z_step(m.doc_ptr, m.tokens, plain, m.phi, m.tables, SEED, m.iteration + 1)
            m.sweep(1)
            assert np.array_equal(m.z, plain), "%s sweep %d" % (name, s + 1)


def test_an_empty_cell_list_is_not_plain_spalias_and_no_priors_is(oracle, cats):
    K = 5
    z0 = java_lcg_initial_z(cats.num_tokens, K, 5)
    none = np.zeros(0, np.int32)
    plain = R.Model(K, cats.num_types, 0.1, 0.01, SEED, cats.doc_ptr, cats.tokens, z0)
    nothing = PR.Model(K, cats.num_types, 0.1, 0.01, SEED, cats.doc_ptr, cats.tokens, z0, cells=None)
    empty = PR.Model(K, cats.num_types, 0.1, 0.01, SEED, cats.doc_ptr, cats.tokens, z0, cells=(none, none))
    for m in (plain, nothing, empty):
        m.init_phi()
        m.sweep(2)
    assert np.array_equal(nothing.z, plain.z) and np.array_equal(nothing.phi.view(np.int64), plain.phi.view(np.int64))
    assert (empty.P == 1.0).all()
    assert not np.array_equal(empty.phi.view(np.int64), plain.phi.view(np.int64))
    assert np.allclose(empty.phi, plain.phi, rtol=1e-12, atol=0)     # the same gammas, normalised by another expression
