"""heldout_particles_kernel against the model: the device's own per-document values under the two statistics of
tests/test_heldout_model.py (the enumerated sequential-proposal limit, tests/heldout_model.py), and bit for bit against the
oracle where the oracle is fast enough (up to K = 1024: two seconds; four at K = 2049).

The fixture has K = 3.  The other instantiations are reached without leaving it:
  padded topics   alpha = 1e-12 for topics 3 .. K - 1, no training token on them: K = 100 (the shallow coefficient table),
                  1024 (the LDS-bound shape) and 2049 (SPILL).  The statistic is still taken against the K = 3 limit: the
                  padding moves sum log E_n by order K * 1e-12 (HM.padding_bound; asserted against limit() with the padded
                  smoothing mass in tests/test_heldout_model.py and again here), many orders below the 3e-3 standard error.
  wider counts    every document padded to 300 tokens with out-of-vocabulary ids: the two-byte count class
                  (heldout_particles_kernel<uint16_t>), at K = 1100 the spilled one.  Those ids take no draw and no
                  tokensSoFar: the values must be those of the unpadded documents, bit for bit."""
import numpy as np
import pytest

from tests import heldout_model as HM
from tests.test_heldout_model import oracle_on_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def limits():
    n_wk, n_k = HM.train_counts()
    return [HM.limit(doc, n_wk, n_k, HM.ALPHA, HM.BETA) for doc in HM.DOCS]


def device_on_fixture(native, seed, num_topics=HM.K):
    ptr, tok, z = HM.train_corpus()
    g = native.GGSHandle(num_topics, HM.V, HM.padded_alpha(num_topics), HM.BETA, seed)
    g.set_corpus(ptr, tok)
    g.set_z(z, redraw_phi=False)
    n_wk, n_k = HM.train_counts(num_topics)
    assert np.array_equal(g.get_type_topic_counts(), n_wk) and np.array_equal(g.get_topic_totals(), n_k)
    return g


def assert_same_bits(got, want, what):
    bad = np.flatnonzero(np.asarray(got).view(np.int64) != np.asarray(want).view(np.int64))
    assert bad.size == 0, (what, bad.size, bad[:5], np.asarray(got)[bad[:5]], np.asarray(want)[bad[:5]])


@pytest.mark.parametrize("num_topics,with_oracle", [(3, True), (100, True), (1024, True), (2049, False)])
def test_device_estimates_against_the_enumerated_limit(native, oracle, limits, num_topics, with_oracle):
    seed = 7 + num_topics
    n_wk, n_k = HM.train_counts()
    for doc, lim in zip(HM.DOCS, limits):                                # what the padding moves: far below the statistic's bound
        on_paths, leaked = HM.padding_bound(doc, n_wk, n_k, HM.ALPHA, HM.BETA, num_topics - HM.K)
        padded = HM.limit(doc, n_wk, n_k, HM.ALPHA, HM.BETA, pad_topics=num_topics - HM.K, pad_alpha=HM.PAD_ALPHA)
        assert abs(padded.log_e - lim.log_e) <= on_paths + leaked
        assert (on_paths + leaked) / np.sqrt(lim.var_g / HM.P) * np.sqrt(HM.R) <= 0.05
    ptr, tok, which = HM.heldout_corpus()
    g = device_on_fixture(native, seed, num_topics)
    g.set_test_corpus(ptr, tok)
    total, ll = g.heldout_log_likelihood(HM.P)
    g.close()
    stats = HM.statistics(ll, which, limits, HM.P)
    print("device, K = %d: (|mean z| sqrt(R), mean z^2, max |z|) per document %s" % (num_topics, np.round(stats, 2).tolist()))
    if with_oracle:
        o = oracle_on_fixture(oracle, seed, num_topics, threads=16)
        want_total, want = o.heldout_log_likelihood(ptr, tok, HM.P)
        o.close()
        assert_same_bits(ll, want, "K = %d" % num_topics)
        assert total == want_total
    assert HM.accepted(stats), stats


@pytest.mark.parametrize("num_topics", [3, 1100])
def test_out_of_vocabulary_padding_to_the_wider_count_types_changes_no_bit(native, num_topics):
    copies = 12                                                          # 48 documents * 4 000 particles * 300 positions * 8 bytes = 461 MB of word probabilities
    assert copies * len(HM.DOCS) * HM.P * 300 * 8 < 512e6
    ptr, tok, _ = HM.heldout_corpus(copies)
    wide_ptr, wide_tok, _ = HM.heldout_corpus(copies, pad_to=300)
    assert (np.diff(wide_ptr) == 300).all() and (wide_tok >= HM.V).sum() == wide_tok.size - tok.size
    g = device_on_fixture(native, 31, num_topics)
    g.set_test_corpus(ptr, tok)
    total, ll = g.heldout_log_likelihood(HM.P)
    g.set_test_corpus(wide_ptr, wide_tok)
    wide_total, wide_ll = g.heldout_log_likelihood(HM.P)
    g.close()
    assert_same_bits(wide_ll, ll, "K = %d, 300-token documents" % num_topics)
    assert wide_total == total
