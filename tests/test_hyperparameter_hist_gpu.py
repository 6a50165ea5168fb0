"""The two histogram kernels of the hyperparameter step (csrc/ggs_hyper_hist.hpp) against np.bincount over the host copies of the
same state: ggs_doc_topic_histogram over get_z() per document, ggs_type_topic_count_histogram over get_type_topic_counts().
Equality of int32 bins; the shapes are the smallest that reach every path of the kernels: the LDS table and the tail beyond it,
a document over 32 768 tokens, a bin above 65 535, V * K that is no multiple of 4, a third work item per workgroup under one CU."""
import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus
from tests import hyperparameter_restatement as R
from tests import persistent_grid as PG

pytestmark = pytest.mark.gpu

# the plan entries' caps (plan_launches, csrc/ggs_host_plan.hpp: pl.dochist, pl.cellhist = kHistPerCu workgroups of kHistWaves waves)
CAP_HIST, HIST_WAVES = 8, 4
CELLS_PER_ITEM = 64 * 16                 # kCellHistPerLane cells per lane and trip (csrc/ggs_hyper_hist.hpp)
HIST_TAB = 4096                          # kHistTabInts: bins below it are private to a workgroup in LDS, the others go to global atomics
LONG = 40000                             # a document beyond the int16 counts (32 767), the 32 768 boundary and every LDS table
V_DOC = 50


def _handle(native, K, V, cus, monkeypatch, scheme="pcgs"):
    monkeypatch.delenv(PG.KNOB, raising=False)
    if cus is not None:
        monkeypatch.setenv(PG.KNOB, str(cus))
    flags = native.FLAG_LIGHTPCLDAW2 if scheme == "lightpcldaw2" else native.SCHEME_FLAGS[scheme]
    h = native.GGSHandle(K, V, 0.1, 0.01, 5, flags=flags)
    monkeypatch.delenv(PG.KNOB, raising=False)
    return h


def _doc_corpus(K, seed=3):
    """documents of 0, 1, 63, 64 and 65 tokens, one of LONG tokens on a single topic, one that touches every topic once, and enough short
    ones that under one CU some workgroup takes a third document"""
    rng = np.random.default_rng(seed)
    lens = [0, 1, 63, 64, 65, LONG, K, 0, 1] + rng.integers(0, 30, 120).tolist()
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = rng.integers(0, V_DOC, int(doc_ptr[-1])).astype(np.int32)
    z = rng.integers(0, K, tokens.size).astype(np.int32)
    z[doc_ptr[5]:doc_ptr[6]] = K - 1
    z[doc_ptr[6]:doc_ptr[7]] = np.arange(K)
    return Corpus(doc_ptr, tokens, V_DOC), z


@pytest.mark.parametrize("cus", [None, 1])
@pytest.mark.parametrize("K", [3, 64, 65, 200, 1024])
def test_doc_topic_histogram_is_bincount_of_z(native, monkeypatch, K, cus):
    c, z0 = _doc_corpus(K)
    if cus is not None:
        PG.assert_trips(c.num_docs, cus, CAP_HIST, "doc_topic_hist_kernel", waves=HIST_WAVES)
    lens = np.diff(c.doc_ptr)
    assert {0, 1, 63, 64, 65, LONG} <= set(lens.tolist()) and LONG > 32768 and LONG > HIST_TAB
    h = _handle(native, K, V_DOC, cus, monkeypatch)
    try:
        h.set_corpus(c.doc_ptr, c.tokens)
        h.set_z(z0, redraw_phi=False)
        z = h.get_z()
        n_bins = int(lens.max()) + 1
        want_len = R.doc_length_counts(c.doc_ptr)
        for symmetric in (True, False):
            want = R.doc_topic_histogram(c.doc_ptr, z, K, symmetric, n_bins)
            assert want[-1 if not symmetric else 0, LONG] >= 1                   # the tail bin: beyond every table
            hist, lengths = h.doc_topic_histogram(symmetric, n_bins)
            assert hist.dtype == np.int32 and hist.shape == want.shape
            assert np.array_equal(hist, want), "symmetric=%s: %d bins differ" % (symmetric, (hist != want).sum())
            assert np.array_equal(lengths, want_len)
            only, none = h.doc_topic_histogram(symmetric, n_bins, lengths=False)
            assert none is None and np.array_equal(only, want)
            # more bins than needed: the same bins, zeros behind them
            wide, wl = h.doc_topic_histogram(symmetric, n_bins + 9)
            assert np.array_equal(wide[:, :n_bins], want) and not wide[:, n_bins:].any() and np.array_equal(wl[:n_bins], want_len) and not wl[n_bins:].any()
        assert int(hist[:, 0].astype(np.int64).sum()) + int(np.count_nonzero(R.doc_topic_counts(c.doc_ptr, z, K))) == c.num_docs * K
    finally:
        h.close()


def test_doc_topic_histogram_bin_range(native, monkeypatch):
    K = 5
    c, z0 = _doc_corpus(K)
    h = _handle(native, K, V_DOC, None, monkeypatch)
    try:
        h.set_corpus(c.doc_ptr, c.tokens)
        h.set_z(z0, redraw_phi=False)
        exact = LONG + 1                                                         # n_dk of the long document's one topic == its length
        for symmetric in (True, False):
            rows = 1 if symmetric else K
            out, lout = np.full((rows, exact - 1), -7, np.int32), np.full(exact - 1, -9, np.int32)
            with pytest.raises(native.GGSError) as e:
                h.doc_topic_histogram(symmetric, exact - 1, out=out, lengths_out=lout)
            assert e.value.code == native.ERR_BAD_ARG
            assert (out == -7).all() and (lout == -9).all()                       # nothing was written
            with pytest.raises(native.GGSError) as e:                             # without the lengths it is n_dk that is out of range
                h.doc_topic_histogram(symmetric, exact - 1, lengths=False, out=out)
            assert e.value.code == native.ERR_BAD_ARG and (out == -7).all()
            hist, _ = h.doc_topic_histogram(symmetric, exact)
            assert np.array_equal(hist, R.doc_topic_histogram(c.doc_ptr, z0, K, symmetric, exact))
        with pytest.raises(native.GGSError) as e:
            h.doc_topic_histogram(True, 0)
        assert e.value.code == native.ERR_BAD_ARG
    finally:
        h.close()


def test_symmetric_bin_zero_wraps_like_a_java_int(native, monkeypatch):
    """D * K pairs pass 2^31: bin 0 is the count modulo 2^32, every other bin exact.  All documents are empty but one, so nothing of
    size moves: the pairs are counted by arithmetic, not by atomics."""
    K, D = 4096, 600000
    assert D * K > 2 ** 31
    lens = np.zeros(D, np.int64)
    lens[17] = 3
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    h = _handle(native, K, 4, None, monkeypatch, "adlda")                        # a count-form scheme: no D x K theta is allocated
    try:
        h.set_corpus(doc_ptr, np.array([0, 1, 2], np.int32))
        h.set_z(np.array([5, 5, 9], np.int32), redraw_phi=False)
        hist, lengths = h.doc_topic_histogram(True, 4)
        assert hist[0, 1:].tolist() == [1, 1, 0] and lengths.tolist() == [D - 1, 0, 0, 1]
        assert hist[0, 0] == R.wrap_int32([D * K - 2])[0] and hist[0, 0] < 0
    finally:
        h.close()


SCHEMES = ("ggs", "pcgs", "collapsed", "polyaurn", "spalias", "lightpclda", "polyaurn_sparse", "lightcollapsed", "nzvsspalias", "adlda", "lightpcldaw2")


@pytest.mark.parametrize("scheme", SCHEMES)
def test_histograms_under_every_scheme_after_a_sweep(native, monkeypatch, scheme):
    """both calls read only z, doc_ptr and the counts: the same answers whatever the scheme, on the state a sweep left"""
    K, V = 7, 40
    c = PG.mixed_corpus([(30, 0, 25)], V, 8)
    h = _handle(native, K, V, None, monkeypatch, scheme)
    try:
        h.set_corpus(c.doc_ptr, c.tokens)
        h.init_z_java_lcg(11)
        h.init_phi()
        h.sweep(2)
        z, n_wk = h.get_z(), h.get_type_topic_counts()
        n_bins = int(np.diff(c.doc_ptr).max()) + 1
        for symmetric in (True, False):
            hist, lengths = h.doc_topic_histogram(symmetric, n_bins)
            assert np.array_equal(hist, R.doc_topic_histogram(c.doc_ptr, z, K, symmetric, n_bins)) and np.array_equal(lengths, R.doc_length_counts(c.doc_ptr))
        m = R.max_type_count(c.tokens, V)
        assert np.array_equal(h.type_topic_count_histogram(m + 1), R.cell_histogram(n_wk, m + 1))
        h.sweep(1)                                                               # and the chain goes on
    finally:
        h.close()


# ---- countHistogram ---------------------------------------------------------------------------------------------------------------
BULK = 70000                             # one word's tokens, all on one topic: a bin above 65 535, through the tail path


def _cell_corpus(V, K, seed=4):
    """word 0: BULK tokens on topic 1 % K and no others; word V - 1: no token (an all-zero row); the rest Zipf over a few thousand tokens"""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.full(7, BULK // 7), rng.integers(0, 60, 150)])
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p = 1.0 / np.arange(1, V - 1)
    tokens = (1 + rng.choice(V - 2, int(doc_ptr[-1]), p=p / p.sum())).astype(np.int32)
    z = rng.integers(0, K, tokens.size).astype(np.int32)
    tokens[:BULK] = 0
    z[:BULK] = 1 % K
    return Corpus(doc_ptr, tokens, V), z


@pytest.mark.parametrize("cus", [None, 1])
@pytest.mark.parametrize("V,K", [(97, 3), (1000, 65), (50, 4096)])
def test_cell_histogram_is_bincount_of_the_counts(native, monkeypatch, V, K, cus):
    c, z0 = _cell_corpus(V, K)
    assert BULK // 7 * 7 == BULK and BULK > 65535
    if cus is not None and V * K >= 3 * CAP_HIST * HIST_WAVES * CELLS_PER_ITEM:
        PG.assert_trips(-(-V * K // CELLS_PER_ITEM), cus, CAP_HIST, "cell_hist_kernel", waves=HIST_WAVES)
    h = _handle(native, K, V, cus, monkeypatch)
    try:
        h.set_corpus(c.doc_ptr, c.tokens)
        h.set_z(z0, redraw_phi=False)
        n_wk = h.get_type_topic_counts()
        assert n_wk[0, 1 % K] == BULK and not n_wk[V - 1].any()
        m = R.max_type_count(c.tokens, V)
        assert m == BULK
        want = R.cell_histogram(n_wk, m + 1)
        assert want[BULK] == 1 and want[0] == V * K - np.count_nonzero(n_wk)
        got = h.type_topic_count_histogram(m + 1)
        assert got.dtype == np.int32 and np.array_equal(got, want), "%d bins differ" % (got != want).sum()
        wide = h.type_topic_count_histogram(m + 30)
        assert np.array_equal(wide[:m + 1], want) and not wide[m + 1:].any()
        # n_bins one too small: refused, the buffer as it was; the exact size again afterwards
        out = np.full(m, -3, np.int32)
        with pytest.raises(native.GGSError) as e:
            h.type_topic_count_histogram(m, out=out)
        assert e.value.code == native.ERR_BAD_ARG and (out == -3).all()
        assert np.array_equal(h.type_topic_count_histogram(m + 1), want)
    finally:
        h.close()


def test_cell_histogram_small_counts_out_of_range(native, monkeypatch):
    """the counts 1, 2 and 3 are counted in registers: a histogram too short for them is refused all the same"""
    V, K = 6, 3
    doc_ptr = np.array([0, 6], np.int64)
    tokens = np.array([0, 0, 0, 1, 1, 2], np.int32)
    h = _handle(native, K, V, None, monkeypatch)
    try:
        h.set_corpus(doc_ptr, tokens)
        h.set_z(np.zeros(6, np.int32), redraw_phi=False)                          # cells of 3, 2 and 1
        for n_bins in (1, 2, 3):
            out = np.full(n_bins, -1, np.int32)
            with pytest.raises(native.GGSError) as e:
                h.type_topic_count_histogram(n_bins, out=out)
            assert e.value.code == native.ERR_BAD_ARG and (out == -1).all()
        assert h.type_topic_count_histogram(4).tolist() == [V * K - 3, 1, 1, 1]
    finally:
        h.close()
