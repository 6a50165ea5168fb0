"""lightcollapsed_wave_kernel and count_alias_build_kernel on the knife-edge rows of tests/lightcollapsed_knife_edge.py:
every comparison of the token step -- table or beta branch, table cell, beta cell, word accept, length branch, alpha
cell, document accept -- with its two sides equal or one double apart, z and the three Metropolis-Hastings counters
bit-compared with the restatement.  The kernel does not evaluate pi_w and pi_d as the restatement writes them (r2 .. r5 a
chunk ahead, q_a / q_b ahead or fresh, the t_is_z0 decrement); that they round as the reference's left-to-right products
is what these rows test (tests/test_lightcollapsed_knife_edge_model.py shows that each wrong order, cancelled pair or
comparison moves some of them, and none of the random corpora).

Alpha and beta are fixed at ggs_create: every knob value is a handle of its own, closed before the next opens."""
import time

import numpy as np
import pytest

from tests import lightcollapsed_knife_edge as KE
from tests import lightcollapsed_restatement as R
from tests.ranks import assert_bit_equal
from tests.test_lightcollapsed_knife_edge_model import assert_survey, print_survey
from tests.test_lightpclda_knife_edge_gpu import compare, report

pytestmark = pytest.mark.gpu

KERNEL = "lightcollapsed_wave_kernel"


def check_tables(g, want, what):
    """the tables and lists the sweep is about to build (tests/test_lightcollapsed_gpu.py::assert_tables_equal)"""
    ps, a, tn, nw, lists, _ = want
    gps, ga, gtn = g.alias_tables()
    gnw, glists = g.word_topic_lists()
    assert_bit_equal(gnw, nw, "nw, " + what)
    assert_bit_equal(glists, lists, "lists, " + what)
    assert_bit_equal(gtn, tn, "type_norm, " + what)
    assert_bit_equal(ga, a, "a, " + what)
    assert_bit_equal(gps, ps, "ps, " + what)


def run_family(native, ed, what):
    mism, stat_mism, ms = [], [], []
    handles = ed.handles()
    assert len(handles) <= KE.MAX_HANDLES
    for h in handles:
        alpha, _, beta = ed.knobs(h)
        t0 = time.perf_counter()
        g = native.GGSHandle(ed.nK, ed.V, np.asarray(alpha, np.float64), beta, KE.SEED, flags=native.FLAG_LIGHTCOLLAPSED | native.FLAG_PARANOID)
        g.set_corpus(ed.doc_ptr, ed.tokens)
        ms.append(1e3 * (time.perf_counter() - t0))
        try:
            g.set_z(ed.z0, redraw_phi=True)
            g.set_iteration(KE.ITERATION - 1)
            if h in (handles[0], handles[-1]):                      # a wrong table must not hide behind a matching z
                check_tables(g, ed.built(beta), "%s %d" % (what, h))
            before = g.mh_stats()
            g.sweep(1)
            compare(ed, h, g.get_z(), g.mh_stats() - before, mism, stat_mism)
            assert g.launch_info()["z_kernel"].startswith(KERNEL)
        finally:
            g.close()                                               # each closed before the next opens
    print("create + set_corpus of a handle of the %ss (K = %d, V = %d, %d tokens): median %.1f ms, max %.1f ms over %d handles" % (
        what, ed.nK, ed.V, ed.tokens.size, float(np.median(ms)), max(ms), len(ms)))
    print_survey(ed.survey())
    report(ed, "%s rows" % what, mism, stat_mism)


def test_alpha_knob_rows_word_accept_length_branch_alpha_cell_and_document_accept(native, oracle):
    ae = KE.edges("alpha")
    run_family(native, ae, "alpha vector")
    assert_survey(dict(list(ae.survey().items()) + list(KE.edges("beta").survey().items())))


def test_beta_knob_rows_branch_table_cell_and_beta_cell(native, oracle):
    run_family(native, KE.edges("beta"), "beta value")


def test_equal_count_words_through_the_table_build(native, oracle):
    """The words of tests/test_lightcollapsed_knife_edge_model.py whose topics all weigh the same, nnz = 1, 2, 3, 5, 7, 64,
    65: every bs is +-0 or one rounding away, so the lows / highs split of count_alias_build_kernel's pairing chain sits
    on its edge.  Tables and lists bit for bit, then one sweep's z and counters."""
    n_wk, n_k = KE.equal_count_words()
    doc_ptr, tokens, z0 = KE.equal_count_corpus()
    V, K, alpha, beta = n_wk.shape[0], KE.EQUAL_K, 0.1, 0.01
    g = native.GGSHandle(K, V, alpha, beta, KE.SEED, flags=native.FLAG_LIGHTCOLLAPSED | native.FLAG_PARANOID)
    g.set_corpus(doc_ptr, tokens)
    g.set_z(z0, redraw_phi=True)
    m = R.Model(K, V, alpha, beta, KE.SEED, doc_ptr, tokens, z0)
    assert (m.n_wk == n_wk).all() and (m.n_k == n_k).all()
    want = m.tables()
    assert want[3].tolist() == list(KE.EQUAL_NNZ) + [K]
    check_tables(g, want, "equal-count words")
    g.sweep(1)
    m.sweep(1)
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after one sweep")
    assert_bit_equal(g.mh_stats(), m.stats, "MH counters after one sweep")
    check_tables(g, m.tables(), "after one sweep")
    g.close()
