"""lightpc_wave_kernel on the knife-edge rows of tests/lightpclda_knife_edge.py: every comparison of the token step --
alias cell, word accept, length branch, alpha-branch cell, document accept -- with its two sides equal or one double
apart, z and the three Metropolis-Hastings counters bit-compared with the restatement.  The kernel has no margin and no
replay path; that its few IEEE operations are the reference's, in the reference's order, is what these rows test
(tests/test_lightpclda_knife_edge_model.py shows that each wrong order or comparison moves some of them, and none of the
random corpus).

Phi-knob rows (a, e): one handle, one set_phi and one z step per scan value from the same z and iteration.  Alpha-knob
rows (b, c, d): one handle per alpha vector.  The alias rows also go through spalias_wave_kernel as one-token documents
(the empty-list path: x = U1, the same tables)."""
import time

import numpy as np
import pytest

from tests import lightpclda_knife_edge as KE
from tests import spalias_restatement as SR
from tests.ranks import assert_bit_equal

pytestmark = pytest.mark.gpu

KERNEL = "lightpc_wave_kernel"


def z_step_from_z0(g, ed, phi):
    """the builder's z, the builder's iteration, Phi: one z step; returns (z, the step's three counters)"""
    g.set_phi(phi)
    g.set_z(ed.z0, redraw_phi=False)
    g.set_iteration(KE.ITERATION - 1)
    before = g.mh_stats()
    g.sample_z_given_phi(1)
    return g.get_z(), g.mh_stats() - before


def compare(ed, h, z, stats, mism, stat_mism):
    want = ed.restatement(h)
    assert want is not None, "the restatement raises on %s" % h
    for tok in np.flatnonzero(z != want[0]):
        mism.append((h, int(tok), int(z[tok]), int(want[0][tok])))
    if not np.array_equal(stats, want[1]):
        stat_mism.append((h, stats.tolist(), want[1].tolist()))


def report(ed, what, mism, stat_mism):
    """counts by (comparison, tag, dt source), then the first eight rows with the device's and the restatement's topics"""
    if mism:
        row_of = {r.target: r for r in ed.rows}
        by, first = {}, []
        for h, tok, dev, want in mism:
            row = row_of.get(tok)
            key = ed.label(row, h) if row is not None else ("one-hot token", "-", "-")
            by[key] = by.get(key, 0) + 1
            if len(first) < 8:
                first.append("%s at %s: device %d restatement %d" % (ed.describe(row) if row is not None else "token %d" % tok, h, dev, want))
        pytest.fail("%s: %d tokens differ; by (comparison, tag, dt source) %s; first: %s" % (what, len(mism), sorted(by.items()), first))
    assert not stat_mism, "%s: MH counters (step, device, restatement): %s" % (what, stat_mism[:8])


def check_tables(g, phi, alpha, what):
    ps, a, tn = g.alias_tables()
    wps, wa, wtn = SR.alias_tables(phi, alpha)
    assert_bit_equal(tn, wtn, "typeNorm, " + what)
    assert_bit_equal(a, wa, "a, " + what)
    assert_bit_equal(ps, wps, "ps, " + what)


def test_phi_knob_rows_alias_cell_and_document_accept(native, oracle):
    pe = KE.edges("phi")
    t0 = time.perf_counter()
    g = native.GGSHandle(KE.K, pe.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_LIGHTPCLDA | native.FLAG_PARANOID)
    g.set_corpus(pe.doc_ptr, pe.tokens)
    t1 = time.perf_counter()
    g.set_z(pe.z0, redraw_phi=True)
    mism, stat_mism = [], []
    for j in range(2 * KE.SCAN + 1):
        phi = pe.phi(j)
        z, stats = z_step_from_z0(g, pe, phi)
        compare(pe, j, z, stats, mism, stat_mism)
        if j in (0, KE.SCAN, 2 * KE.SCAN):                          # a table off in the scanned cell must not hide behind a matching z
            check_tables(g, phi, KE.ALPHA, "Phi matrix %d" % j)
    assert g.launch_info()["z_kernel"].startswith(KERNEL)
    g.close()
    print("create + set_corpus of the Phi-knob handle (K = %d, %d tokens): %.1f ms; %d z steps; rows %s" % (
        KE.K, pe.tokens.size, 1e3 * (t1 - t0), 2 * KE.SCAN + 1, sorted((k, v) for k, v in pe.survey().items() if len(k) == 2)))
    report(pe, "Phi-knob rows", mism, stat_mism)


def test_alpha_knob_rows_word_accept_length_branch_and_alpha_cell(native, oracle):
    ae = KE.edges("alpha")
    mism, stat_mism, ms = [], [], []
    for v in range(KE.N_VECTORS):
        t0 = time.perf_counter()
        g = native.GGSHandle(ae.nK, ae.V, ae.vectors[v], KE.BETA, KE.SEED, flags=native.FLAG_LIGHTPCLDA | native.FLAG_PARANOID)
        g.set_corpus(ae.doc_ptr, ae.tokens)
        ms.append(1e3 * (time.perf_counter() - t0))
        try:
            g.set_z(ae.z0, redraw_phi=True)
            z, stats = z_step_from_z0(g, ae, ae.phi)
            compare(ae, v, z, stats, mism, stat_mism)
            if v in (0, KE.N_VECTORS - 1):
                check_tables(g, ae.phi, ae.vectors[v], "alpha vector %d" % v)
            assert g.launch_info()["z_kernel"].startswith(KERNEL)
        finally:
            g.close()                                               # each closed before the next opens
    print("create + set_corpus of an alpha-knob handle (K = %d, %d tokens): median %.1f ms, max %.1f ms over %d handles; rows %s" % (
        ae.nK, ae.tokens.size, float(np.median(ms)), max(ms), len(ms), sorted(ae.survey().items())))
    report(ae, "alpha-knob rows", mism, stat_mism)


def test_alias_rows_through_spalias_as_one_token_documents(native, oracle):
    al = KE.edges("alias")
    g = native.GGSHandle(KE.K, al.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(al.doc_ptr, al.tokens)
    g.set_z(al.z0, redraw_phi=True)
    mism = []
    for j in range(2 * KE.SCAN + 1):
        phi = al.phi(j)
        g.set_phi(phi)
        g.set_z(al.z0, redraw_phi=False)
        g.set_iteration(KE.ITERATION - 1)
        g.sample_z_given_phi(1)
        z, want = g.get_z(), al.spalias_z(j)
        for tok in np.flatnonzero(z != want):
            mism.append((j, int(tok), int(z[tok]), int(want[tok])))
        if j in (0, KE.SCAN, 2 * KE.SCAN):
            check_tables(g, phi, KE.ALPHA, "Phi matrix %d" % j)
    assert g.launch_info()["z_kernel"].startswith("spalias_wave_kernel")
    g.close()
    report(al, "alias rows through spalias", mism, [])
