"""adlda_wave_kernel and adlda_head_kernel on the knife-edge rows of tests/adlda_knife_edge.py: every comparison of the
token draw -- sample < Q, sample - Q < R, the stop of the Q, the R and the S walk -- with its two sides equal or one double
apart, at the first entries, across the 63 / 64 seam of a list of more than 64 entries, at the last entries and next to a
score-0.0 entry; the reference's rare paths that alpha can reach (a Q walk past its last entry: GGS_ERR_INVALID_TOPIC and
the clamped topic; the R walk's K - 1 fallback); and the proposal rows, which the wave scans decide when the margin is
unset.  Both forms: GGS_DEBUG_MARGIN unset (the proposal with its margins, the undecided tokens replayed) and 1e30 (every
token through the exact chains).  That the chains and the walks round as the restatement's left-to-right ones is what these
rows test (tests/test_adlda_knife_edge_model.py shows that each wrong order or comparison moves some of them, and none of
the random corpora of tests/test_adlda_gpu.py).

Alpha is fixed at ggs_create: every knob value is a handle of its own, closed before the next opens.  The whole z step is
compared with the restatement's at Edges.full_handles() (the first, the last, the proposal rows' and one per comparison,
with the four counters and, at the first and the last, the words' lists); at every other handle the target of EVERY row
and the tokens in front of it are compared with the builder's step(), which the model test holds against the whole
restatement step at all of them."""
import time

import numpy as np
import pytest

from tests import adlda_knife_edge as KE
from tests import adlda_restatement as R
from tests.ranks import assert_bit_equal, force_form
from tests.test_adlda_knife_edge_model import assert_survey, print_survey
from tests.test_polyaurn_sparse_knife_edge_gpu import FORMS

pytestmark = pytest.mark.gpu

KERNEL = "adlda_wave_kernel"


def report(ed, what, mism, stat_mism):
    """counts by (comparison, position, tag), then the first eight tokens with the device's and the expected topics"""
    if mism:
        row_of = {r.target: r for r in ed.rows}
        proposal = {t: k for k, toks in ed.proposals.items() for t in toks}
        by, first = {}, []
        for h, tok, dev, want in mism:
            row = row_of.get(tok)
            key = ed.label(row, h) if row is not None else ("proposal",) + proposal[tok] if tok in proposal and h == ed.base else ("another token", "-", "-")
            by[key] = by.get(key, 0) + 1
            if len(first) < 8:
                first.append("%s at handle %d: device %d expected %d" % (ed.describe(row) if row is not None else "token %d" % tok, h, dev, want))
        pytest.fail("%s: %d tokens differ; by (comparison, position, tag) %s; first: %s" % (what, len(mism), sorted(by.items()), first))
    assert not stat_mism, "%s: bucket counters (handle, device, restatement): %s" % (what, stat_mism[:8])


@pytest.mark.parametrize("margin", FORMS)
def test_knife_edge_rows(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    t_start = time.perf_counter()
    ed = KE.edges()
    handles, full = ed.handles(), ed.full_handles()
    assert len(handles) <= KE.MAX_HANDLES and ed.raises and not set(full) & ed.raises
    _, _, nw, lists = R.head(ed.n_wk, ed.n_k, KE.ALPHA, KE.BETA)
    mism, stat_mism, ms, raised = [], [], [], []
    for h in handles:
        t0 = time.perf_counter()
        g = native.GGSHandle(KE.K, ed.V, ed.knobs(h), KE.BETA, KE.SEED, flags=native.FLAG_ADLDA | native.FLAG_PARANOID)
        g.set_corpus(ed.doc_ptr, ed.tokens)
        ms.append(1e3 * (time.perf_counter() - t0))
        try:
            g.set_z(ed.z0, redraw_phi=True)
            g.set_iteration(KE.ITERATION - 1)
            if h in (handles[0], handles[-1]):                      # a wrong list must not hide behind a matching z
                gnw, glists = g.word_topic_lists()
                assert_bit_equal(gnw, nw, "nw, handle %d" % h)
                assert_bit_equal(glists, lists, "lists, handle %d" % h)
            before = g.sparse_stats()
            if h in ed.raises:                                      # the Q walk past its last entry: reported, the topic clamped
                with pytest.raises(native.GGSError) as e:
                    g.sweep(1)
                assert e.value.code == native.ERR_INVALID_TOPIC
                raised.append(h)
            else:
                g.sweep(1)
            z = g.get_z()
            if h in full:
                want, stats = ed.restatement(h)
                for tok in np.flatnonzero(z != want):
                    mism.append((h, int(tok), int(z[tok]), int(want[tok])))
                got = g.sparse_stats() - before
                if not np.array_equal(got, stats):
                    stat_mism.append((h, got.tolist(), stats.tolist()))
            else:
                for tok, k in sorted(ed.expect[h].items()):
                    if z[tok] != k:
                        mism.append((h, tok, int(z[tok]), k))
            assert g.launch_info()["z_kernel"].startswith(KERNEL)
        finally:
            g.close()                                               # each closed before the next opens
    assert raised == sorted(ed.raises)
    print("GGS_DEBUG_MARGIN %s: %d handles, %d of them compared whole, %d raise GGS_ERR_INVALID_TOPIC; create + set_corpus of a handle "
          "(K = %d, V = %d, %d tokens): median %.1f ms, max %.1f ms; the test took %.1f s" % (
              margin, len(handles), len(full), len(raised), KE.K, ed.V, ed.tokens.size, float(np.median(ms)), max(ms), time.perf_counter() - t_start))
    print_survey(ed)
    assert_survey(ed)
    report(ed, "knife-edge rows, GGS_DEBUG_MARGIN %s" % margin, mism, stat_mism)
