"""heldout_particles_kernel on the knife-edge vectors of tests/heldout_knife_edge.py: every comparison of the particle
pass -- term bucket, term walk, beta bucket, beta walk, smoothing walk -- with its two sides equal or one double apart, at
the ends of the kernel's own structure (compacted cells 0, 7, 8, 63, 64 and the last of 70; the beta walk's rounds of eight
topics; the first and the last topics of the smoothing walk; a count at the depth of the coefficient table).  The kernel
skips zero cells, pads its last round of cells and takes coefficients from a table or from a division where the oracle
does none of it: here the per-document values must still be the oracle's, bit for bit, and the total identical
(tests/test_heldout_knife_edge_model.py shows that each wrong relation moves some of these rows, and none of a random corpus).

Alpha is fixed at create: one handle per vector, each closed before the next opens."""
import time

import numpy as np
import pytest

from tests import heldout_knife_edge as KE
from tests.test_heldout_knife_edge_model import oracle_for

pytestmark = pytest.mark.gpu


def run_vectors(native, oracle, fam, monkeypatch, split_kind=None):
    """every vector of the family on the device against the oracle; the vectors of comparison split_kind once more with
    the test set cut into several batches.  Returns what differs."""
    ptr, tok = fam.test_corpus()
    train_ptr, train_tok, z = fam.train_corpus()
    cells = int(ptr[len(ptr) // 2]) * fam.P                          # word probabilities of half the test set: two batches at least
    mism, ms, splits = [], [], 0
    for v in fam.vectors:
        o = oracle_for(oracle, fam, v.slack)
        t0 = time.perf_counter()
        g = native.GGSHandle(fam.K, fam.V, fam.alpha_vector(v.slack), fam.beta, fam.seed)
        try:
            g.set_corpus(train_ptr, train_tok)
            g.set_z(z, redraw_phi=False)
            g.set_iteration(fam.iteration)
            g.set_test_corpus(ptr, tok)
            ms.append(1e3 * (time.perf_counter() - t0))
            assert np.array_equal(g.get_type_topic_counts(), fam.n_wk)
            if v.invalid:
                with pytest.raises(oracle.OracleError) as want:
                    o.heldout_log_likelihood(ptr, tok, fam.P)
                with pytest.raises(native.GGSError) as got:
                    g.heldout_log_likelihood(fam.P)
                assert want.value.code == oracle.ERR_INVALID_TOPIC and got.value.code == native.ERR_INVALID_TOPIC
                continue
            want_total, want = o.heldout_log_likelihood(ptr, tok, fam.P)
            runs = [g.heldout_log_likelihood(fam.P)]
            if v.kind == split_kind:
                monkeypatch.setenv("GGS_DEBUG_HELDOUT_CELLS", str(cells))
                runs.append(g.heldout_log_likelihood(fam.P))
                monkeypatch.delenv("GGS_DEBUG_HELDOUT_CELLS")
                splits += 1
            for total, ll in runs:
                bad = np.flatnonzero(ll.view(np.int64) != want.view(np.int64))
                if bad.size or total != want_total:
                    mism.append((fam.describe(v), "aimed document differs" if v.doc in bad else "another document differs", bad[:4].tolist(),
                                 ll[bad[:4]].tolist(), want[bad[:4]].tolist(), total, want_total))
        finally:
            g.close()
            o.close()
    print("%s: %d handles (K = %d, %d test documents, %d particles), create + corpus + test set median %.1f ms, max %.1f ms; %d vectors also in batches of %d cells" % (
        fam.name, len(fam.vectors), fam.K, len(fam.docs), fam.P, float(np.median(ms)), max(ms), splits, cells))
    return mism


def test_wide_rows_every_comparison_and_walk_end(native, oracle, monkeypatch):
    wide = KE.families(oracle)[0]
    mism = run_vectors(native, oracle, wide, monkeypatch, split_kind="b")
    assert not mism, "%d vectors differ; first: %s" % (len(mism), mism[:4])


def test_rows_at_the_depth_of_the_coefficient_table(native, oracle, monkeypatch):
    cap = KE.families(oracle)[1]
    mism = run_vectors(native, oracle, cap, monkeypatch)
    assert not mism, "%d vectors differ; first: %s" % (len(mism), mism[:4])
