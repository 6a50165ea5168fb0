"""scheme=polyaurn_sparse on the device at its exact edges (tests/polyaurn_sparse_knife_edge.py): every scan value of the
narrow fixture (K = 8, lists of 3 to 5) bit for bit against the whole restatement z step, every scan value of the wide
one (K = 160, every walk over more than 64 candidates) against the builder's expectation at the targets and z0 at the
prefix, the whole restatement step at three of them; both forms (GGS_DEBUG_MARGIN unset: the proposal with its margins;
1e30: every token replayed).  The alias rows whose column is non-zero in every topic are spalias's draw formula for
formula: they also run through spalias_wave_kernel, whose alias branch has no other edge test."""
import numpy as np
import pytest

from tests import polyaurn_sparse_knife_edge as KE
from tests.ranks import force_form

pytestmark = pytest.mark.gpu

KERNEL = "polyaurn_sparse_wave_kernel (wave per document)"
FORMS = [None, "1e30"]


def row_key(ke, sv, r, j):
    row = ke.rows[r]
    return (KE.LIST_NAME[row.lst], row.kind, row.pos, sv["evals"][r][j][0])


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_knife_edge_rows(native, oracle, monkeypatch, name, margin):
    force_form(monkeypatch, margin)
    ke = KE.fixture(name)
    sv = ke.survey()
    g = native.GGSHandle(ke.K, ke.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_POLYAURN_SPARSE | native.FLAG_PARANOID)
    g.set_corpus(ke.doc_ptr, ke.tokens)
    g.set_z(ke.z0, redraw_phi=True)
    row_of = {row.target: r for r, row in enumerate(ke.rows)}
    targets = np.array(sorted(row_of))
    prefix = np.ones(ke.z0.size, bool)
    prefix[targets] = False
    by_j = {}
    for j, tok, want, r, cat in sv["expect"]:
        by_j.setdefault(j, []).append((tok, want, r))
    valid = [j for j in range(ke.J) if j not in sv["invalid"]]
    full = set(valid) if name == "narrow" else {valid[0], min(valid, key=lambda j: abs(j - ke.SCAN)), valid[-1], valid[-2]}
    wrong, builder_wrong, raised = {}, {}, 0
    want_stats, per_step = np.zeros(4, np.int64), None
    for j in range(ke.J):
        g.set_phi(ke.phi(j))
        g.set_z(ke.z0, redraw_phi=False)
        g.set_iteration(KE.ITERATION - 1)
        if j in sv["invalid"]:                                      # x rounds to 1.0 right under the branch's edge
            if name == "narrow":
                assert ke.restatement_z(j)[0] is None
            with pytest.raises(native.GGSError) as e:
                g.sample_z_given_phi(1)
            assert e.value.code == native.ERR_INVALID_TOPIC
            raised += 1
            continue
        g.sample_z_given_phi(1)
        z = g.get_z()
        if j in full:
            want_z, stats = ke.restatement_z(j)
            assert want_z is not None
            want_stats += stats
            per_step = stats if per_step is None else per_step
            assert (stats == per_step).all()                        # which list and how many candidates: the same at every scan value
            for tok in np.flatnonzero(z != want_z):
                key = row_key(ke, sv, row_of[int(tok)], j) if int(tok) in row_of else ("prefix", "-", "-", "-")
                wrong[key] = wrong.get(key, 0) + 1
        for tok in np.flatnonzero(z[prefix] != ke.z0[prefix]):
            wrong[("prefix", "-", "-", "moved")] = wrong.get(("prefix", "-", "-", "moved"), 0) + 1
        for tok, want, r in by_j.get(j, ()):
            if z[tok] != want:
                key = row_key(ke, sv, r, j)
                builder_wrong[key] = builder_wrong.get(key, 0) + 1
    assert g.launch_info()["z_kernel"] == KERNEL
    stats = g.sparse_stats()
    g.close()
    print("%s, GGS_DEBUG_MARGIN %s: %d scan values, %d raise INVALID_TOPIC; pairs %s; sparse_stats %s" %
          (name, margin, ke.J, raised, sorted(sv["pairs"].items()), [int(x) for x in stats]))
    assert not wrong and not builder_wrong, "mismatches by (list, kind, position, category) against the restatement: %s; against the builder: %s" % (
        sorted(wrong.items()), sorted(builder_wrong.items()))
    if name == "narrow":     # a step that raises has still run every token: its counters are any other step's
        want_stats += raised * per_step
        assert [int(x) for x in stats] == [int(x) for x in want_stats]


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_the_same_rows_through_spalias(native, oracle, monkeypatch, name, margin):
    """The same corpus, uniforms and Phi matrices under GGS_FLAG_SPALIAS.  spalias walks the document's list in every
    row, so every DOC row is on its edge there too: the alias rows whose column is non-zero in every topic (frac against
    ps[w][i], ups against an integer), the branch rows, and in the wide fixture the walks across the seam of a list of
    more than 64 entries.  Every target against spalias's restatement of that token, every prefix token against z0, the
    whole restatement step at three scan values."""
    force_form(monkeypatch, margin)
    ke = KE.fixture(name)
    sv = ke.survey()
    want = ke.spalias_expect()
    shared = [r for r, row in enumerate(ke.rows) if row.shared and row.kind != "plain"]
    assert len(shared) >= 8
    g = native.GGSHandle(ke.K, ke.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(ke.doc_ptr, ke.tokens)
    g.set_z(ke.z0, redraw_phi=True)
    targets = np.array([row.target for row in ke.rows])
    prefix = np.ones(ke.z0.size, bool)
    prefix[targets] = False
    valid = [j for j in range(ke.J) if (want[j] >= 0).all()]
    full = {valid[0], min(valid, key=lambda j: abs(j - ke.SCAN)), valid[-1], valid[-2]}
    wrong, raised, moved = {}, 0, 0
    for j in range(ke.J):
        g.set_phi(ke.phi(j))
        g.set_z(ke.z0, redraw_phi=False)
        g.set_iteration(KE.ITERATION - 1)
        if (want[j] < 0).any():
            with pytest.raises(native.GGSError) as e:
                g.sample_z_given_phi(1)
            assert e.value.code == native.ERR_INVALID_TOPIC
            raised += 1
            continue
        g.sample_z_given_phi(1)
        z = g.get_z()
        if j in full:
            whole = ke.spalias_z(j)
            assert whole is not None and (z == whole).all(), "scan value %d: z differs from spalias's restatement step" % j
        moved += int((z[prefix] != ke.z0[prefix]).sum())
        for r in np.flatnonzero(z[targets] != want[j]):
            key = row_key(ke, sv, int(r), j)
            wrong[key] = wrong.get(key, 0) + 1
    assert g.launch_info()["z_kernel"].startswith("spalias_wave_kernel")
    g.close()
    print("%s, GGS_DEBUG_MARGIN %s through spalias: %d rows share the alias draw, %d scan values raise INVALID_TOPIC" % (name, margin, len(shared), raised))
    assert not wrong and not moved, "mismatches by (list, kind, position, polyaurn_sparse's category): %s; prefix tokens moved: %d" % (sorted(wrong.items()), moved)
