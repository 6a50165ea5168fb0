"""scheme=nzvsspalias on the device at its exact edges (tests/nzvs_knife_edge.py; tests/test_nzvs_knife_edge_model.py checks the
rows themselves on the CPU).

The chain: the cascade rows (one round per 32-cell word, up to 258 rounds) and the window rows (lookups on the last entry of the
table of p(s), on the first behind it and far above it; the window clamped at 0 and at kVsTab) with their uniforms handed in --
drawn set, s at the row's end AND the round count against the numpy model of the rounds, on both paths; rows of 8193, 16385,
kVsLdsMaxV and kVsLdsMaxV + 1 cells under the Philox uniforms against the sequential chain; one whole handle at kVsLdsMaxV + 1
words, whose chain can only run in global scratch.

The z step: the narrow and the wide fixture of tests/polyaurn_sparse_knife_edge.py through nzvs_wave_kernel (every token there has
a candidate: the expectation is polyaurn_sparse's, which the model test shows), and the rows without a candidate on the edge of
frac > ps[w][i]; both forms of GGS_DEBUG_MARGIN."""
import numpy as np
import pytest

from tests import nzvs_knife_edge as NE
from tests import nzvs_restatement as R
from tests import polyaurn_sparse_knife_edge as KE
from tests.ranks import assert_bit_equal, force_form

pytestmark = pytest.mark.gpu

SEED = 777
BETA = NE.BETA
KERNEL = "nzvs_wave_kernel (wave per document)"
FORMS = [None, "1e30"]                  # GGS_DEBUG_MARGIN: the proposal with its margins / every token replayed exactly
PATHS = ["lds", "global"]               # the chain's rows in LDS / in global scratch (GGS_DEBUG_VS_GLOBAL=1)


def force_path(monkeypatch, path):
    """path None: no knob set, the library's own choice by V"""
    monkeypatch.setenv("GGS_DEBUG", "1")
    if path == "global":
        monkeypatch.setenv("GGS_DEBUG_VS_GLOBAL", "1")
    else:
        monkeypatch.delenv("GGS_DEBUG_VS_GLOBAL", raising=False)


# ---- the chain ------------------------------------------------------------------------------------------------------
def run_rows(native, rows, pi):
    """rows [(counts, prev_phi, U)] of one length in one call, a row per topic: drawn set, s_end and rounds against the rounds'
    model, all exactly.  Returns the device's rounds."""
    want = [R.rounds_chain(c, p, u, BETA, pi) for c, p, u in rows]
    d, s, rounds = native.debug_vs_indicators(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), BETA, pi, SEED, 1,
                                              u=np.array([r[2] for r in rows]))
    for i, (wd, ws, wr) in enumerate(want):
        wrong = np.flatnonzero(d[i] != wd)
        assert wrong.size == 0, "row %d of V=%d: %d cells differ, the first at %d; %d rounds against %d" % (i, d[i].size, wrong.size, wrong[0], rounds[i], wr)
        assert s[i] == ws, "row %d: s at the row's end" % i
        assert rounds[i] == wr, "row %d of V=%d: %d rounds on the device, %d in the model (the drawn set agrees)" % (i, d[i].size, rounds[i], wr)
    return [int(r) for r in rounds]


@pytest.mark.parametrize("path", PATHS)
def test_cascade_rows_round_for_round(native, oracle, monkeypatch, path):
    force_path(monkeypatch, path)
    for W in NE.CASCADE_W:
        for tail in NE.CASCADE_TAILS:
            rounds = run_rows(native, NE.cascade_group(W, tail, BETA, 0.5), 0.5)
            print("%s: cascade W=%d tail=%d: rounds %s" % (path, W, tail, rounds))
            assert rounds == [W + 1] * 3


@pytest.mark.parametrize("path", PATHS)
def test_window_rows(native, oracle, monkeypatch, path):
    force_path(monkeypatch, path)
    rows = NE.window_rows(BETA)
    for V in sorted({r[1].size for r in rows}):
        for pi in (0.5, 0.01):
            group = [r for r in rows if r[1].size == V and r[4] == pi]
            if group:
                rounds = run_rows(native, [r[1:4] for r in group], pi)
                print("%s: V=%d pi=%g: %s" % (path, V, pi, ", ".join("%s: %d rounds" % (r[0], n) for r, n in zip(group, rounds))))


_long = {}


def long_reference(V):
    """the long rows' sequential chain and the model's rounds under the Philox uniforms: once per length, for both paths"""
    if V not in _long:
        from oracle import oracle as O
        counts, prev = NE.long_row_inputs(V)
        K = counts.shape[0]
        U = O.uniforms(SEED, 3, R.PURPOSE_VS, 0, K * V).reshape(K, V)
        seq = [R.sequential_chain(counts[k], prev[k], U[k], BETA, 0.5) for k in range(K)]
        assert not any(r[2] for r in seq)
        rounds = [R.rounds_chain(counts[k], prev[k], U[k], BETA, 0.5)[2] for k in range(K)]
        _long[V] = (counts, prev, np.array([r[0] for r in seq]), np.array([r[1] for r in seq], np.int32), np.array(rounds, np.int32))
    return _long[V]


@pytest.mark.parametrize("V,path", [(V, p) for V in NE.LONG_V[:3] for p in PATHS] + [(NE.LONG_V[3], None)])
def test_long_rows_equal_the_sequential_chain(native, oracle, monkeypatch, V, path):
    force_path(monkeypatch, path)
    counts, prev, drawn, s_end, want_rounds = long_reference(V)
    d, s, rounds = native.debug_vs_indicators(counts, prev, BETA, 0.5, SEED, 3)
    print("V=%d (%d words, %d to a thread of the scan) %s: rounds %s" % (V, (V + 31) // 32, ((V + 31) // 32 + NE.KVS_BLOCK - 1) // NE.KVS_BLOCK,
                                                                        path or "no knob: global scratch", [int(r) for r in rounds]))
    assert_bit_equal(d, drawn, "drawn set, V=%d" % V)
    assert_bit_equal(s, s_end, "s at the row's end, V=%d" % V)
    assert_bit_equal(rounds, want_rounds, "rounds, V=%d" % V)


def test_a_whole_handle_past_the_lds_limit(native, oracle, monkeypatch):
    """V = kVsLdsMaxV + 1 and no knob: ggs_create's own choice of the global path and its work space.  Two sweeps: the second
    chain starts from a Phi with zeros."""
    force_path(monkeypatch, None)
    K, V, docs, length = 3, NE.KVS_LDS_MAX_V + 1, 40, 30
    tokens = np.random.default_rng(2).integers(0, V, docs * length).astype(np.int32)
    tokens[0], tokens[-1] = 0, V - 1
    doc_ptr = (np.arange(docs + 1) * length).astype(np.int64)
    g = native.GGSHandle(K, V, 0.1, BETA, SEED, flags=native.FLAG_NZVSSPALIAS | native.FLAG_PARANOID)
    g.set_corpus(doc_ptr, tokens)
    g.init_z_java_lcg(5)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, V, 0.1, BETA, SEED, doc_ptr, tokens, z0)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(2):
        zeros_before = int((m.phi == 0.0).sum())
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
        assert_bit_equal(g.get_phi(), m.phi, "phi after sweep %d" % (s + 1))
        vs = g.vs_stats()
        assert tuple(vs[:2]) == m.vs_stats_first_two(), "vs_stats after sweep %d" % (s + 1)
        assert_bit_equal(g.word_topic_lists()[0], m.nw, "nw after sweep %d" % (s + 1))
        assert 1 <= vs[2] <= V + 1
        print("V=%d handle, sweep %d: the chain started from %d zeros; %d cells undrawn, %d zero, at most %d rounds" % (V, s + 1, zeros_before, vs[0], vs[1], vs[2]))
        assert s == 0 or zeros_before > K * V // 100
    assert g.launch_info()["z_kernel"] == KERNEL
    g.close()


# ---- the z step -----------------------------------------------------------------------------------------------------
def row_key(ke, sv, r, j):
    row = ke.rows[r]
    return (KE.LIST_NAME[row.lst], row.kind, row.pos, sv["evals"][r][j][0])


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("name", ["narrow", "wide"])
def test_polyaurn_sparse_knife_edge_rows_through_nzvs(native, oracle, monkeypatch, name, margin):
    """tests/test_polyaurn_sparse_knife_edge_gpu.py::test_knife_edge_rows, loop for loop, under GGS_FLAG_NZVSSPALIAS"""
    force_form(monkeypatch, margin)
    ke = KE.fixture(name)
    sv = ke.survey()
    g = native.GGSHandle(ke.K, ke.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_NZVSSPALIAS | native.FLAG_PARANOID)
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
    print("%s through nzvs, GGS_DEBUG_MARGIN %s: %d scan values, %d raise INVALID_TOPIC; pairs %s; sparse_stats %s" %
          (name, margin, ke.J, raised, sorted(sv["pairs"].items()), [int(x) for x in stats]))
    assert not wrong and not builder_wrong, "mismatches by (list, kind, position, category) against the restatement: %s; against the builder: %s" % (
        sorted(wrong.items()), sorted(builder_wrong.items()))
    assert stats[R.ALIAS] == 0                                      # no token without a candidate: nothing here is the scheme's own branch
    if name == "narrow":     # a step that raises has still run every token: its counters are any other step's
        want_stats += raised * per_step
        assert [int(x) for x in stats] == [int(x) for x in want_stats]


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("K", [8, 160])
def test_rows_without_a_candidate(native, oracle, monkeypatch, K, margin):
    """the alias draw of a token without a candidate with ps[w][i] on frac, next to it and far from it; every scan value against
    the restatement's whole step"""
    force_form(monkeypatch, margin)
    ae = NE.alias_fixture(K)
    sv = ae.survey()
    g = native.GGSHandle(K, ae.V, NE.ALPHA, BETA, NE.SEED, flags=native.FLAG_NZVSSPALIAS | native.FLAG_PARANOID)
    g.set_corpus(ae.doc_ptr, ae.tokens)
    g.set_z(ae.z0, redraw_phi=True)
    row_of = {row.target: r for r, row in enumerate(ae.rows)}
    wrong, want_stats = {}, np.zeros(4, np.int64)
    for j in range(ae.J):
        g.set_phi(ae.phi(j))
        g.set_z(ae.z0, redraw_phi=False)
        g.set_iteration(NE.ITERATION - 1)
        g.sample_z_given_phi(1)
        z = g.get_z()
        want_z, stats, _ = ae.restatement_z(j)
        want_stats += stats
        for tok in np.flatnonzero(z != want_z):
            key = sv["evals"][row_of[int(tok)]][j][0] if int(tok) in row_of else "zero column" if int(tok) in ae.zero_targets else "prefix"
            wrong[key] = wrong.get(key, 0) + 1
    assert g.launch_info()["z_kernel"] == KERNEL
    stats = g.sparse_stats()
    g.close()
    print("K=%d, GGS_DEBUG_MARGIN %s: %d rows without a candidate, %d scan values; scan values per category %s; sparse_stats %s" %
          (K, margin, len(ae.rows) + len(ae.zero_targets), ae.J, sorted(sv["values"].items()), [int(x) for x in stats]))
    assert not wrong, "mismatches by category: %s" % sorted(wrong.items())
    assert [int(x) for x in stats] == [int(x) for x in want_stats]
    assert stats[R.ALIAS] == ae.J * (len(ae.rows) + len(ae.zero_targets))
