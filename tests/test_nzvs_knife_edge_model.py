"""The knife-edge rows of scheme=nzvsspalias (tests/nzvs_knife_edge.py) on the CPU: the cascade rows need one round per word and
come out wrong from a round loop that stops early; the window rows leave the chain kernel's table of p(s) on every side; the
restatement's z step is polyaurn_sparse's on every row of that scheme's knife-edge fixtures; the rows without a candidate
stand on the edge of frac > ps[w][i], and the two nearest wrong draws (polyaurn's uniform topic, >= for >) are told apart."""
import re
import time

import numpy as np

from tests import nzvs_knife_edge as NE
from tests import nzvs_restatement as R
from tests import polyaurn_sparse_knife_edge as KE
from tests import polyaurn_sparse_restatement as PS
from tests import spalias_restatement as SR

BETA = NE.BETA


# ---- the chain ------------------------------------------------------------------------------------------------------
def test_the_helper_restates_the_headers_constants():
    from ldagroupedgibbssampler_amd import _lib
    import os
    text = open(os.path.join(_lib.CSRC, "ggs_phi_vs.hpp")).read()
    m = re.search(r"constexpr int kVsBlock = (\d+), kVsTab = (\d+);", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (NE.KVS_BLOCK, NE.KVS_TAB)
    assert "constexpr int kVsLdsMaxV = 32 * ((48 * 1024) / 20);" in text and NE.KVS_LDS_MAX_V == 78624
    assert "w0 = max(0, s_min - 32), tn = min(kVsTab, s_max + 32 - w0 + 1)" in text      # window_report's rule
    assert "ti < (uint32_t)tn ? ptab[ti]" in text
    # what the long rows are for: words per thread of the block scan, and the two sides of the LDS limit
    per = [((V + 31) // 32 + NE.KVS_BLOCK - 1) // NE.KVS_BLOCK for V in NE.LONG_V]
    assert per[:2] == [2, 3] and ((8193 + 31) // 32) % per[0] == 1 and per[2] == per[3] == 10   # 257 words by twos: the last stretch is short
    assert max(NE.CASCADE_W) > NE.KVS_BLOCK


def test_cascade_rows_need_a_round_per_word(oracle):
    for W in NE.CASCADE_W:
        for tail in NE.CASCADE_TAILS:
            for c, p, u in NE.cascade_group(W, tail, BETA, 0.5):
                assert c.size == 32 * W + tail and int((c == 0).sum()) == W
                drawn, s_end, bad = R.sequential_chain(c, p, u, BETA, 0.5)
                assert not bad and (~drawn).sum() == W // 2                 # the odd words' cells, and only they, are undrawn
                d, s, rounds = R.rounds_chain(c, p, u, BETA, 0.5)
                assert np.array_equal(d, drawn) and s == s_end
                print("cascade W=%d tail=%d: V=%d, s0=%d, %d rounds" % (W, tail, c.size, int((p == 0.0).sum()), rounds))
                assert rounds == W + 1
                before = R.states_before(c, p, u, BETA, 0.5)
                assert before.min() > 32                                    # s stays well above 0
                # stopping at the first round that changes no decision: wrong on every one of them
                d, s, r = R.rounds_chain(c, p, u, BETA, 0.5, confirm=False)
                assert not np.array_equal(d, drawn)
                # a round loop that never reaches its fifth round: right while four suffice, wrong from W = 9 on
                d, s, r = R.rounds_chain(c, p, u, BETA, 0.5, max_rounds=4)
                assert np.array_equal(d, drawn) == (W + 1 <= 4), "the rows have no power over the round loop"


def test_window_rows_leave_the_table_on_every_side(oracle):
    seen = dict.fromkeys(NE.WINDOW_CATEGORIES, 0)
    for name, c, p, u, pi in NE.window_rows(BETA):
        rep = NE.window_report(c, p, u, BETA, pi)
        d, s, rounds = R.rounds_chain(c, p, u, BETA, pi)
        drawn, s_end, bad = R.sequential_chain(c, p, u, BETA, pi)
        assert np.array_equal(rep["drawn"], d) and rep["s_end"] == s and rep["rounds"] == rounds, name
        assert np.array_equal(d, drawn) and s == s_end and not bad, name
        print("%-28s %d rounds; lookups at ti == tn - 1: %d, ti == tn: %d, ti > tn: %d; w0 clamped at 0: %s, tn at kVsTab: %s" %
              (name, rounds, rep["at_last"], rep["at_end"], rep["above"], rep["w0_clamped"], rep["tn_clamped"]))
        for cat in NE.WINDOW_CATEGORIES:
            seen[cat] += int(rep[cat])
        if name.startswith("staircase"):                                # every lookup of a staircase is an exact tie
            assert rep["at_last"] >= 1 and rep["at_end"] >= 1 and rep["tn_clamped"], name
            steps, up = 1100, "up" in name
            before = R.states_before(c, p, u, BETA, pi)
            P = R.Probabilities(int(c.sum()), BETA, pi)
            for v in range(steps):
                assert u[v] == (np.nextafter(P(before[v]), 2.0) if up else P(before[v]))
            assert (not drawn[:steps].any()) if up else drawn[:steps].all()
        if name == "random V=4097 pi=0.01":
            assert rep["at_end"] + rep["above"] == 1303                 # the figure the rows were chosen by
        if not rep["tn_clamped"]:                                       # the table reaches s_max + 32: no lookup past tn - 2
            assert rep["at_last"] == rep["at_end"] == rep["above"] == 0, name
    for cat in NE.WINDOW_CATEGORIES:
        assert seen[cat] >= 1, "no row reaches %s" % cat


def test_the_long_rows_settle_in_a_few_rounds(oracle):
    """The long rows of the device test, here with uniforms of numpy's: the sequential chain is what the rounds give.  Only
    the shortest is run through the rounds (the device test holds every length against the sequential chain)."""
    V = NE.LONG_V[0]
    counts, prev = NE.long_row_inputs(V)
    U = np.random.default_rng(5).random(counts.shape)
    for k in range(counts.shape[0]):
        drawn, s_end, bad = R.sequential_chain(counts[k], prev[k], U[k], BETA, 0.5)
        d, s, rounds = R.rounds_chain(counts[k], prev[k], U[k], BETA, 0.5)
        assert np.array_equal(d, drawn) and s == s_end and not bad
        print("V=%d row %d: %d rounds" % (V, k, rounds))


# ---- the z step -----------------------------------------------------------------------------------------------------
def test_on_the_polyaurn_sparse_rows_the_draw_is_polyaurn_sparses(oracle):
    """Every target at every scan value of both fixtures through nzvsspalias's token_draw: the same list, the same number of
    candidates (three or more), the same topic or the same refusal, and no table read where polyaurn_sparse reads none.
    Whole steps at a few scan values: the same z and the same counters, none of them an alias-only draw."""
    t0 = time.time()
    for name in ("narrow", "wide"):
        ke = KE.fixture(name)
        sv = ke.survey()
        checked = 0
        for row, ev in zip(ke.rows, sv["evals"]):
            for j, (cat, want, new, det) in enumerate(ev):
                col = ke.column(row, j)
                ps, a = det["tables"] if det["tables"] is not None else (KE._NO_TABLE, KE._NO_TABLE)
                mine = {}
                try:
                    got = R.token_draw(row.st, col, np.flatnonzero(col != 0.0), ps, a, det["tn"], row.U, ke.K, mine)
                except SR.InvalidTopic:
                    got = None
                assert got == new and (got is None) == (cat == "invalid"), (name, row.kind, row.pos, j)
                assert mine["kind"] == det["kind"] and mine["n"] == det["n"] >= 3
                checked += 1
        valid = [j for j in range(ke.J) if j not in sv["invalid"]]
        js = [valid[0], min(valid, key=lambda j: abs(j - ke.SCAN)), valid[-1]]
        for j in js if name == "narrow" else js[1:2]:
            want_z, want_stats = ke.restatement_z(j)
            phi = ke.phi(j)
            z, stats = ke.z0.astype(np.int64), np.zeros(4, np.int64)
            R.z_step(ke.doc_ptr, ke.tokens, z, phi, SR.alias_tables(phi, KE.ALPHA), PS.word_lists(phi)[1], KE.SEED, KE.ITERATION, stats=stats)
            assert (z == want_z).all() and (stats == want_stats).all() and stats[R.ALIAS] == 0
        print("%s: %d draws of %d rows agree with polyaurn_sparse's" % (name, checked, len(ke.rows)))
    print("wall time %.1f s" % (time.time() - t0))


def test_rows_without_a_candidate_stand_on_the_alias_edge(oracle):
    for K in (8, 160):
        ae = NE.alias_fixture(K)
        sv = ae.survey()
        print("K=%d: %d one-token rows (%d aimed, %d plain), %d scan values; rows / scan values per category: %s" % (
            K, len(ae.rows), sum(r.kind == "aimed" for r in ae.rows), sum(r.kind == "plain" for r in ae.rows), ae.J,
            ", ".join("%s %d / %d" % (c, sv["rows"].get(c, 0), sv["values"].get(c, 0)) for c in NE.EDGE_CATS + ("far", "plain"))))
        for cat in NE.EDGE_CATS:
            assert sv["rows"].get(cat, 0) >= NE.MIN_PER_CATEGORY, (K, cat)
        assert sv["rows"].get("plain", 0) + sum(r.kind == "aimed" for r in ae.rows) == len(ae.rows)
        uniform_differs = ge_differs = 0
        for row, ev in zip(ae.rows, sv["evals"]):
            assert row.i == int(row.U * K) and row.frac == row.U * K - row.i
            for j, (cat, new, det) in enumerate(ev):
                ps_i, a_i = det["ps_i"], det["a_i"]
                assert a_i != row.i or ps_i == 1.0
                assert new == (a_i if row.frac > ps_i else row.i)
                # mutant 1: polyaurn's draw for a token without a candidate
                if PS.uniform_topic(row.U, K) != new:
                    uniform_differs += 1
                assert (PS.uniform_topic(row.U, K) != new) == (row.frac > ps_i and a_i != row.i)
                if cat == "above":
                    assert PS.uniform_topic(row.U, K) != new
                # mutant 2: >= in place of >: the ties and no others
                ge = a_i if row.frac >= ps_i else row.i
                assert (ge != new) == (cat == "tie"), (K, row.target, j, cat)
                ge_differs += ge != new
        assert uniform_differs >= sv["values"]["above"] > 0 and ge_differs == sv["values"]["tie"] > 0
        print("K=%d: floor(U K) is wrong at %d scan values, >= at the %d ties" % (K, uniform_differs, ge_differs))
        # whole steps: the targets draw what the rows expect, every other token stays, the counters know the branch
        targets = np.array([row.target for row in ae.rows])
        for j in (0, NE.SCAN, ae.J - 1):
            z, stats, trace = ae.restatement_z(j)
            assert (z[targets] == [ev[j][1] for ev in sv["evals"]]).all()
            kinds = {t["pos"]: (t["kind"], len(t["list"])) for t in trace}
            assert all(kinds[int(t)] == (R.ALIAS, 0) for t in targets)                 # nd == 0
            for pos in ae.zero_targets:                                                # nw == 0 < nd: the identity table's draw
                assert kinds[pos][0] == R.ALIAS and kinds[pos][1] > 0 and z[pos] == int(ae.U[pos] * K)
            rest = np.ones(z.size, bool)
            rest[targets] = False
            rest[ae.zero_targets] = False
            assert (z[rest] == ae.z0[rest]).all()
            assert stats[R.ALIAS] == len(ae.rows) + len(ae.zero_targets) and stats[R.DOC] == 0 and stats[R.WORD] == rest.sum()
