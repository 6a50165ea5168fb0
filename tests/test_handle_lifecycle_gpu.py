"""The host state of a handle with a history, for all eleven schemes (tests/handle_lifecycle.py, ROWS): a chain resumed on a
fresh handle from its exports, a handle rewound to an earlier state of itself, a handle reused for a second and a third
corpus, and a chain continued across shards -- each bit-equal, in everything the scheme exposes, to the uninterrupted
chain or a fresh handle, and to the oracle over the same script of calls.  What decides these cases is not a kernel but
the flags and buffers ggs_set_corpus, ggs_set_z, ggs_set_phi and ggs_set_iteration reset or leave (csrc/ggs_api.hip); the
sentences of include/ggs_hip.h on them ("A handle with a history") are each pinned by a test here."""
import re

import numpy as np
import pytest

from tests import handle_lifecycle as H
from tests.handle_lifecycle import ROWS, assert_bit_equal, assert_is_oracle, assert_same

pytestmark = pytest.mark.gpu

NAMES = [r.name for r in ROWS]
LANE, WAVE = "pcgs_sliced_kernel (lane per document)", "pcgs_wave_kernel (wave per document)"


def sweeps_collecting_phi(h, row, n, phis):
    """n whole sweeps, one call each, Phi read back after every one (the phi mean's addends)"""
    for _ in range(n):
        h.sweep(1)
        if row.mean != "none":
            phis[h.iteration] = h.get_phi()


def split_sweeps(h, n):
    for _ in range(n):
        h.sweep_begin()
        h.sweep_end()


def assert_phi_mean(snap, row, phis, n_before, tag):
    mean, n = H.expected_phi_mean(row, phis, n_before)
    assert snap["n_sampled"] == n, "%s: n_sampled %d, the rule gives %d" % (tag, snap["n_sampled"], n)
    assert ("phi_mean" in snap) == (mean is not None), tag
    if mean is not None:
        assert_bit_equal(snap["phi_mean"], mean, tag + ": phi mean")


def assert_preconditions(h, row, tag):
    """what the exported Phi must be like for the case to mean what it says"""
    if row.zeros_in_phi:
        assert H.zero_cells(h.get_phi()) > 0, tag + ": the Poisson Phi has exact zeros"
    if row.vs:
        und, zero, _ = h.vs_stats()
        assert 0 < und == zero, "%s: every zero cell of Phi is an undrawn one (%d undrawn, %d zero): no drawn cell holds 0.0" % (tag, und, zero)


# ---- 1. resume on a fresh handle ----------------------------------------------------------------------------------------
RESUME = [(n, K, "sweep", "sweep") for n in NAMES for K in H.KS]
RESUME += [(n, 8, "split", "mixed") for n in NAMES]                      # exported after sweep_begin + sweep_end; whole sweeps on one side, split on the other
RESUME += [(r.name, 8, "sweep", "zgiven") for r in ROWS if r.z_given_phi]
RESUME += [("ggs", 200, "split", "zgiven"), ("pcgs", 200, "split", "mixed")]


@pytest.mark.parametrize("name,K,first,then", RESUME)
def test_resume_on_a_fresh_handle(native, name, K, first, then):
    """Handle a runs 2 sweeps and exports what the helper's docstring lists for its scheme; handle b, of the same
    configuration, is given that; both go on for 2 more.  They and the oracle after the same 4 steps agree.  Corpus A has more
    documents than word types: for ggs at K = 8 the theta draw keeps the handle's stream (theta_main).  (The float32 rows of Phi
    have a case of their own below: every word of corpus A fits the hot table, and only cold chunks read them.)"""
    row, c = H.ROW[name], H.corpus("A")
    script = H.CANON if then != "zgiven" else (("sweep", 2), ("zgiven", 2))
    want = H.oracle_state(name, K, "A", script)
    a, b = H.create(native, row, K), None
    try:
        H.start(a, c, H.initial_z(c, K))
        pa, pb = {}, {}
        if first == "sweep":
            sweeps_collecting_phi(a, row, 2, pa)
        else:
            split_sweeps(a, 2)
            if row.mean != "none":
                pa[2] = a.get_phi()                                         # iteration 1 is within the burn-in
        assert_preconditions(a, row, name)
        state = H.export_state(a, row)
        assert state["iteration"] == 2
        b = H.create(native, row, K)
        b.set_corpus(c.doc_ptr, c.tokens)
        H.restore(b, row, state)
        if "phi" in state:
            assert_bit_equal(b.get_phi(), state["phi"], "set_phi / get_phi")
        if row.vs:                                                           # include/ggs_hip.h: after ggs_set_phi the cells with phi != 0.0
            nw, lists = b.word_topic_lists()
            assert_bit_equal(nw, (state["phi"] != 0.0).sum(axis=0).astype(np.int32), "nzvsspalias' lists after set_phi")
            assert_bit_equal(lists, a.word_topic_lists()[1], "the non-zero cells are the drawn cells")
        if then == "sweep":
            sweeps_collecting_phi(a, row, 2, pa)
            sweeps_collecting_phi(b, row, 2, pb)
        elif then == "mixed":
            sweeps_collecting_phi(a, row, 2, pa)
            split_sweeps(b, 2)
            pb = {k: v for k, v in pa.items() if k > 2}                      # b's own Phi are compared with a's below
        else:
            a.sample_z_given_phi(2)
            b.sample_z_given_phi(2)
        sa, sb = H.snapshot(a, row), H.snapshot(b, row)
        own = H.OWN + H.CUMULATIVE
        if row.vs and then == "zgiven":                                      # include/ggs_hip.h: no draw stands behind a Phi that was set, and b has drawn none since
            assert_bit_equal(sb.pop("vs_stats"), np.array([0, sa["vs_stats"][1], 0]), "vs_stats of a handle whose Phi was set")
            own += ("vs_stats",)
        assert_is_oracle(sa, want, name + " uninterrupted")
        assert_is_oracle(sb, want, name + " resumed")
        assert_same(sa, sb, name + " resumed against uninterrupted", skip=own)
        for k in H.CUMULATIVE:                                               # b counted its own 2 steps, a all 4
            if k in sa:
                assert int(sb[k][:3].sum()) == 2 * c.num_tokens and int(sa[k][:3].sum()) == 4 * c.num_tokens, k
        assert_phi_mean(sa, row, pa, 0, name + " uninterrupted")
        assert_phi_mean(sb, row, pb, 0, name + " resumed")
        a.check_invariants()
        b.check_invariants()
    finally:
        a.close()
        if b is not None:
            b.close()


@pytest.mark.parametrize("K,counted", [(8, False), (100, False), (100, True)])
def test_resume_and_rewind_where_cold_chunks_score_from_the_float32_rows(native, monkeypatch, capfd, K, counted):
    """The float32 shadow of Phi (d_phiT32) is read by one kernel only: scheme ggs at K <= 160, the cold chunks of the
    score-register z step -- the pcgs family scores from the fp64 rows.  With the small tables of H.HOT_ENV corpus HOT keeps 64 of
    its words cold, so the resumed handle's z step reads the float32 rows phi_to_phiT_kernel wrote from the Phi that was set where
    the uninterrupted handle reads those its sweep's repack wrote; then the first handle is rewound and runs the two sweeps again.
    That the float32 kernel is the one launched: GGS_DEBUG_PHI64 (the fp64 cold path of the same build) is unset, and the
    `counted` case runs the kernel's counting form (GGS_DEBUG_REPLAYS=1, as tests/test_phi32_gpu.py does), whose handles report
    their launches of z_sliced32_kernel when they are destroyed -- a report only a handle planned with the float32 path makes."""
    row, c = H.ROW["ggs"], H.corpus("HOT")
    want = H.oracle_state("ggs", K, "HOT")
    monkeypatch.delenv("GGS_DEBUG_PHI64", raising=False)
    env = dict(H.HOT_ENV, GGS_DEBUG_REPLAYS="1") if counted else H.HOT_ENV
    a = b = None
    try:
        with monkeypatch.context() as m:                     # the knobs are read when a handle is created
            for k, v in env.items():
                m.setenv(k, v)
            a = H.create(native, row, K)
            b = H.create(native, row, K)
        H.start(a, c, H.initial_z(c, K))
        a.sweep(2)
        info = a.launch_info()
        assert info["num_hot"] == 8 + 3 * 16 < H.shape_of(c)["distinct"] and info["z_kernel"].startswith("z_sliced_kernel"), info
        state = H.export_state(a, row)
        b.set_corpus(c.doc_ptr, c.tokens)
        H.restore(b, row, state)
        a.sweep(2)
        b.sweep(2)
        sa, sb = H.snapshot(a, row), H.snapshot(b, row)
        assert_is_oracle(sa, want, "uninterrupted")
        assert_is_oracle(sb, want, "resumed")
        assert_same(sa, sb, "resumed against uninterrupted", skip=H.OWN)
        H.restore(a, row, state, ("phi", "iteration", "z"))
        a.sweep(2)
        assert_same(H.snapshot(a, row), sa, "rewound against its first pass", skip=H.OWN)
    finally:
        for h in (a, b):
            if h is not None:
                h.close()
    if counted:
        launches = [int(n) for n in re.findall(r"\[ggs\] z replays: \d+ tokens in (\d+) launches of z_sliced32_kernel", capfd.readouterr().err)]
        assert len(launches) == 2 and launches[0] >= 6 and launches[1] >= 2, launches     # a: 4 sweeps and 2 after the rewind; b: 2


def test_nzvsspalias_lists_after_set_phi_when_a_drawn_cell_is_zero(native):
    """include/ggs_hip.h: after a sweep the lists are the DRAWN cells, after ggs_set_phi the cells with phi != 0.0.  With
    beta = 0.001 a gamma draw of a cell without tokens underflows to 0.0 about every other time, so the two differ: the resumed
    handle's lists are exactly the non-zero cells and a subset of the exporting handle's.  (The chains may then part: the lists
    decide which walk a token takes.  That is the header's rule, not pinned further.)"""
    import dataclasses
    row = dataclasses.replace(H.ROW["nzvsspalias"], beta=0.001)
    c, K = H.corpus("A"), 8
    a, b = H.create(native, row, K), None
    try:
        H.start(a, c, H.initial_z(c, K))
        a.sweep(2)
        und, zero, _ = a.vs_stats()
        assert zero > und > 0, "some drawn cell holds 0.0"
        state = H.export_state(a, row)
        b = H.create(native, row, K)
        b.set_corpus(c.doc_ptr, c.tokens)
        H.restore(b, row, state)
        (nwa, la), (nwb, lb) = a.word_topic_lists(), b.word_topic_lists()
        nonzero = state["phi"] != 0.0
        assert_bit_equal(nwb, nonzero.sum(axis=0).astype(np.int32), "nw after set_phi")
        assert int(nwa.sum()) == K * H.V - und and int(nwb.sum()) == K * H.V - zero
        for w in range(H.V):
            assert lb[w, :nwb[w]].tolist() == np.flatnonzero(nonzero[:, w]).tolist()
            assert set(lb[w, :nwb[w]].tolist()) <= set(la[w, :nwa[w]].tolist())
        assert_bit_equal(b.vs_stats(), np.array([0, zero, 0]), "no draw stands behind a Phi that was set")
        b.sweep(1)
        b.check_invariants()
    finally:
        a.close()
        if b is not None:
            b.close()


# ---- 2. rewind on the same handle ---------------------------------------------------------------------------------------
def rewind_orders(row, K):
    """K = 8: every order of the row's setters (six, two for the count form).  K = 200 picks other kernels, not other setters:
    one order, the reverse of the listed one."""
    o = H.orders(row)
    return o if K == 8 else [o[-1]]


@pytest.mark.parametrize("name,K,order", [(r.name, K, "-".join(o)) for r in ROWS for K in H.KS for o in rewind_orders(r, K)])
def test_rewind_on_the_same_handle(native, name, K, order):
    """One sweep, save (z, Phi, iteration), three more; the saved state put back with the setters in `order` (rewind_orders: each
    of their orders at K = 8); three more.
    Behind the rewind stand a theta drawn ahead for iteration 5, the tables and lists of the Phi of iteration 4, counters that
    went on and a phi mean in progress.  Everything equals the first pass; the cumulative counters grew by the same amounts;
    the phi mean follows ggs_set_phi's rule: the sum restarts, n_sampled keeps counting."""
    row, c = H.ROW[name], H.corpus("A")
    want = H.oracle_state(name, K, "A")
    g = H.create(native, row, K)
    try:
        H.start(g, c, H.initial_z(c, K))
        p1, p2 = {}, {}
        sweeps_collecting_phi(g, row, 1, p1)
        saved = H.export_state(g, row)
        c1 = {k: v for k, v in H.snapshot(g, row).items() if k in H.CUMULATIVE}
        sweeps_collecting_phi(g, row, 3, p1)
        s1 = H.snapshot(g, row)
        assert_is_oracle(s1, want, name + " first pass")
        assert_phi_mean(s1, row, p1, 0, name + " first pass")
        H.restore(g, row, saved, order.split("-"))
        assert g.iteration == 1
        sweeps_collecting_phi(g, row, 3, p2)
        s2 = H.snapshot(g, row)
        assert_is_oracle(s2, want, name + " second pass")
        assert_same(s1, s2, name + " second pass against the first", skip=H.OWN + H.CUMULATIVE)
        for k in c1:                                                         # cumulative since ggs_set_corpus: differences
            assert_bit_equal(s2[k] - s1[k], s1[k] - c1[k], "%s: what the three sweeps added to %s" % (name, k))
        # only ggs_set_phi restarts the running sum: the count form and its rows never accept a Phi
        assert_phi_mean(s2, row, p2, s1["n_sampled"], name + " second pass")
        g.check_invariants()
    finally:
        g.close()


@pytest.mark.parametrize("name,K", [(n, 8) for n in NAMES] + [("ggs", 200), ("pcgs", 200), ("collapsed", 200)])
def test_set_iteration_alone(native, name, K):
    """ggs_set_iteration with no ggs_set_z (and, one sweep later, ggs_set_z of the z the handle has): to the number the handle already has (a theta drawn ahead for the next iteration
    exists and is the right one: the chain is the uninterrupted one), then to another number (that theta is for an iteration
    that will not come: it is not used, and the sweep is the oracle's at the new number)."""
    row, c = H.ROW[name], H.corpus("A")
    jump = (("sweep", 4), ("iteration", 9), ("sweep", 1))
    g = H.create(native, row, K)
    try:
        H.start(g, c, H.initial_z(c, K))
        phis = {}
        sweeps_collecting_phi(g, row, 2, phis)
        g.set_iteration(2)
        sweeps_collecting_phi(g, row, 1, phis)
        g.set_z(g.get_z(), redraw_phi=False)              # the z it has: the chain goes on, and like ggs_set_iteration it leaves the phi mean alone
        if row.form == "count":
            g.init_phi()
        sweeps_collecting_phi(g, row, 1, phis)
        s = H.snapshot(g, row)
        assert_is_oracle(s, H.oracle_state(name, K, "A"), name + " set_iteration to the same number")
        assert_phi_mean(s, row, phis, 0, name + ": neither ggs_set_iteration nor ggs_set_z touches the phi mean")
        g.set_iteration(9)
        g.sweep(1)
        s = H.snapshot(g, row)
        assert s["iteration"] == 10
        assert_is_oracle(s, H.oracle_state(name, K, "A", jump), name + " set_iteration to another number")
        g.check_invariants()
    finally:
        g.close()


@pytest.mark.parametrize("name,K,order", [(r.name, 8, "-".join(o)) for r in ROWS for o in (H.orders(r)[0], H.orders(r)[-1])] +
                         [("ggs", 200, "iteration-phi-z"), ("ggs", 200, "z-phi-iteration")])
def test_another_state_at_the_iteration_number_the_handle_is_at(native, name, K, order):
    """The one case where a stale theta has the right label: after 4 sweeps a theta for iteration 5 stands ready, drawn from the z
    of iteration 4.  The handle is then given the z and Phi of iteration 1 and the iteration number 4 again: the next sweep is
    iteration 5 and must draw its theta from the z that was set (ggs_set_z drops the one drawn ahead, whether it is the first
    setter called or the last: the listed order and its reverse).  The oracle runs the same script; for the other schemes the tables, lists and counts behind the setters are as stale."""
    row, c = H.ROW[name], H.corpus("A")
    g = H.create(native, row, K)
    try:
        H.start(g, c, H.initial_z(c, K))
        g.sweep(1)
        saved = H.export_state(g, row)
        g.sweep(3)
        H.restore(g, row, dict(saved, iteration=4), order.split("-"))
        g.sweep(1)
        s = H.snapshot(g, row)
        assert s["iteration"] == 5
        assert_is_oracle(s, H.oracle_state(name, K, "A", (("sweep", 1), ("iteration", 4), ("sweep", 1))), name)
        g.check_invariants()
    finally:
        g.close()


@pytest.mark.parametrize("K", H.KS)
def test_init_z_java_lcg_drops_the_theta_drawn_ahead(native, K):
    """include/ggs_hip.h: ggs_init_z_java_lcg drops a theta drawn ahead, as ggs_set_z does.  After 2 sweeps of ggs a theta for
    iteration 3 stands ready, drawn from the z of iteration 2; a new seeded z leaves the iteration number at 2, so the next sweep is
    the very iteration that theta was drawn for and must draw its own from the new z.  Phi stays the one of iteration 2."""
    row, c = H.ROW["ggs"], H.corpus("A")
    g = H.create(native, row, K)
    try:
        H.start(g, c, H.initial_z(c, K))
        g.sweep(2)
        g.init_z_java_lcg(H.ZSEED + 1)
        assert g.iteration == 2
        assert_bit_equal(g.get_z(), H.initial_z(c, K, H.ZSEED + 1), "the new seeded z")
        g.sweep(1)
        assert_is_oracle(H.snapshot(g, row), H.oracle_state("ggs", K, "A", (("sweep", 2), ("initz", H.ZSEED + 1), ("sweep", 1))), "ggs")
        g.check_invariants()
    finally:
        g.close()


def test_collapsed_serial_sweep_after_a_rewind(native, oracle):
    """include/ggs_hip.h: after ggs_set_z a new Random(java_seed) is created at the first serial sweep -- also on a handle whose
    seeded start and earlier serial sweeps left a stream behind."""
    row, c, K = H.ROW["collapsed"], H.corpus("A"), 8
    g = H.create(native, row, K)
    try:
        g.set_corpus(c.doc_ptr, c.tokens)
        g.init_z_java_lcg(H.ZSEED)                       # the handle owns a stream now
        g.init_phi()
        g.collapsed_serial_sweep(H.ZSEED, 1)
        saved = H.export_state(g, row)
        g.sweep(2)
        g.collapsed_serial_sweep(H.ZSEED, 1)
        H.restore(g, row, saved)
        g.collapsed_serial_sweep(123, 2)
        o = oracle.OracleSampler(K, H.V, H.ALPHA, row.beta, H.SEED)
        o.set_corpus(c.doc_ptr, c.tokens)
        o.set_z(saved["z"], redraw_phi=False)
        o.collapsed_sweep(123, 2)
        assert_bit_equal(g.get_z(), o.get_z(), "z of the serial chain after the rewind")
        assert_bit_equal(g.get_type_topic_counts(), o.get_type_topic_counts(), "n_wk")
        assert_bit_equal(g.get_topic_totals(), o.get_topic_totals(), "n_k")
        assert g.iteration == 3
    finally:
        g.close()


# ---- 3. reuse: a second and a third corpus --------------------------------------------------------------------------------
def other_corpus(row, K):
    """the pcgs z step proper at K = 8 goes lane -> wave -> lane over a document of 33 000 tokens"""
    return "LONG" if K == 8 and row.name in ("pcgs", "collapsed", "polyaurn") else "B"


def geometry(info):
    """launch_info() without what the first z step's TIMING decides (ggs at K <= 160: split or fused)"""
    return {k: v for k, v in info.items() if k != "z_form"}


def run_corpus(h, row, c, K, sweeps, iteration=None):
    h.set_corpus(c.doc_ptr, c.tokens)
    if iteration is not None:
        h.set_iteration(iteration)
    h.set_z(H.initial_z(c, K), redraw_phi=False)
    h.init_phi()
    phis = {}
    sweeps_collecting_phi(h, row, sweeps, phis)
    h.check_invariants()
    return H.snapshot(h, row), phis, h.launch_info()


@pytest.mark.parametrize("K", H.KS)
@pytest.mark.parametrize("name", NAMES)
def test_reuse_for_a_second_and_a_third_corpus(native, name, K):
    """Handle g runs corpus A, then another corpus, then A again; every run equals a fresh handle's on that corpus and the
    oracle's, in everything -- the counters and the phi mean included, which start again at ggs_set_corpus.  The iteration number
    is the caller's: it carries over a ggs_set_corpus (the second run starts at 4, and so do its fresh comparator and the
    oracle), and the third run sets it back to 0."""
    row = H.ROW[name]
    other = other_corpus(row, K)
    A, B = H.corpus("A"), H.corpus(other)
    nb = 1 if other == "LONG" else 2
    g, f = H.create(native, row, K), None
    try:
        s1, p1, i1 = run_corpus(g, row, A, K, 4)
        assert_is_oracle(s1, H.oracle_state(name, K, "A"), name + " first corpus")
        assert_phi_mean(s1, row, p1, 0, name + " first corpus")
        if row.priors:
            priors = g.get_topic_priors()
            assert H.zero_cells(priors) == 6
        g.set_corpus(B.doc_ptr, B.tokens)
        assert g.iteration == 4, "ggs_set_corpus leaves the iteration number"
        assert g.get_phi_mean() == (None, 0), "ggs_set_corpus starts the phi mean again"
        if row.priors:                                   # the priors are the handle's, not the corpus': they stay, and may be replaced while there is no Phi
            assert_bit_equal(g.get_topic_priors(), priors, "priors after a second ggs_set_corpus")
            g.set_topic_priors(*H.prior_cells(K))
        s2, p2, i2 = run_corpus(g, row, B, K, nb)
        if row.priors:
            with pytest.raises(native.GGSError) as e:
                g.set_topic_priors(*H.prior_cells(K))
            assert e.value.code == native.ERR_STATE      # the handle has a Phi again
        f = H.create(native, row, K)
        sf, pf, jf = run_corpus(f, row, B, K, nb, iteration=4)
        assert_same(s2, sf, name + " second corpus against a fresh handle")
        assert_is_oracle(s2, H.oracle_state(name, K, other, (("sweep", nb),), 4), name + " second corpus")
        assert_phi_mean(s2, row, p2, 0, name + " second corpus")
        assert geometry(i2) == geometry(jf), "launch_info of the second corpus"
        if other == "LONG":
            assert i1["z_kernel"].startswith(LANE) and i2["z_kernel"].startswith(WAVE)
        if row.name in ("spalias", "spalias_priors", "polyaurn_sparse"):   # their lists are sized by the longest document
            assert i1["lds_bytes_z"] != i2["lds_bytes_z"] or K == 8
        s3, p3, i3 = run_corpus(g, row, A, K, 4, iteration=0)
        assert_same(s3, s1, name + " third corpus against the first run")
        assert_phi_mean(s3, row, p3, 0, name + " third corpus")
        assert geometry(i3) == geometry(i1), "launch_info of the third corpus"
    finally:
        g.close()
        if f is not None:
            f.close()


def test_reuse_ggs_across_hot_word_sets_and_warm_tiers(native, monkeypatch):
    """ggs at K <= 160 with small tables (H.HOT_ENV): corpus HOT has 8 hot words, warm tiers and cold words behind them, so its
    first z step times the split and the fused form; corpus FEW has 8 words in all -- every chunk is a hot chunk, there is
    nothing to split and no tier; then HOT again: the split is tried anew and the tables are HOT's."""
    row, K = H.ROW["ggs"], 8
    g = f = None
    try:
        with monkeypatch.context() as m:                     # the knobs are read when a handle is created
            for k, v in H.HOT_ENV.items():
                m.setenv(k, v)
            g = H.create(native, row, K)
            f = H.create(native, row, K)
        hot, few = H.corpus("HOT"), H.corpus("FEW")
        s1, _, i1 = run_corpus(g, row, hot, K, 3)
        assert i1["num_hot"] == 8 + 3 * 16 and i1["warm_tiers"] == 3 and i1["z_form_calibrated"], i1
        assert_is_oracle(s1, H.oracle_state("ggs", K, "HOT", (("sweep", 3),)), "HOT")
        s2, _, i2 = run_corpus(g, row, few, K, 3)
        assert i2["num_hot"] == 8 and i2["warm_tiers"] == 0 and not i2["z_form_calibrated"], i2
        assert_is_oracle(s2, H.oracle_state("ggs", K, "FEW", (("sweep", 3),), 3), "FEW")
        sf, _, jf = run_corpus(f, row, few, K, 3, iteration=3)
        assert_same(s2, sf, "FEW against a fresh handle")
        assert geometry(i2) == geometry(jf)
        s3, _, i3 = run_corpus(g, row, hot, K, 3, iteration=0)
        assert i3["z_form_calibrated"] and (i3["num_hot"], i3["warm_tiers"], i3["num_warm"]) == (i1["num_hot"], i1["warm_tiers"], i1["num_warm"])
        assert_same(s3, s1, "HOT again against the first run")
    finally:
        for h in (g, f):
            if h is not None:
                h.close()


def test_reuse_ggs_across_z_parts(native):
    """ggs at K = 200: corpus PARTS is cut into eight z parts (the next theta of a part drawn beside the following parts),
    corpus B is one part, then PARTS again."""
    row, K = H.ROW["ggs"], 200
    g, f = H.create(native, row, K), None
    try:
        parts, one = H.corpus("PARTS"), H.corpus("B")
        s1, _, i1 = run_corpus(g, row, parts, K, 3)
        assert i1["z_parts"] == 8, i1
        assert_is_oracle(s1, H.oracle_state("ggs", K, "PARTS", (("sweep", 3),)), "PARTS")
        s2, _, i2 = run_corpus(g, row, one, K, 3)
        assert i2["z_parts"] == 1, i2
        assert_is_oracle(s2, H.oracle_state("ggs", K, "B", (("sweep", 3),), 3), "B")
        f = H.create(native, row, K)
        sf, _, _ = run_corpus(f, row, one, K, 3, iteration=3)
        assert_same(s2, sf, "B against a fresh handle")
        s3, _, i3 = run_corpus(g, row, parts, K, 3, iteration=0)
        assert i3["z_parts"] == 8
        assert_same(s3, s1, "PARTS again against the first run")
    finally:
        g.close()
        if f is not None:
            f.close()


# ---- 4. resume across shards ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "sparse"])
@pytest.mark.parametrize("name", NAMES)
def test_resume_across_shards(native, name, mode):
    """One handle runs 2 sweeps and exports; a world of 2 ranks -- each given its slice of z, the whole Phi and the iteration
    number, with the exchange already attached -- runs 2 more.  And the converse: a world of 2 runs 2 sweeps from the start,
    exports, and one handle runs 2 more.  Both equal the uninterrupted one-handle chain after 4 sweeps.  K = 9: topic slices of
    5 and 4.  A Phi that was SET while an exchange is attached: the counts of the rank are then its own, not a sweep's merge."""
    row, c, K, world = H.ROW[name], H.corpus("A"), 9, 2
    z0 = H.initial_z(c, K)
    u = H.create(native, row, K)
    try:
        H.start(u, c, z0)
        u.sweep(2)
        half = H.export_state(u, row)
        u.sweep(2)
        whole = H.snapshot(u, row)
    finally:
        u.close()

    def resumed(h, rank, sub, tok_base):
        H.restore(h, row, half, z_slice=slice(tok_base, tok_base + sub.num_tokens))
        h.sweep(2)
        h.check_invariants()
        return H.snapshot(h, row)

    def from_the_start(h, rank, sub, tok_base):
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=False)
        h.init_phi()
        h.sweep(2)
        return H.export_state(h, row)

    per_rank = ("z", "theta", "log_posterior", "model_log_likelihood") + H.OWN + H.CUMULATIVE + ("vs_stats",)
    out = H.run_world(native, row, K, c, world, mode, resumed)
    assert_bit_equal(np.concatenate([o["z"] for o in out]), whole["z"], name + ": z of the ranks")
    if row.theta:
        assert_bit_equal(np.concatenate([o["theta"] for o in out]), whole["theta"], name + ": theta of the ranks")
    # The likelihoods: the topic side is computed from what every rank holds whole (the gathered counts, Phi), in the same fixed
    # tree: bit-equal to one handle's on every rank.  The document side covers a rank's own documents (include/ggs_hip.h: the model's
    # value is the SUM of the shards' document sides): two trees over 80 documents each and two D * lgS(alphaSum) terms round
    # differently from one tree over 160, so there is no bit equality to ask for there.
    for k in ("model_log_likelihood", "log_posterior"):
        if k in whole:
            for r, o in enumerate(out):
                assert_bit_equal(o[k][1:], whole[k][1:], "%s rank %d: topic side of %s" % (name, r, k))
    for r, o in enumerate(out):                          # Phi, the corpus-wide counts, tables and lists are replicated
        assert_same(o, whole, "%s rank %d of the resumed world" % (name, r), skip=per_rank)
    for k in H.CUMULATIVE:                               # the ranks' 2 sweeps over their shards add up to 2 sweeps of the corpus
        if k in whole:
            assert int(sum(o[k][:3].sum() for o in out)) == 2 * c.num_tokens, k
    if row.vs:                                           # undrawn and zero cells cover all topics on every rank
        for o in out:
            assert_bit_equal(o["vs_stats"][:2], whole["vs_stats"][:2], "vs_stats of a rank")

    exports = H.run_world(native, row, K, c, world, mode, from_the_start)
    state = {"z": np.concatenate([e["z"] for e in exports]), "iteration": exports[0]["iteration"]}
    if "phi" in row.exports:
        state["phi"] = exports[0]["phi"]
        assert_bit_equal(exports[1]["phi"], state["phi"], "Phi is replicated")
        assert_bit_equal(state["phi"], half["phi"], "Phi of the world after 2 sweeps")
    assert_bit_equal(state["z"], half["z"], "z of the world after 2 sweeps")
    v = H.create(native, row, K)
    try:
        v.set_corpus(c.doc_ptr, c.tokens)
        H.restore(v, row, state)
        v.sweep(2)
        v.check_invariants()
        assert_same(H.snapshot(v, row), whole, name + ": one handle continuing the world's chain", skip=H.OWN + H.CUMULATIVE)
    finally:
        v.close()
