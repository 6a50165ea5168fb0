"""The pure parts of tests/handle_lifecycle.py, without a device: the scheme rows against the recorded capabilities, the corpus
builders with the properties the device tests rely on, the exported-state table, the phi mean's rule against the oracle's own
bookkeeping, and -- through the oracle, where it restates the scheme -- the preconditions of the resume cases and the resume
itself: an oracle fed the exports of another continues as the uninterrupted one does."""
import numpy as np
import pytest

from tests import handle_lifecycle as H
from tests import scheme_table_cases as T


def test_rows_are_the_scheme_table_plus_priors():
    from ldagroupedgibbssampler_amd import native
    assert [r.name for r in H.ROWS if not r.priors] == list(native.SCHEME_FLAGS)
    assert [r.name for r in H.ROWS if r.priors] == ["spalias_priors"] and H.ROW["spalias_priors"].scheme == "spalias"
    assert len(H.ROWS) == 11
    caps = T.golden("scheme_capabilities.json")
    for r in H.ROWS:
        c = caps[r.scheme]
        assert r.tables == (c["ggs_get_alias_tables"] == native.OK), r.name
        assert r.lists == (c["ggs_get_word_topic_lists"] == native.OK), r.name
        assert r.mh == (c["ggs_get_mh_stats"] == native.OK), r.name
        assert r.sparse == (c["ggs_get_sparse_stats"] == native.OK), r.name
        assert r.vs == (c["ggs_get_vs_stats"] == native.OK), r.name
        assert c["ggs_get_phi"] == native.OK
        if r.theta:
            assert c["ggs_get_theta"] == native.OK


def test_exported_state_per_scheme():
    for r in H.ROWS:
        assert r.exports == (("z", "iteration") if r.form == "count" else ("z", "phi", "iteration")), r.name
        assert r.z_given_phi == (r.form != "count")
        assert (r.mean == "none") == (r.form == "count"), r.name
        assert r.name in H.__doc__
        orders = H.orders(r)
        assert len(orders) == (2 if r.form == "count" else 6) and len(set(orders)) == len(orders)
    assert [r.name for r in H.ROWS if r.form == "count"] == ["collapsed", "lightcollapsed", "adlda"]
    assert [r.name for r in H.ROWS if r.zeros_in_phi] == ["polyaurn", "polyaurn_sparse"]
    assert H.ROW["nzvsspalias"].mean == "zero" and H.ROW["nzvsspalias"].beta == 0.5 and H.VS_PI != 0.5
    t, w = H.prior_cells(8)
    assert len(t) == len(w) == 6 and len(set(zip(t.tolist(), w.tolist()))) == 6
    for K in H.KS + (9,):
        t, w = H.prior_cells(K)
        assert t.max() == K - 1 and np.bincount(w).max() < K and np.bincount(t).max() < H.V


def test_corpora_have_the_properties_the_device_tests_rely_on():
    shapes = {n: H.shape_of(H.corpus(n)) for n in ("A", "B", "LONG", "PARTS", "HOT", "FEW")}       # the builders assert their own
    for n, s in shapes.items():
        c = H.corpus(n)
        assert c.num_types == H.V and c.tokens.max() < H.V and s["empty"] > 0, n
        assert s["N"] < 40000, n
    a = shapes["A"]
    assert a["D"] > H.V                                   # ggs, K <= 160: the theta_main / chain_main legs
    assert a["D"] > 128                                   # three groups of 64 documents for the lane-per-document kernels
    assert shapes["B"]["longest"] > 200 > a["longest"]    # the spalias / polyaurn_sparse lists: min(K, longest) differs at K = 200
    assert shapes["LONG"]["longest"] > 32767
    assert shapes["PARTS"]["D"] >= 2 * H.V and shapes["PARTS"]["D"] >= 512 and shapes["B"]["D"] <= H.V
    assert shapes["FEW"]["distinct"] == int(H.HOT_ENV["GGS_DEBUG_HOT"])
    assert H.corpus("A") is H.corpus("A")
    with pytest.raises(ValueError):
        H.corpus("A").tokens[0] = 1                       # shared: read-only
    z = H.initial_z(H.corpus("A"), 8)
    assert z.shape == (a["N"],) and z.min() == 0 and z.max() == 7
    n = H.counts_of(H.corpus("A"), z, 8)
    assert n.sum() == a["N"] and n.shape == (H.V, 8)
    assert H.point_estimate(n, 0.05).shape == (8, H.V)
    np.testing.assert_allclose(H.point_estimate(n, 0.05).sum(axis=1), 1.0, rtol=1e-12)


def test_shards_cover_the_corpus():
    c = H.corpus("A")
    subs = [H.shard_of(c, r, 2) for r in range(2)]
    assert subs[0][2] == 0 and subs[1][2] == subs[0][0].num_tokens and sum(s.num_tokens for s, _, _ in subs) == c.num_tokens
    assert np.array_equal(np.concatenate([s.tokens for s, _, _ in subs]), c.tokens)


def test_phi_mean_rule_is_the_oracle_s(oracle):
    """expected_phi_mean against orc_get_phi_mean: an uninterrupted chain, and one whose Phi is set halfway (the sum restarts,
    the count goes on)."""
    row, c, K = H.ROW["ggs"], H.corpus("B"), 5
    assert [it for it in range(1, 8) if H.accepted(it)] == [2, 4, 6] and not H.accepted(4, burn_in=0) and not H.accepted(4, burn_in=4)
    o = oracle.OracleSampler(K, H.V, H.ALPHA, row.beta, H.SEED)
    o.set_phi_mean_gating(True, H.BURN_IN, H.THIN)
    o.set_corpus(c.doc_ptr, c.tokens)
    o.set_z(H.initial_z(c, K), redraw_phi=True)
    assert H.expected_phi_mean(row, {}) == (None, 0)
    phis = {}
    for _ in range(5):
        o.sweep(1)
        phis[o.iteration] = o.get_phi()
    mean, n = H.expected_phi_mean(row, phis)
    om, on = o.get_phi_mean()
    assert n == on == 2
    H.assert_bit_equal(mean, om, "phi mean")
    o.set_phi(o.get_phi())
    later = {}
    for _ in range(3):
        o.sweep(1)
        later[o.iteration] = o.get_phi()
    mean, n = H.expected_phi_mean(row, later, n_before=2)
    om, on = o.get_phi_mean()
    assert n == on == 4
    H.assert_bit_equal(mean, om, "phi mean after set_phi")
    H.assert_bit_equal(mean, (later[6] + later[8]) / 4.0, "the two Phi accepted since, over all four")
    zero, n = H.expected_phi_mean(H.ROW["nzvsspalias"], later, n_before=2)
    assert n == 4 and not zero.any()
    assert H.expected_phi_mean(H.ROW["adlda"], later) == (None, 0)


@pytest.mark.parametrize("name", [r.name for r in H.ROWS])
def test_oracle_resumes_as_it_runs_on(name):
    """The oracle of every row: 2 sweeps, export, a second oracle given the exports, 2 more on both -- the same state, which is
    also the shared state the device tests compare with.  On the way: the preconditions of the device's resume cases."""
    row, c, K = H.ROW[name], H.corpus("A"), 8
    z0 = H.initial_z(c, K)
    a = H.Chain(row, K, c, z0).run((("sweep", 2),))
    half = a.state()
    if row.zeros_in_phi:
        assert H.zero_cells(half["phi"]) > 0
    if row.vs:
        und, zero = half["vs_first_two"]
        assert 0 < und == zero                            # beta = 0.5: no drawn cell underflowed to 0.0
    if row.priors:
        t, w = H.prior_cells(K)
        assert not half["phi"][t, w].any() and H.zero_cells(half["phi"]) == 6
    b = H.Chain(row, K, c, half["z"], iteration=2)        # its initial Phi is replaced below; the count form has none
    if row.form != "count":
        if row.oracle == "c":
            b.o.set_phi(half["phi"])
        elif hasattr(b.m, "set_phi"):
            b.m.set_phi(half["phi"])
        else:
            b.m.phi = half["phi"].copy()                  # the polyaurn model keeps nothing else of a Phi
    a.run((("sweep", 2),))
    b.run((("sweep", 2),))
    sa, sb, want = a.state(), b.state(), H.oracle_state(name, K, "A")
    assert sa["iteration"] == sb["iteration"] == want["iteration"] == 4
    for k in ("z", "n_wk", "n_k", "phi", "theta", "vs_first_two"):
        if k in want:
            H.assert_bit_equal(sa[k], want[k], "%s uninterrupted: %s" % (name, k))
            H.assert_bit_equal(sb[k], want[k], "%s resumed: %s" % (name, k))
    assert (sa["z"] != z0).mean() > 0.25


def test_oracle_scripts():
    """the steps a script may hold, on the C oracle: whole sweeps, z given Phi, a jump of the iteration number"""
    c, K = H.corpus("B"), 8
    s = H.oracle_state("pcgs", K, "B", (("sweep", 1), ("zgiven", 2)))
    t = H.oracle_state("pcgs", K, "B", (("sweep", 1),))
    H.assert_bit_equal(s["phi"], t["phi"], "z given Phi leaves Phi")
    assert s["iteration"] == 3 and (s["z"] != t["z"]).any()
    j = H.oracle_state("ggs", K, "B", (("sweep", 1), ("iteration", 9), ("sweep", 1)))
    assert j["iteration"] == 10 and j["theta"].shape == (c.num_docs, K)
    assert H.oracle_state("ggs", K, "B", (("sweep", 1),), 4)["iteration"] == 5
    i = H.oracle_state("ggs", K, "B", (("sweep", 1), ("initz", 5), ("sweep", 1)))
    assert i["iteration"] == 2 and (i["z"] != H.oracle_state("ggs", K, "B", (("sweep", 2),))["z"]).any()
    assert not s["z"].flags.writeable


def test_snapshot_comparators():
    a = {"z": np.arange(4), "phi": np.array([0.0, 1.0]), "n_sampled": 2}
    H.assert_same(a, dict(a), "same")
    with pytest.raises(AssertionError):
        H.assert_same(a, dict(a, phi=np.array([-0.0, 1.0])), "the sign of zero is a bit")
    with pytest.raises(AssertionError):
        H.assert_same(a, {k: v for k, v in a.items() if k != "phi"}, "a missing name")
    H.assert_same(a, dict(a, n_sampled=3), "skipped", skip=H.OWN)
    with pytest.raises(AssertionError):
        H.assert_is_oracle(a, {"z": np.arange(4)[::-1]}, "oracle")
