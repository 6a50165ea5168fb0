"""scheme=nzvsspalias on the device (GGS_FLAG_NZVSSPALIAS), bit for bit against the CPU restatement (tests/nzvs_restatement.py):
StrictMath.exp, the indicator chain on its own (the LDS path and the global-scratch path, Philox and explicit uniforms on the
edges of p(s)), whole sweeps -- z, Phi, counts, alias tables, the words' lists, the counters -- the z step given a Phi, the phi
mean, misuse, the launch plan.

The z kernel is nzvs_wave_kernel (sparse_wave_body with the alias draw for a token without a candidate): the wave scans'
proposal, and the exact chain that replays what it leaves open.  GGS_DEBUG_MARGIN=1e30 (FORMS) sends every token with
candidates through the replay; both ways give the same bits."""

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import nzvs_restatement as R
from tests import polyaurn_sparse_restatement as PS
from tests.ranks import assert_bit_equal, force_form, run_ranks

pytestmark = pytest.mark.gpu

SEED = 777
BETA = 0.01
KERNEL = "nzvs_wave_kernel (wave per document)"
FORMS = [None, "1e30"]                  # GGS_DEBUG_MARGIN: the proposal with its margins / every token replayed exactly
PATHS = ["lds", "global"]               # the chain's rows in LDS / in global scratch (GGS_DEBUG_VS_GLOBAL=1)


def force_path(monkeypatch, path):
    monkeypatch.setenv("GGS_DEBUG", "1")
    if path == "global":
        monkeypatch.setenv("GGS_DEBUG_VS_GLOBAL", "1")
    else:
        monkeypatch.delenv("GGS_DEBUG_VS_GLOBAL", raising=False)


# ---- exp ------------------------------------------------------------------------------------------------------------
def test_strict_exp_equals_the_restatement(native):
    x = R.exp_grid()
    got = native.debug_math("exp", x)
    want = np.array([R.strict_exp(v) for v in x])
    nan = np.isnan(want)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got), nan)
    assert_bit_equal(got[~nan], want[~nan], "strict_exp")


# ---- the indicator chain on its own ---------------------------------------------------------------------------------
KMAX = 70                                                           # 33 crosses a mask word, 70 a wave
_refs = {}


def chain_inputs(V, pi, half_zero):
    """counts, prev_phi [70][V] and the sequential chain of every topic under the Philox uniforms: computed once per shape and
    shared by the smaller K (a topic's uniforms are those of the elements k * V + v, whatever K is) and by both paths"""
    key = (V, pi, half_zero)
    if key not in _refs:
        from oracle import oracle as O
        rng = np.random.default_rng(V * 7 + half_zero)
        counts = np.where(rng.random((KMAX, V)) < 0.8, 0, rng.integers(1, 40, (KMAX, V))).astype(np.int32)
        prev = rng.random((KMAX, V)) + 1e-3
        if half_zero:
            prev[rng.random((KMAX, V)) < 0.5] = 0.0
        counts[1] = 0                                               # a topic without tokens: n_k == 0
        U = O.uniforms(SEED, 3, R.PURPOSE_VS, 0, KMAX * V).reshape(KMAX, V)
        ref = [R.sequential_chain(counts[k], prev[k], U[k], BETA, pi) for k in range(KMAX)]
        _refs[key] = (counts, prev, np.array([r[0] for r in ref]), np.array([r[1] for r in ref], np.int32))
    return _refs[key]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("V", [1, 63, 64, 65, 1000, 4097])
def test_indicators_equal_the_sequential_chain(native, oracle, monkeypatch, V, path):
    force_path(monkeypatch, path)
    most = 0
    for pi in (0.5, 0.01):
        for half_zero in (True, False):
            counts, prev, drawn, s_end = chain_inputs(V, pi, half_zero)
            for K in (1, 3, 33, 70):
                d, s, rounds = native.debug_vs_indicators(counts[:K], prev[:K], BETA, pi, SEED, 3)
                what = "V=%d K=%d pi=%g %s" % (V, K, pi, "half zeros" if half_zero else "no zeros")
                assert_bit_equal(d, drawn[:K], "drawn set, " + what)
                assert_bit_equal(s, s_end[:K], "s at the row's end, " + what)
                assert (rounds >= 1).all() and (rounds <= (counts[:K] == 0).sum(axis=1) + 1).all(), what
                most = max(most, int(rounds.max()))
    print("V=%d %s: at most %d rounds" % (V, path, most))


@pytest.mark.parametrize("path", PATHS)
def test_indicators_on_the_edge_rows(native, oracle, monkeypatch, path):
    """the rows of the model test (U on p(s) and one ulp above it, s back at 0, s0 == 0 and V, n_k == 0) with their uniforms
    handed in; rows of one length go in one call, a row per topic"""
    force_path(monkeypatch, path)
    rows = R.chain_cases(BETA)
    for V in sorted({r[1].size for r in rows}):
        for pi in (0.5, 0.01):
            group = [r for r in rows if r[1].size == V and r[4] == pi]
            if not group:
                continue
            ref = [R.sequential_chain(c, p, u, BETA, pi) for _, c, p, u, _ in group]
            d, s, rounds = native.debug_vs_indicators(np.array([r[1] for r in group]), np.array([r[2] for r in group]), BETA, pi, SEED, 1,
                                                      u=np.array([r[3] for r in group]))
            for i, (name, c, p, u, _) in enumerate(group):
                assert np.array_equal(d[i], ref[i][0]) and s[i] == ref[i][1], name
                assert 1 <= rounds[i] <= int((c == 0).sum()) + 1, name


# ---- whole sweeps ---------------------------------------------------------------------------------------------------
def assert_derived_state_equal(g, m):
    ps, a, tn = g.alias_tables()
    assert_bit_equal(tn, m.tables[2], "typeNorm")
    assert_bit_equal(a, m.tables[1], "a")
    assert_bit_equal(ps, m.tables[0], "ps")
    nw, topics = g.word_topic_lists()
    assert_bit_equal(nw, m.nw, "nw")
    assert_bit_equal(topics, PS.padded(m.lists, m.K), "the words' lists")
    assert_bit_equal(g.sparse_stats(), m.stats, "sparse_stats")
    vs = g.vs_stats()
    assert tuple(vs[:2]) == m.vs_stats_first_two(), "vs_stats"
    return vs


def run_pair(native, c, K, alpha, beta, sweeps, pi=0.5, zseed=5, flags=0, burn_in=0, thin=1):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_NZVSSPALIAS | native.FLAG_PARANOID | flags, phi_burn_in=burn_in, phi_mean_thin=thin)
    if pi != 0.5:
        g.set_variable_selection_prior(pi)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, pi=pi)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    assert (g.word_topic_lists()[0] == 0).all()                     # no list before the first Phi draw of a sweep
    assert tuple(g.vs_stats()) == (0, int((m.phi == 0.0).sum()), 0)
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
        assert_bit_equal(g.get_phi(), m.phi, "phi after sweep %d" % (s + 1))
        if s == 0:                                                  # drawn from the alias tables alone
            assert list(g.sparse_stats()) == [0, 0, c.num_tokens, 0]
    assert g.launch_info()["z_kernel"] == KERNEL
    n_kw = m.counts()
    assert_bit_equal(g.get_type_topic_counts(), n_kw.T.astype(np.int32), "n_wk")
    assert_bit_equal(g.get_topic_totals(), n_kw.sum(axis=1).astype(np.int32), "n_k")
    vs = assert_derived_state_equal(g, m)
    assert 1 <= vs[2] <= c.num_types + 1
    print("K=%d V=%d pi=%g: %d of %d cells undrawn, %d zero, at most %d rounds; sparse_stats %s" % (K, c.num_types, pi, vs[0], K * c.num_types, vs[1], vs[2], m.stats))
    assert int(m.stats[:3].sum()) == sweeps * c.num_tokens
    return g, m


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, monkeypatch, K, alpha, beta, margin):
    force_form(monkeypatch, margin)
    g, m = run_pair(native, cats, K, alpha, beta, 3)
    g.close()


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("pi", [0.5, 0.9])
def test_a_hundred_topics(native, oracle, monkeypatch, margin, pi):
    """pi = 0.9 keeps most cells: the words' lists are then longer than a wave"""
    force_form(monkeypatch, margin)
    g, m = run_pair(native, random_corpus(300, 700, 60, seed=9), 100, 0.1, 0.01, 3, pi=pi)
    assert m.stats[R.DOC] > 0 and (m.stats[R.WORD] > 0 if pi < 0.9 else m.nw.max() > 64)
    g.close()


@pytest.mark.parametrize("margin", FORMS)
def test_walks_of_more_than_64_candidates(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    lens = np.array([600, 500, 1, 0, 700, 40, 300], np.int64)
    p = 1.0 / np.arange(1, 31)
    tokens = np.random.default_rng(3).choice(30, int(lens.sum()), p=p / p.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 30)
    g, m = run_pair(native, c, 200, 0.1, 0.5, 3)
    assert m.nw.max() > 64 and m.stats[3] > 64 * m.stats[:2].sum() / 4   # lists of both kinds pass a wave's 64 lanes
    g.close()


@pytest.mark.parametrize("path", PATHS)
def test_a_small_prior_and_both_paths(native, oracle, monkeypatch, path):
    force_path(monkeypatch, path)
    g, m = run_pair(native, random_corpus(120, 300, 40, seed=3), 33, 0.1, 0.01, 3, pi=0.01)
    g.close()


def test_an_empty_and_a_one_token_document(native, oracle):
    lens = np.array([0, 1, 25, 7, 0, 1, 40, 13, 2, 31], np.int64)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), np.random.default_rng(9).integers(0, 90, int(lens.sum())).astype(np.int32), 90)
    g, m = run_pair(native, c, 10, 0.1, 0.01, 3)
    g.close()


def test_set_phi_then_z_given_phi(native, oracle):
    c = random_corpus(80, 50, 30, seed=4)
    K = 12
    z0 = oracle.jrandom_ints(2, K, c.num_tokens)
    g = native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=native.FLAG_NZVSSPALIAS)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.set_z(np.asarray(z0, np.int32), redraw_phi=True)
    assert (g.word_topic_lists()[0] == 0).all()                     # the redraw leaves the lists empty
    phi = g.get_phi()
    phi[:, 3] = 0.0                                                 # an all-zero column: no list, no table weight
    phi[np.random.default_rng(1).random(phi.shape) < 0.4] = 0.0
    g.set_phi(phi)
    m = R.Model(K, c.num_types, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, z0)
    m.set_phi(phi)
    nw, topics = g.word_topic_lists()
    assert_bit_equal(nw, (phi != 0.0).sum(axis=0).astype(np.int32), "nw = the cells with phi != 0.0")
    g.sample_z_given_phi(2)
    m.sample_z_given_phi(2)
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z given phi")
    assert_derived_state_equal(g, m)
    g.close()


def test_the_phi_mean_stays_zero_and_n_sampled_counts(native, oracle, cats):
    g, m = run_pair(native, cats, 20, 0.1, 0.01, 4, flags=native.FLAG_SAVE_PHI_MEAN, burn_in=1, thin=1)
    mean, n = g.get_phi_mean()
    assert n == 3
    assert (mean == 0.0).all()                                      # the reference's loopOverTopics override never adds to it
    g.close()


# ---- sharded: bit-identical to one handle ---------------------------------------------------------------------------
# Each rank runs the indicator chain of its own topic slice; the drawn sets travel as the sign of zero of the gathered gammas.
# A drawn cell whose gamma underflowed holds +0.0 and stays listed: every case asserts that it has one.
def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_NZVSSPALIAS)
        h.set_variable_selection_prior(0.4)
        return h

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), phi=h.get_phi(), how=h.count_exchange(), tables=h.alias_tables(),
                    lists=h.word_topic_lists(), stats=h.sparse_stats(), vs=h.vs_stats(), kernel=h.launch_info()["z_kernel"])
    return make_handle, body


def ranks_equal_one_handle(native, world, K, mode):
    sweeps, V = 3, 900
    whole = random_corpus(310, V, 90, seed=K + V, empty_every=9)
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    h = native.GGSHandle(K, V, 0.1, 0.01, SEED, flags=native.FLAG_NZVSSPALIAS)
    h.set_variable_selection_prior(0.4)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    ref = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), phi=h.get_phi(), tables=h.alias_tables(), lists=h.word_topic_lists(), stats=h.sparse_stats(),
               vs=h.vs_stats())
    h.close()
    assert_bit_equal(np.concatenate([out[r]["z"] for r in range(world)]), ref["z"], "z")
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse") and out[r]["kernel"] == KERNEL
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert not np.signbit(out[r]["phi"]).any()                  # the sign that carried the drawn set is cleared on arrival
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))
        for i, name in enumerate(("nw", "the words' lists")):
            assert_bit_equal(out[r]["lists"][i], ref["lists"][i], "%s rank %d" % (name, r))
        assert tuple(out[r]["vs"][:2]) == tuple(ref["vs"][:2]), "undrawn and zero cells, rank %d" % r
    assert max(out[r]["vs"][2] for r in range(world)) == ref["vs"][2]   # a rank reports the rounds of its own topics' chains
    assert_bit_equal(np.sum([out[r]["stats"] for r in range(world)], axis=0), ref["stats"], "sparse_stats summed over the ranks")
    assert ref["vs"][0] > 0 and ref["stats"][0] > 0 and ref["stats"][1] > 0
    # a drawn cell whose Gamma(beta) underflowed: +0.0 and listed.  The sign of zero that carries the drawn set between the ranks
    # must not take it for an undrawn cell (-0.0 on the way); the lists above are already equal on every rank.
    nw, topics = ref["lists"]
    listed = np.zeros((K, V), bool)
    for w in range(V):
        listed[topics[w, :nw[w]], w] = True
    underflowed = int((listed & (ref["phi"] == 0.0)).sum())
    print("world=%d K=%d %s: %d drawn cells hold +0.0, %d cells undrawn" % (world, K, mode, underflowed, ref["vs"][0]))
    assert underflowed >= 1 and int((~listed).sum()) == ref["vs"][0]


@pytest.mark.parametrize("mode", ["dense", "sparse"])
def test_two_ranks_equal_one_handle(native, oracle, mode):
    ranks_equal_one_handle(native, 2, 40, mode)


def test_three_ranks_whose_slices_straddle_the_mask_words(native, oracle):
    """K = 70 over three ranks: slices of 24, 23 and 23 topics, so k0 = 24 and 47 fall inside the 32-bit words of the masks that
    vs_bits_kernel and vs_mask_kernel write by topic"""
    ranks_equal_one_handle(native, 3, 70, "dense")


# ---- misuse and the launch plan -------------------------------------------------------------------------------------
def test_misuse_is_rejected(native):
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA, native.FLAG_POLYAURN_SPARSE,
                  native.FLAG_LIGHTCOLLAPSED):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_NZVSSPALIAS | other)
        assert e.value.code == native.ERR_BAD_ARG
    c = random_corpus(20, 10, 8, seed=1)
    h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_NZVSSPALIAS)
    for bad in (0.0, 1.0, -1.0, float("nan")):
        with pytest.raises(native.GGSError) as e:
            h.set_variable_selection_prior(bad)
        assert e.value.code == native.ERR_BAD_ARG
    h.set_variable_selection_prior(0.3)
    with pytest.raises(native.GGSError) as e:                       # before the first Phi
        h.vs_stats()
    assert e.value.code == native.ERR_STATE
    h.set_corpus(c.doc_ptr, c.tokens)
    h.set_variable_selection_prior(0.4)                             # still no Phi
    h.init_z_java_lcg(1)
    h.init_phi()
    with pytest.raises(native.GGSError) as e:
        h.set_variable_selection_prior(0.5)
    assert e.value.code == native.ERR_STATE
    h.close()
    p = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_PCGS)
    p.set_corpus(c.doc_ptr, c.tokens)
    p.init_z_java_lcg(1)
    p.init_phi()
    for call in (lambda: p.set_variable_selection_prior(0.5), p.vs_stats, p.word_topic_lists, p.sparse_stats):
        with pytest.raises(native.GGSError) as e:
            call()
        assert e.value.code == native.ERR_STATE
    assert "nzvs" not in p.launch_info()["z_kernel"]
    p.close()


def test_launch_info_is_the_scheme_s_own(native):
    rng = np.random.default_rng(1)
    lens = rng.permutation(np.arange(130) % 31)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = Corpus(doc_ptr, rng.integers(0, 40, int(doc_ptr[-1])).astype(np.int32), 40)
    K = 8
    g = native.GGSHandle(K, 40, 0.1, 0.01, SEED, flags=native.FLAG_NZVSSPALIAS | native.FLAG_PARANOID)
    try:
        before = g.launch_info()
        assert before["z_kernel"] == KERNEL and (before["lds_bytes_z"], before["num_chunks"]) == (0, 0)
        g.set_corpus(c.doc_ptr, c.tokens)
        g.init_z_java_lcg(SEED)
        g.init_phi()
        g.sweep(2)
        info = g.launch_info()
        cap = min(K, 30)
        assert info["z_kernel"] == KERNEL
        assert (info["lds_bytes_z"], info["num_chunks"]) == (cap * 8 + K * 4 + K * 2 + ((cap + 3) & ~3) * 2, 130)
        assert info["num_hot"] == 0 and info["warm_tiers"] == 0 and info["z_parts"] == 1 and info["z_form"] == "n/a"
        assert int(g.sparse_stats()[:3].sum()) == 2 * c.num_tokens
    finally:
        g.close()
