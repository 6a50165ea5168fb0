"""scheme=polyaurn_sparse on the device (GGS_FLAG_POLYAURN_SPARSE): whole sweeps, the z step given a Phi, the phi mean and
sharded runs bit for bit against the CPU restatement (tests/polyaurn_sparse_restatement.py) or one handle -- z, counts,
Phi, the alias tables, the words' lists and the counters of which list each token walked; the held-out likelihood
against pcgs; misuse.

There is one z kernel, polyaurn_sparse_wave_kernel (a wave per document), with two ways through it: the wave scans'
proposal, decided outside its margins, and the exact chain that replays what the proposal leaves open.
GGS_DEBUG_MARGIN=1e30 (FORMS) sends every token with candidates through the replay; both ways give the same bits."""

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus, synthetic_lda_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import polyaurn_sparse_restatement as R
from tests.ranks import assert_bit_equal, force_form, run_ranks, z_kernel

pytestmark = pytest.mark.gpu

SEED = 777
KERNEL = "polyaurn_sparse_wave_kernel (wave per document)"
FORMS = [None, "1e30"]                  # GGS_DEBUG_MARGIN: the proposal with its margins / every token replayed exactly


def assert_derived_state_equal(g, m):
    """what follows the handle's current Phi and its z steps so far: tables, lists, counters"""
    ps, a, tn = g.alias_tables()
    assert_bit_equal(tn, m.tables[2], "typeNorm")
    assert_bit_equal(a, m.tables[1], "a")
    assert_bit_equal(ps, m.tables[0], "ps")
    nw, topics = g.word_topic_lists()
    assert_bit_equal(nw, m.nw, "nw")
    assert_bit_equal(topics, R.padded(m.lists, m.K), "the words' lists")
    assert_bit_equal(g.sparse_stats(), m.stats, "sparse_stats")


def run_pair(native, c, K, alpha, beta, sweeps, zseed=5, flags=0, burn_in=0, thin=1, L=0):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_POLYAURN_SPARSE | native.FLAG_PARANOID | flags,
                         phi_burn_in=burn_in, phi_mean_thin=thin, alias_poisson_threshold=L)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, L=L, save_phi_mean=bool(flags & native.FLAG_SAVE_PHI_MEAN),
                phi_burn_in=burn_in, phi_thin=thin)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
    assert z_kernel(g) == KERNEL
    n_kw = m.counts()
    assert_bit_equal(g.get_type_topic_counts(), n_kw.T.astype(np.int32), "n_wk")
    assert_bit_equal(g.get_topic_totals(), n_kw.sum(axis=1).astype(np.int32), "n_k")
    assert_bit_equal(g.get_phi(), m.phi, "phi")
    assert_derived_state_equal(g, m)
    assert int(m.stats[:3].sum()) == sweeps * c.num_tokens
    return g, m


# ---- whole runs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, monkeypatch, K, alpha, beta, margin):
    force_form(monkeypatch, margin)
    g, m = run_pair(native, cats, K, alpha, beta, 4)
    g.close()


@pytest.mark.parametrize("margin", FORMS)
def test_empty_and_one_token_documents_and_all_three_ways(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    c = random_corpus(300, 700, 60, seed=9, empty_every=7)
    lens = np.diff(c.doc_ptr)
    assert (lens == 0).any() and (lens == 1).any()
    g, m = run_pair(native, c, 100, 0.1, 0.01, 2, L=7)
    stats = g.sparse_stats()
    print("K=100: %d tokens walked the word's list, %d the document's, %d drawn uniformly; sum of n %d" % tuple(stats))
    assert (stats[:3] > 0).all()
    g.close()


def long_lists_corpus():
    lens = np.array([600, 500, 1, 0, 700, 40, 300], np.int64)
    p = 1.0 / np.arange(1, 31)
    tokens = np.random.default_rng(3).choice(30, int(lens.sum()), p=p / p.sum()).astype(np.int32)
    return Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 30)


@pytest.mark.parametrize("margin", FORMS)
def test_lists_of_both_kinds_longer_than_a_wave(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    g, m = run_pair(native, long_lists_corpus(), 200, 0.1, 0.5, 2)
    print("K=200: stats %s; more than 64 candidates: %d word-list tokens, %d document-list tokens" % (m.stats, m.over64[R.WORD], m.over64[R.DOC]))
    assert m.over64[R.WORD] > 0 and m.over64[R.DOC] > 0
    g.close()


def test_a_document_of_33000_tokens(native, oracle):
    rng = np.random.default_rng(3)
    lens = np.array([33000, 1, 40, 0, 7], np.int64)
    tokens = rng.integers(0, 300, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 300)
    g, m = run_pair(native, c, 30, 0.1, 0.01, 2)
    g.close()


def test_4096_topics(native, oracle):
    c = random_corpus(40, 60, 150, seed=4096, empty_every=11)
    g, m = run_pair(native, c, 4096, 0.05, 0.01, 1)
    assert m.stats[R.WORD] > 0 and m.stats[R.DOC] > 0
    g.close()


def test_phi_mean_with_burn_in_and_thin(native, oracle, cats):
    g, m = run_pair(native, cats, 20, 0.1, 0.01, 6, flags=native.FLAG_SAVE_PHI_MEAN, burn_in=2, thin=2)
    mean, n = g.get_phi_mean()
    assert n == m.n_sampled == 2
    assert_bit_equal(mean, m.phi_mean(), "phi mean")
    g.close()


# ---- the z step given a Phi -----------------------------------------------------------------------------------------
def given_phi(native, c, K, alpha, z0, phi):
    """(handle, restatement) after set_phi(phi) and one sample_z_given_phi from z0"""
    g = native.GGSHandle(K, c.num_types, alpha, 0.01, SEED, flags=native.FLAG_POLYAURN_SPARSE)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.set_z(np.asarray(z0, np.int32), redraw_phi=True)
    if phi is None:
        phi = g.get_phi()
    elif callable(phi):
        phi = phi(g.get_phi())
    g.set_phi(phi)
    m = R.Model(K, c.num_types, alpha, 0.01, SEED, c.doc_ptr, c.tokens, z0)
    m.set_phi(phi)
    g.sample_z_given_phi(1)
    m.sample_z_given_phi(1)
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z given phi")
    assert_derived_state_equal(g, m)
    return g, m


def test_zeroed_columns_draw_floor_u_k(native, oracle):
    c = random_corpus(80, 50, 30, seed=4)
    K = 12

    def zeroed(phi):
        phi[:, 3] = 0.0                                             # words 3 and 5: all-zero columns
        phi[:, 5] = 0.0
        return phi
    g, m = given_phi(native, c, K, 0.1, oracle.jrandom_ints(2, K, c.num_tokens), zeroed)
    U = oracle.uniforms(SEED, 1, R.PURPOSE_Z, 0, c.num_tokens)
    hit = np.flatnonzero(np.isin(c.tokens, [3, 5]))
    assert hit.size and (g.get_z()[hit] == np.minimum((U[hit] * K).astype(np.int32), K - 1)).all()
    assert g.sparse_stats()[2] >= hit.size
    nw, topics = g.word_topic_lists()
    assert nw[3] == nw[5] == 0 and (topics[[3, 5]] == -1).all()
    g.close()


def test_a_dense_phi_never_walks_a_words_list(native, oracle):
    c = random_corpus(80, 50, 30, seed=4)
    K = 12
    phi = np.random.default_rng(1).random((K, c.num_types)) + 0.01  # no zeros: nw = K >= nd for every token
    phi /= phi.sum(axis=1, keepdims=True)
    g, m = given_phi(native, c, K, 0.1, oracle.jrandom_ints(2, K, c.num_tokens), phi)
    stats = g.sparse_stats()
    assert stats[0] == 0 and stats[1] > 0
    assert (g.word_topic_lists()[0] == K).all()
    g.close()


def test_a_tie_goes_to_the_documents_list_and_one_below_to_the_words(native, oracle):
    """Word 0 has phi != 0 at topic 0 only (nw = 1).  Document A, two tokens of it on topics 0, 1: each token finds one
    topic left in the document (nd = 1 = nw): the document's list, twice.  Document B, three tokens on topics 0, 1, 2:
    the first two find nd = 2 = nw + 1: the word's list; both move to topic 0, so the third finds nd = 1: a tie again.
    Every token ends on topic 0 (the only topic with weight)."""
    K = 4
    c = Corpus(np.array([0, 2, 5], np.int64), np.zeros(5, np.int32), 2)
    phi = np.zeros((K, 2))
    phi[0] = [0.5, 0.5]
    phi[1:, 1] = 1.0
    g, m = given_phi(native, c, K, 0.1, np.array([0, 1, 0, 1, 2]), phi)
    assert (g.get_z() == 0).all()
    assert list(g.sparse_stats()) == [2, 3, 0, 5]
    g.close()


# ---- sharded: bit-identical to one handle ---------------------------------------------------------------------------
CREATE = dict(phi_burn_in=1, phi_mean_thin=2, alias_poisson_threshold=20)


def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN_SPARSE | native.FLAG_SAVE_PHI_MEAN, **CREATE)

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(),
                    how=h.count_exchange(), tables=h.alias_tables(), lists=h.word_topic_lists(), stats=h.sparse_stats(), kernel=z_kernel(h))
    return make_handle, body


def one_handle(native, whole, K, sweeps):
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN_SPARSE | native.FLAG_SAVE_PHI_MEAN, **CREATE)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    r = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), tables=h.alias_tables(),
             lists=h.word_topic_lists(), stats=h.sparse_stats())
    h.close()
    return r


@pytest.mark.parametrize("mode,K,V", [("dense", 40, 900), ("sparse", 100, 1100)])
def test_two_ranks_equal_one_handle(native, oracle, mode, K, V):
    world, sweeps = 2, 4
    whole = random_corpus(310, V, 90, seed=K + V, empty_every=9)
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    ref = one_handle(native, whole, K, sweeps)
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert z.size == whole.num_tokens
    assert_bit_equal(z, ref["z"], "z")
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        assert out[r]["kernel"] == KERNEL
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], ref["nk"], "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))
        for i, name in enumerate(("nw", "the words' lists")):
            assert_bit_equal(out[r]["lists"][i], ref["lists"][i], "%s rank %d" % (name, r))
    assert_bit_equal(out[0]["lists"][1], out[1]["lists"][1], "the words' lists of the two ranks")
    assert_bit_equal(out[0]["stats"] + out[1]["stats"], ref["stats"], "sparse_stats summed over the ranks")
    assert ref["stats"][0] > 0 and ref["stats"][1] > 0


# ---- statistics -----------------------------------------------------------------------------------------------------
def heldout_after(native, flags, train, test, K, sweeps):
    h = native.GGSHandle(K, train.num_types, 0.1, 0.01, 4711, flags=flags)
    h.set_corpus(train.doc_ptr, train.tokens)
    h.init_z_java_lcg(4711)
    h.init_phi()
    h.sweep(sweeps)
    h.set_test_corpus(test.doc_ptr, test.tokens)
    ll, _ = h.heldout_log_likelihood(100)
    stats = h.sparse_stats() if flags & native.FLAG_POLYAURN_SPARSE else None
    h.close()
    return ll, stats


def test_heldout_likelihood_matches_pcgs(native):
    """The held-out log likelihood after 300 sweeps within 1 % of pcgs's (the bar the polyaurn and spalias tests use).  A
    wrong split of U between the alias draw and the walk, or a walk over the wrong list, would show here."""
    full = synthetic_lda_corpus(2200, 2000, 60, true_topics=20, seed=99)
    train, _, _ = full.shard(0, 2000)
    test, _, _ = full.shard(2000, 2200)
    K, sweeps = 20, 300
    ps, stats = heldout_after(native, native.FLAG_POLYAURN_SPARSE, train, test, K, sweeps)
    pc, _ = heldout_after(native, native.FLAG_PCGS, train, test, K, sweeps)
    gap = abs(ps - pc) / abs(pc)
    print("held-out log likelihood after %d sweeps: polyaurn_sparse %.2f, pcgs %.2f, gap %.4f; sparse_stats %s" % (sweeps, ps, pc, gap, stats))
    assert gap < 0.01


# ---- the launch and misuse ------------------------------------------------------------------------------------------
def spalias_lds(K, cap):               # polyaurn_sparse_lds_bytes = spalias_lds_bytes: [cap] doubles, [K] int32, [K] int16, [cap rounded up to 4] int16
    return cap * 8 + K * 4 + K * 2 + ((cap + 3) & ~3) * 2


@pytest.mark.parametrize("K", [8, 200])
def test_launch_info_is_the_scheme_s_own(native, K):
    rng = np.random.default_rng(1)
    lens = rng.permutation(np.arange(130) % 31)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c = Corpus(doc_ptr, rng.integers(0, 40, int(doc_ptr[-1])).astype(np.int32), 40)
    g = native.GGSHandle(K, 40, 0.1, 0.01, SEED, flags=native.FLAG_POLYAURN_SPARSE | native.FLAG_PARANOID)
    try:
        before = g.launch_info()
        assert before["z_kernel"] == KERNEL and (before["lds_bytes_z"], before["num_chunks"]) == (0, 0)
        g.set_corpus(c.doc_ptr, c.tokens)
        g.init_z_java_lcg(SEED)
        g.init_phi()
        g.sweep(2)
        info = g.launch_info()
        assert info["z_kernel"] == KERNEL
        assert (info["lds_bytes_z"], info["num_chunks"]) == (spalias_lds(K, min(K, 30)), 130)
        assert info["num_hot"] == 0 and info["warm_tiers"] == 0 and info["z_parts"] == 1 and info["z_form"] == "n/a"
        assert int(g.sparse_stats()[:3].sum()) == 2 * c.num_tokens
    finally:
        g.close()


def test_misuse_is_rejected(native):
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN_SPARSE | other)
        assert e.value.code == native.ERR_BAD_ARG
    with pytest.raises(native.GGSError) as e:
        native.GGSHandle(4097, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN_SPARSE)
    assert e.value.code == native.ERR_UNSUPPORTED
    # every other scheme: no lists, no counters -- the getters say so, and launch_info names another kernel
    others = {"ggs": 0, "pcgs": native.FLAG_PCGS, "collapsed": native.FLAG_COLLAPSED, "polyaurn": native.FLAG_POLYAURN,
              "spalias": native.FLAG_SPALIAS, "lightpclda": native.FLAG_LIGHTPCLDA}
    c = random_corpus(20, 10, 8, seed=1)
    for scheme, flags in others.items():
        h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=flags)
        h.set_corpus(c.doc_ptr, c.tokens)
        h.init_z_java_lcg(1)
        h.init_phi()
        for getter in (h.word_topic_lists, h.sparse_stats):
            with pytest.raises(native.GGSError) as e:
                getter()
            assert e.value.code == native.ERR_STATE, scheme
        assert "polyaurn_sparse" not in h.launch_info()["z_kernel"]
        h.close()
    h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN_SPARSE)
    for getter in (h.word_topic_lists, h.alias_tables):             # before the first Phi
        with pytest.raises(native.GGSError) as e:
            getter()
        assert e.value.code == native.ERR_STATE
    assert (h.sparse_stats() == 0).all()
    assert h.launch_info()["z_kernel"] == KERNEL
    h.close()
