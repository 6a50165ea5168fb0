"""z_pairs_kernel (csrc/ggs_z_sliced.hpp): the hot words by pair-chunks -- each (document, hot word) pair scored once, its tokens
drawn from the pair's checkpoints -- against z_hot_kernel (GGS_DEBUG_HOT_PAIRS=0) and the oracle, bit for bit after 2 sweeps.

The corpus is tests/hot_pairs_cases.edges_corpus (the edge rows of the pair-chunk builder: a pair of more tokens than a chunk's
cap, documents of distinct hot words only, of one hot token, empty documents, 64 / 65 pairs across the document limit, 64 n and
64 n + 1 tokens; tests/test_hot_pair_lists_cpu.py pins how the builder cuts them) with a hot table of up to 72 rows, so that
most tokens are hot; K = 8, 100 (one theta piece per lane, a whole table at K <= 100), 129 and 160 (two pieces per lane).
Every K runs on the real grid and on one CU (GGS_DEBUG_NUM_CUS=1: four waves for > 100 pair-chunks, every wave takes a second
and later chunk), each with GGS_DEBUG_MARGIN scaled up so that nearly every token takes the element-by-element replay."""
import numpy as np
import pytest

from tests import persistent_grid as PG
from tests.hot_pairs_cases import HOT, edges_corpus
from tests.ranks import assert_bit_equal

pytestmark = pytest.mark.gpu

SEED, ZSEED, ALPHA, BETA, SWEEPS = 4242, 11, 0.1, 0.01, 2
ENV = {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_SPLIT": "2", "GGS_DEBUG_HOT": str(HOT), "GGS_DEBUG_WARM": "0"}
KS = (8, 100, 129, 160)
MARGIN = "1e13"          # as test_parity_gpu's margin13: delta ~ 10^-2 of the sum, nearly every token is too close to call

_corpus = {}
_oracle = {}


def corpus(name="A"):
    if name not in _corpus:
        _corpus[name] = edges_corpus() if name == "A" else edges_corpus(seed=8, fillers=90)
    return _corpus[name]


def create(native, monkeypatch, env, K, V):
    env = dict(env)
    monkeypatch.delenv(PG.KNOB, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return native.GGSHandle(K, V, ALPHA, BETA, SEED, flags=native.FLAG_PARANOID)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def state_of(s):
    return dict(z=s.get_z(), n_wk=s.get_type_topic_counts(), phi=s.get_phi(), theta=s.get_theta())


def oracle_state(oracle, K):
    """the oracle's state after SWEEPS sweeps over corpus A, once per K"""
    if K not in _oracle:
        c = corpus()
        o = oracle.OracleSampler(K, c.num_types, ALPHA, BETA, SEED, threads=4)
        o.set_corpus(c.doc_ptr, c.tokens)
        o.init_z_java_lcg(ZSEED)
        o.init_phi()
        o.sweep(SWEEPS)
        _oracle[K] = state_of(o)
        for v in _oracle[K].values():
            v.setflags(write=False)
    return _oracle[K]


def device_state(native, monkeypatch, K, env, pairs):
    c = corpus()
    g = create(native, monkeypatch, dict(ENV, **env), K, c.num_types)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(ZSEED)
    g.init_phi()
    info = g.launch_info()
    assert info["z_form"] == "split" and info["num_hot"] > 0, info
    assert info["hot_pairs"] == pairs and ("z_pairs_kernel" in info["z_kernel"]) == pairs, info
    if pairs:
        assert 0 < info["hot_pairs_per_token"] < 1 and info["hot_pair_chunks"] > 0, info
        if env.get(PG.KNOB) == "1":                                 # every one of the CU's four waves takes three chunks and more
            PG.assert_trips(info["hot_pair_chunks"], 1, PG.CAP_SLICED, "z_pairs_kernel", waves=PG.SLICED_WAVES)
    g.sweep(SWEEPS)
    s = state_of(g)
    g.check_invariants()
    g.close()
    return s


def assert_same(got, want, tag):
    for k in ("z", "n_wk", "phi", "theta"):
        assert_bit_equal(got[k], want[k], "%s %s" % (tag, k))


@pytest.mark.parametrize("K", KS)
def test_pairs_kernel_hot_kernel_and_oracle_agree(native, oracle, monkeypatch, K):
    want = oracle_state(oracle, K)
    assert_same(device_state(native, monkeypatch, K, {}, True), want, "z_pairs_kernel")
    assert_same(device_state(native, monkeypatch, K, {"GGS_DEBUG_HOT_PAIRS": "0"}, False), want, "z_hot_kernel")


@pytest.mark.parametrize("K", KS)
def test_pairs_kernel_second_and_later_chunks(native, oracle, monkeypatch, K):
    assert_same(device_state(native, monkeypatch, K, {PG.KNOB: "1"}, True), oracle_state(oracle, K), "one CU")


@pytest.mark.parametrize("cus", [None, "1"])
@pytest.mark.parametrize("K", KS)
def test_pairs_kernel_replays(native, oracle, monkeypatch, K, cus):
    env = {"GGS_DEBUG_MARGIN": MARGIN}
    if cus:
        env[PG.KNOB] = cus
    assert_same(device_state(native, monkeypatch, K, env, True), oracle_state(oracle, K), "margin x %s" % MARGIN)


def test_pairs_kernel_handle_life_cycle(native, oracle, monkeypatch):
    """One handle over corpus A, then B (other documents, tokens and lists; a z given by the caller, an iteration to resume at),
    then A again from the z it left there: every leg against a fresh oracle."""
    K = 100
    A, B = corpus("A"), corpus("B")
    assert (A.num_docs, A.num_tokens) != (B.num_docs, B.num_tokens) and A.num_types == B.num_types
    g = create(native, monkeypatch, ENV, K, A.num_types)
    g.set_corpus(A.doc_ptr, A.tokens)
    g.init_z_java_lcg(ZSEED)
    g.init_phi()
    g.sweep(SWEEPS)
    assert g.launch_info()["hot_pairs"]
    a2 = state_of(g)
    assert_same(a2, oracle_state(oracle, K), "A")

    def resumed(c, z0, iteration, sweeps):
        o = oracle.OracleSampler(K, c.num_types, ALPHA, BETA, SEED, threads=4)
        o.set_corpus(c.doc_ptr, c.tokens)
        o.set_iteration(iteration)
        o.set_z(z0, redraw_phi=False)
        o.init_phi()
        o.sweep(sweeps)
        return state_of(o)

    for c, z0, it, tag in ((B, oracle.jrandom_ints(3, K, B.num_tokens), 5, "B"), (A, a2["z"], SWEEPS, "A again")):
        g.set_corpus(c.doc_ptr, c.tokens)
        g.set_iteration(it)
        g.set_z(z0, redraw_phi=False)
        g.init_phi()
        assert g.launch_info()["hot_pairs"]
        g.sweep(1)
        assert_same(state_of(g), resumed(c, z0, it, 1), tag)
    g.check_invariants()
    g.close()
