"""The cold chunks of the score-register path scored from the float32 shadow of phiT (z_sliced32_kernel): every draw is
decided by the margin of ggs_z_sliced.hpp or replayed exactly from the fp64 row, so z stays the oracle's bit for bit --
with the margin scaled up so that a share of / all the cold tokens take the replay (GGS_DEBUG_MARGIN), with Phi rows that
hold values below FLT_MIN, exact ties and a dominant topic (loaded through ggs_set_phi), and against the fp64 path of the
same build (GGS_DEBUG_PHI64=1)."""
import re

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests.ranks import assert_bit_equal

pytestmark = pytest.mark.gpu


def make_pair(native, oracle, corpus, K, seed, zseed):
    g = native.GGSHandle(K, corpus.num_types, 0.1, 0.01, seed, flags=native.FLAG_PARANOID)
    o = oracle.OracleSampler(K, corpus.num_types, 0.1, 0.01, seed, threads=4)
    g.set_corpus(corpus.doc_ptr, corpus.tokens, 0, 0)
    o.set_corpus(corpus.doc_ptr, corpus.tokens, 0, 0)
    g.init_z_java_lcg(zseed)
    o.init_z_java_lcg(zseed)
    g.init_phi()
    o.init_phi()
    return g, o


def compare_state(g, o, tag):
    assert_bit_equal(g.get_z(), o.get_z(), tag + " z")
    assert_bit_equal(g.get_type_topic_counts(), o.get_type_topic_counts(), tag + " n_wk")
    assert_bit_equal(g.get_phi(), o.get_phi(), tag + " phi")
    assert_bit_equal(g.get_theta(), o.get_theta(), tag + " theta")


def replays_reported(err):
    m = re.findall(r"\[ggs\] z replays: (\d+) tokens in (\d+) launches", err)
    assert m, err[-2000:]
    return int(m[-1][0]), int(m[-1][1])


def split_env(monkeypatch, extra):
    # the cold kernel beside z_hot_kernel whatever the first step's timing says, a small hot table: most chunks are cold
    for k, v in dict({"GGS_DEBUG": "1", "GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_SPLIT": "2", "GGS_DEBUG_HOT": "4", "GGS_DEBUG_REPLAYS": "1"}, **extra).items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("margin", ["1", "1e4", "1e9"])
@pytest.mark.parametrize("K", [20, 64, 100, 104, 113, 160])
def test_float32_cold_path_replays_agree(native, oracle, monkeypatch, capfd, K, margin):
    """margin 1: the proved margin; 1e4: a good share of the cold tokens is too close to call; 1e9: every one of them is
    (delta > A): each is replayed from the fp64 row, and the replay count says so."""
    split_env(monkeypatch, {"GGS_DEBUG_MARGIN": margin})
    c = random_corpus(150, 400, 140, seed=K + 11, empty_every=11)
    g, o = make_pair(native, oracle, c, K, 90 + K, K)
    assert g.launch_info()["num_hot"] <= 4
    g.sweep(3)
    o.sweep(3)
    compare_state(g, o, "float32 cold path K=%d margin %s" % (K, margin))
    g.close()
    n, launches = replays_reported(capfd.readouterr().err)
    assert launches >= 3
    if margin == "1e9":
        assert n > 0.3 * 3 * c.num_tokens, (n, c.num_tokens)
    elif margin == "1e4":
        assert n > 0


@pytest.mark.parametrize("K", [20, 100, 113, 160])
def test_float32_cold_path_adversarial_phi(native, oracle, monkeypatch, capfd, K):
    """Phi rows through ggs_set_phi that the float32 shadow cannot hold as they are: values below FLT_MIN (1e-300, the
    subnormal 1e-40, 0), words whose rows are exact copies of each other across topics (ties of every partial sum
    between topics), a dominant topic beside 1e-30 entries; z given that Phi (UPLDA:975-1014) against the oracle."""
    split_env(monkeypatch, {})
    c = random_corpus(150, 400, 140, seed=K + 23, empty_every=11)
    g, o = make_pair(native, oracle, c, K, 50 + K, K + 3)
    V = c.num_types
    rng = np.random.default_rng(K)
    phi = rng.dirichlet(np.full(V, 0.05), K)
    phi[:, 0:40] = np.where(rng.random((K, 40)) < 0.5, 1e-300, 1e-40)   # whole words below FLT_MIN
    phi[::3, 40:80] = 0.0
    phi[:, 80:120] = 1.0 / V                                          # ties: the same value in every topic
    phi[:, 120:160] = 1e-30
    phi[K // 2, 120:160] = 0.5                                        # a dominant topic
    phi[:, 160:200] = np.where((np.arange(K) % 2 == 0)[:, None], 3e-39, 2.0 ** -126)   # around FLT_MIN
    g.set_phi(phi)
    o.set_phi(phi)
    g.sample_z_given_phi(2)
    for _ in range(2):
        o.set_iteration(o.iteration + 1)
        o.z_step()
        o.update_counts()
    assert_bit_equal(g.get_z(), o.get_z(), "z given adversarial phi K=%d" % K)
    assert_bit_equal(g.get_type_topic_counts(), o.get_type_topic_counts(), "counts given adversarial phi K=%d" % K)
    g.close()
    replays_reported(capfd.readouterr().err)


@pytest.mark.parametrize("K", [100, 160])
def test_fp64_switch_same_bits(native, oracle, monkeypatch, K):
    """GGS_DEBUG_PHI64=1 (the fp64 cold path of the same build) and the default float32 path draw the same z."""
    c = random_corpus(150, 400, 140, seed=K + 31, empty_every=11)
    out = []
    for phi64 in ("1", "0"):
        split_env(monkeypatch, {"GGS_DEBUG_PHI64": phi64})
        g, o = make_pair(native, oracle, c, K, 7 + K, K)
        g.sweep(3)
        out.append((g.get_z(), g.get_phi()))
        g.close()
    assert_bit_equal(out[0][0], out[1][0], "z fp64 vs float32 cold path")
    assert_bit_equal(out[0][1], out[1][1], "phi fp64 vs float32 cold path")
