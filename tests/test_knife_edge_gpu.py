"""Every z kernel on knife-edge rows (tests/test_knife_edge_model.py): Phi columns that end one chosen token's Java walk
exactly on a boundary -- t_{J+1} == 0, the smallest positive / negative t_{J+1}, at the 16 / 32 / 64-topic slice and
checkpoint edges, beside zero and sub-FLT_MIN scores, around the float32 path's 2^-60 gate -- put through each kernel
form a debug switch reaches, z and n_wk bit-compared with the oracle, failures reported by category and position.

The float32 cold path (z_sliced32_kernel) is tied to its numpy model (tests/test_margin32_model.kernel_rule): the replay
count GGS_DEBUG_REPLAYS reports is the number of tokens the model leaves undecided at margin 1, and with
GGS_DEBUG_MARGIN=0 the device draws the model's cnt wherever the model decides -- which differs from the Java draw on the
"decisive" rows, so these rows do reach the float32 decision.  Both hold with float32 denormals KEPT (flush=False in the
model): the kernels are compiled without denormal flushing (hipcc's default for gfx950, no -ffast-math /
-fgpu-flush-denormals-to-zero), and the model with flushing disagrees on the sub-FLT_MIN rows."""
import re

import numpy as np
import pytest

from tests.test_knife_edge_model import KnifeEdge, repeated_word_corpus, unique_word_corpus
from tests.test_margin32_model import java_draw, kernel_rule

pytestmark = pytest.mark.gpu

DECISIVE_MIN = 20


def replays_reported(err):
    m = re.findall(r"\[ggs\] z replays: (\d+) tokens in (\d+) launches", err)
    assert m, err[-2000:]
    return int(m[-1][0]), int(m[-1][1])


def device_step(native, monkeypatch, ke, env, flags=0):
    """A handle in the state the KnifeEdge was built from (the switches set before set_corpus, which reads several of
    them), the boundary Phi, one z step given Phi.  Returns (handle, launch_info)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = ke.c
    g = native.GGSHandle(ke.K, c.num_types, ke.alpha, ke.beta, ke.seed, flags=native.FLAG_PARANOID | flags)
    g.set_corpus(c.doc_ptr, c.tokens, 0, 0)
    g.init_z_java_lcg(ke.zseed)
    g.init_phi()
    g.set_phi(ke.phi)
    g.sample_z_given_phi(1)
    return g, g.launch_info()


def check_against_oracle(oracle, ke, g, tag):
    zo, nwko = ke.oracle_step(oracle)
    # the builder is checked too: a broken builder must not let a case pass
    wrong = np.flatnonzero(zo[ke.boundary] != ke.predicted)
    assert wrong.size == 0, "%s: the oracle does not draw the builder's walk: %s" % (tag, ke.describe(wrong[:8]))
    zg = g.get_z()
    bad = np.flatnonzero(zg != zo)
    if bad.size:
        pos = {int(t): r for r, t in enumerate(ke.boundary)}
        rows = [pos[int(i)] for i in bad if int(i) in pos]
        by = {}
        for r in rows:
            for t in ke.tags[r]:
                by[t] = by.get(t, 0) + 1
        pytest.fail("%s: %d of %d tokens differ (%d boundary tokens; by category %s); first: %s" % (
            tag, bad.size, zg.size, len(rows), dict(sorted(by.items())),
            ["%s device %d oracle %d" % (d, zg[ke.boundary[r]], zo[ke.boundary[r]]) for d, r in zip(ke.describe(rows[:8]), rows[:8])]))
    assert np.array_equal(g.get_type_topic_counts(), nwko), tag + ": n_wk"


def cold32_env(extra=None):
    return dict({"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_HOT": "0", "GGS_DEBUG_SPLIT": "2", "GGS_DEBUG_REPLAYS": "1"}, **(extra or {}))


WARMSPARSE = {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_WARM": "8", "GGS_DEBUG_WARM_ROWS": "16", "GGS_DEBUG_WARM_FILL": "1", "GGS_DEBUG_HOT": "8",
              "GGS_DEBUG_WARM_CPW": "0"}

# (form, K, env, corpus, scheme, what launch_info must say)
CASES = [("sliced32", K, cold32_env(), "unique", "ggs", "z_sliced") for K in (20, 64, 100, 113, 160)] + \
    [("sliced64", K, cold32_env({"GGS_DEBUG_PHI64": "1"}), "unique", "ggs", "z_sliced") for K in (100, 160)] + \
    [("hot_split", K, {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_SPLIT": "2", "GGS_DEBUG_HOT": "24", "GGS_DEBUG_WARM": "0"}, "repeated", "ggs", "split") for K in (20, 100, 113)] + \
    [("hot_fused", 100, {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_SPLIT": "0", "GGS_DEBUG_HOT": "24", "GGS_DEBUG_WARM": "0"}, "repeated", "ggs", "fused")] + \
    [("warm", K, WARMSPARSE, "repeated", "ggs", "warm") for K in (20, 100, 160)] + \
    [("stream1", K, {"GGS_DEBUG_ZKERNEL": "2"} if K <= 192 else {}, "unique", "ggs", "z_stream1") for K in (48, 200, 257, 1024)] + \
    [("stream2", K, {"GGS_DEBUG_ZKERNEL": "3"}, "unique", "ggs", "z_stream_kernel") for K in (48, 257)] + \
    [("tile", K, {"GGS_DEBUG_ZKERNEL": "0"}, "unique", "ggs", "z_kernel") for K in (5, 100)] + \
    [("pcgs_lane", K, {}, "unique", "pcgs", "lane") for K in (20, 100)] + \
    [("pcgs_stream", K, {"GGS_DEBUG_PCGS_STREAM": "1", "GGS_DEBUG_PCGS_WAVE": "0"}, "unique", "pcgs", "lane") for K in (20, 100)] + \
    [("pcgs_wave", K, {"GGS_DEBUG_PCGS_WAVE": "1"}, "unique", "pcgs", "wave") for K in (20, 100, 200)] + \
    [("sliced32_alpha1e-3", 100, cold32_env(), "unique", "ggs", "z_sliced"), ("stream1_alpha1e-3", 200, {}, "unique", "ggs", "z_stream1")]


def make_knife_edge(oracle, K, corpus, scheme, alpha=0.1, aim_every=1):
    if scheme == "pcgs":
        return KnifeEdge(oracle, unique_word_corpus(300, 5, 900 + K), K, alpha=alpha, seed=40 + K, zseed=K, scheme="pcgs", build_seed=K + 2, scan=128)
    if corpus == "repeated":
        return KnifeEdge(oracle, repeated_word_corpus(300, 30, 300, 50 + K), K, alpha=alpha, seed=70 + K, zseed=K, repeated=True, build_seed=K + 1)
    return KnifeEdge(oracle, unique_word_corpus(80 if K <= 160 else 40, 26, K), K, alpha=alpha, seed=300 + K, zseed=K, build_seed=K,
                     scan=256 if K <= 160 else 64, aim_every=aim_every)


@pytest.mark.parametrize("form,K,env,corpus,scheme,want", CASES, ids=["%s-K%d" % (c[0], c[1]) for c in CASES])
def test_knife_edge_rows_every_z_kernel(native, oracle, monkeypatch, capfd, form, K, env, corpus, scheme, want):
    # the float32 cold path: every other token aimed, the rest keep init_phi's columns -- so that the replay count below
    # separates the tokens the rule decides from those it does not (an aimed token is never decided at margin 1)
    ke = make_knife_edge(oracle, K, corpus, scheme, alpha=1e-3 if form.endswith("alpha1e-3") else 0.1, aim_every=2 if form == "sliced32" else 1)
    g, info = device_step(native, monkeypatch, ke, env, native.FLAG_PCGS if scheme == "pcgs" else 0)
    zk = info["z_kernel"]
    if want == "z_sliced":
        assert zk.startswith("z_sliced_kernel") and info["num_hot"] == 0 and info["num_warm"] == 0, info
    elif want in ("split", "fused"):
        assert zk.startswith("z_sliced_kernel") and info["num_hot"] > 0 and info["num_warm"] == 0 and info["z_form"] == want, info
    elif want == "warm":
        assert "z_warm_kernel" in zk and info["warm_tiers"] >= 1 and info["num_warm"] > 0, info
    elif want == "z_stream1":
        assert zk.startswith("z_stream1_kernel"), info
    else:
        assert want in zk, info
    try:
        check_against_oracle(oracle, ke, g, "%s K=%d (%s)" % (form, K, zk))
    finally:
        g.close()
    if form == "sliced32":
        # margin 1: the kernel replays exactly the tokens the model leaves undecided (every token is cold: GGS_DEBUG_HOT=0)
        n, launches = replays_reported(capfd.readouterr().err)
        assert launches == 1
        decided, _ = kernel_rule(*ke.all_rows(), K, (K + 7) // 8 * 8, False, margin=1.0)
        aimed = np.zeros(decided.size, bool)
        aimed[ke.boundary] = True
        print("%s K=%d: %d replays, the model %d undecided of %d tokens (%d of the %d aimed ones)" % (
            form, K, n, (~decided).sum(), decided.size, (~decided[aimed]).sum(), aimed.sum()))
        assert n == int((~decided).sum()), (n, int((~decided).sum()))
        assert decided[~aimed].mean() > 0.9, decided[~aimed].mean()      # the count is not everything by default


@pytest.mark.parametrize("K", [20, 64, 100, 113, 160])
def test_float32_margin_zero_draws_the_model(native, oracle, monkeypatch, capfd, K):
    """GGS_DEBUG_MARGIN=0 (below the proved margin: z_sliced32_kernel only): the device draws kernel_rule's cnt where the
    model decides at margin 0 and the Java draw where it does not -- and differs from the oracle on the decisive rows."""
    ke = make_knife_edge(oracle, K, "unique", "ggs", aim_every=2)
    g, info = device_step(native, monkeypatch, ke, cold32_env({"GGS_DEBUG_MARGIN": "0"}))
    assert info["z_kernel"].startswith("z_sliced_kernel") and info["num_hot"] == 0, info
    zg = g.get_z()
    g.close()
    n, launches = replays_reported(capfd.readouterr().err)
    assert launches == 1
    th, ph, U = ke.all_rows()
    decided, cnt = kernel_rule(th, ph, U, K, (K + 7) // 8 * 8, False, margin=0.0)
    java = java_draw(th, ph, U)
    want = np.where(decided, cnt, java)
    bad = np.flatnonzero(zg != want)
    assert bad.size == 0, "K=%d margin 0: %d tokens off the model, first %s device %s model %s java %s" % (
        K, bad.size, bad[:8], zg[bad[:8]], want[bad[:8]], java[bad[:8]])
    assert n == int((~decided).sum())
    zo, _ = ke.oracle_step(oracle)
    assert np.array_equal(zo, java)
    differ = int((zg != zo).sum())
    print("K=%d margin 0: %d of %d tokens drawn off the Java walk (the model: %d), %d replays" % (
        K, differ, zg.size, int((decided & (cnt != java)).sum()), n))
    assert differ >= DECISIVE_MIN
