"""The device's chains against the enumerated LDA posterior (tests/lda_posterior.py; the CPU side of the same check is
tests/test_posterior_model.py).  The recipe of every case: a handle started like the parity tests start one (seeded z0,
initial Phi), 50 burn-in sweeps, n = 4000 samples of the whole z vector (sweep(thin), get_z()), and then TWO assertions:

  parity   the histogram of the visited states is IDENTICAL to the one the CPU restatement gives from the same seed
           (where a CPU chain exists and is affordable: every fixture-A case; ggs at K = 40 in the three forced streaming
           forms and at K = 100, default and split; pcgs at K = 100 and 200);
  model    the pooled chi-square of that histogram against the exact posterior gives p > 0.01.

A failure says which of the two it is: equal histograms that are rejected are a model bug shared by the restatement and
the kernel; different histograms are a parity bug.

Fixture A is K = 3.  Fixture B is the same corpus with the topics padded to K = 40 / 100 / 200 / 1024 by alpha = 1e-12: the padded
topics must never be drawn (asserted at every sample) and the state projected on the first three topics has fixture A's
posterior to about 1e-9, so the wide-row kernels are pinned by the same 729 states.

Forced forms that fixture A cannot reach (each is an explicit skip naming the form, and these three cases are the only
ones that may skip; all three run on fixture B at K = 40, where the plan running another kernel is a failure): GGS_DEBUG_ZKERNEL=2, GGS_DEBUG_ZKERNEL=3 and GGS_DEBUG_ZKERNEL=2 with GGS_DEBUG_MARGIN=1e13 --
the streaming kernels take rows of more than 32 topics, below that the plan keeps the whole-row tile kernel.
"""
import functools
import time

import numpy as np
import pytest

from tests import lda_posterior as LP

pytestmark = pytest.mark.gpu

SEED = 1
P_ACCEPT = 0.01
Z_BAR = 4.5
A = LP.FIXTURE_A
N_SAMPLES, BURN_IN, THIN = LP.N_SAMPLES, LP.BURN_IN, LP.THIN

TILE, SLICED, STREAM1, STREAM2 = "z_kernel (whole-row tiles)", "z_sliced_kernel", "z_stream1_kernel", "z_stream_kernel (two passes)"
LANE, WAVE, SPALIAS = "pcgs_sliced_kernel (lane per document)", "pcgs_wave_kernel", "spalias_wave_kernel"


@functools.lru_cache(maxsize=None)
def posterior():
    return LP.enumerate_posterior(A.doc_ptr, A.tokens, A.K, A.V, A.alpha, A.beta)


@functools.lru_cache(maxsize=None)
def cpu_histogram(scheme, K, n=N_SAMPLES):
    """The CPU restatement's histogram of visited states from SEED: computed once per (scheme, K, n), shared by the cases."""
    from oracle import oracle as O
    fx = A if K == A.K else LP.fixture_b(K)
    idx = LP.spalias_chain(O, fx, SEED, n) if scheme == "spalias" else LP.oracle_chain(O, fx, scheme, SEED, n)
    h = LP.histogram(idx, 729)
    h.setflags(write=False)
    return h


def make_handle(native, monkeypatch, fx, flags, env, want_kernel, may_skip=False):
    """A handle on fixture fx with the knobs of env set while the plan is made (the pattern of test_alternate_z_kernels_agree).
    Every error is an error, and the plan must run want_kernel.  may_skip (fixture A with a forced streaming form, nothing
    else) turns ONE thing into a skip that names the form: the plan quietly keeping another kernel than the forced one."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        g = native.GGSHandle(fx.K, fx.V, np.asarray(fx.alpha), fx.beta, SEED, flags=flags, phi_burn_in=BURN_IN)
    finally:
        for k in env:                                               # ggs_create has read every knob
            monkeypatch.delenv(k)
    g.set_corpus(fx.doc_ptr, np.asarray(fx.tokens, np.int32))
    g.init_z_java_lcg(SEED)
    g.init_phi()
    if want_kernel is not None:
        ran = g.launch_info()["z_kernel"]
        if may_skip and want_kernel not in ran:
            pytest.skip("forced form %r does not apply at K = %d: the plan keeps %s" % (env, fx.K, ran))
        assert want_kernel in ran, "K = %d, %r: expected %s, the plan runs %s" % (fx.K, env or "default plan", want_kernel, ran)
    return g


def check(idx, what, reference, n=N_SAMPLES):
    """the two assertions of a case; reference = the CPU histogram or None"""
    h = LP.histogram(idx, 729)
    v = LP.verdict(idx, posterior().p)
    same = None if reference is None else bool(np.array_equal(h, reference))
    print("%s: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f, histogram %s" % (
        what, v.chi2, v.cells, v.pvalue, v.tv, {None: "not compared", True: "identical to the CPU chain's", False: "DIFFERS from the CPU chain's"}[same]))
    assert v.n == n
    assert same is not False, ("PARITY bug: %s visits other states than its CPU restatement from the same seed (%d of 729 cells differ); "
                               "against the posterior: %r" % (what, int((h != reference).sum()), v))
    assert v.pvalue > P_ACCEPT, ("MODEL bug: %s is not a sampler of the LDA posterior (%r); its histogram %s" % (
        what, v, "equals the CPU restatement's, so both are wrong" if same else "has no CPU chain to compare with"))


def run_case(native, monkeypatch, fx, flags, env, want_kernel, scheme, parity, expect=None, may_skip=False, n=N_SAMPLES):
    g = make_handle(native, monkeypatch, fx, flags, env, want_kernel, may_skip)
    info = g.launch_info()
    print("plan: %s, form %s, %d hot words, %d warm" % (info["z_kernel"], info["z_form"], info["num_hot"], info["num_warm"]))
    for key, want in (expect or {}).items():
        assert info[key] == want, "forced form %r: %s is %r, not %r" % (env, key, info[key], want)
    t0 = time.perf_counter()
    step = (lambda m: g.collapsed_serial_sweep(SEED, m)) if scheme == "collapsed" else g.sweep
    idx = LP.run_chain(step, g.get_z, 3, n, THIN[scheme], BURN_IN, max_topic=2)
    dt = time.perf_counter() - t0
    sweeps = BURN_IN + n * THIN[scheme]
    print("device chain: %d sweeps + %d get_z in %.2f s (%.0f us per sweep)" % (sweeps, n, dt, 1e6 * dt / sweeps))
    g.check_invariants()
    g.close()
    check(idx, "%s K=%d n=%d %s" % (scheme, fx.K, n, env or "default plan"), cpu_histogram(scheme, fx.K, n) if parity else None, n)


STREAM_FORMS = [({"GGS_DEBUG_ZKERNEL": "2"}, STREAM1), ({"GGS_DEBUG_ZKERNEL": "3"}, STREAM2),
                ({"GGS_DEBUG_ZKERNEL": "2", "GGS_DEBUG_MARGIN": "1e13"}, STREAM1)]     # the last: the exact replay carries the chain


def ids(forms):
    return ["-".join("%s=%s" % (k[len("GGS_DEBUG_"):], v) for k, v in e.items()) or "default" for e, _ in forms]


# Fixture A has three words, and by default all three sit in the hot table (one fused kernel, every row from LDS).  The forms
# below send the tokens through the other score-register paths: no hot word = every token scored by the cold kernel from its
# float32 rows; one hot word and the split form = z_hot_kernel beside the cold kernel, its walk decided by the margin
# argument, and with the margin scaled by 1e13 by its exact replay.
NO_HOT = {"GGS_DEBUG_HOT": "0"}
SPLIT = {"GGS_DEBUG_HOT": "1", "GGS_DEBUG_SPLIT": "2"}
SPLIT_REPLAY = dict(SPLIT, GGS_DEBUG_MARGIN="1e13")
SLICED_FORMS = [(NO_HOT, SLICED), (SPLIT, SLICED), (SPLIT_REPLAY, SLICED)]
A_FORMS = [({}, SLICED), ({"GGS_DEBUG_ZKERNEL": "0"}, TILE)] + STREAM_FORMS + SLICED_FORMS


def sliced_expectation(env):
    if "GGS_DEBUG_HOT" not in env:
        return None
    return {"num_hot": 0, "z_form": "fused"} if env["GGS_DEBUG_HOT"] == "0" else {"num_hot": 1, "z_form": "split"}


@pytest.mark.parametrize("env,kernel", A_FORMS, ids=ids(A_FORMS))
def test_ggs_fixture_a(native, oracle, monkeypatch, env, kernel):
    run_case(native, monkeypatch, A, 0, env, kernel, "ggs", parity=True, expect=sliced_expectation(env),
             may_skip=env.get("GGS_DEBUG_ZKERNEL") in ("2", "3"))


@pytest.mark.parametrize("env,kernel", STREAM_FORMS, ids=ids(STREAM_FORMS))
def test_ggs_fixture_b_at_40_topics_every_streaming_form(native, oracle, monkeypatch, env, kernel):
    """K = 40 is the narrowest padded row the streaming kernels take (more than two 16-topic slices; not a whole number of
    slices): the one-pass kernel, its two-pass cross-check and the one-pass kernel's exact replay (margin scaled by 1e13)
    each carry a whole chain here."""
    run_case(native, monkeypatch, LP.fixture_b(40), 0, env, kernel, "ggs", parity=True)


@pytest.mark.parametrize("K,env,kernel,parity", [(100, {}, SLICED, True), (100, SPLIT, SLICED, True), (200, {}, STREAM1, False), (1024, {}, STREAM1, False)],
                         ids=["B100", "B100-split", "B200", "B1024"])
def test_ggs_fixture_b_wide_rows(native, oracle, monkeypatch, K, env, kernel, parity):
    """K = 100: the score-register kernels over several 16-topic slices (fused by default; the cold kernel and z_hot_kernel
    side by side when forced); K = 200 and 1024: the one-pass streaming kernel with one and with four slices per checkpoint
    group, by default.  No CPU chain at K = 200 and 1024: the oracle needs 12 s and 63 s for it."""
    run_case(native, monkeypatch, LP.fixture_b(K), 0, env, kernel, "ggs", parity, expect=sliced_expectation(env))


@pytest.mark.parametrize("K,env,kernel,parity", [(3, {}, LANE, True), (3, {"GGS_DEBUG_PCGS_WAVE": "1"}, WAVE, True), (100, {}, LANE, True),
                                                 (200, {}, WAVE, True), (1024, {}, WAVE, False)], ids=["A", "A-wave", "B100", "B200", "B1024"])
def test_pcgs(native, oracle, monkeypatch, K, env, kernel, parity):
    run_case(native, monkeypatch, A if K == 3 else LP.fixture_b(K), native.FLAG_PCGS, env, kernel, "pcgs", parity)


@pytest.mark.parametrize("env,kernel", [({}, LANE), ({"GGS_DEBUG_PCGS_WAVE": "1"}, WAVE)], ids=["lane", "wave"])
def test_pcgs_longer_chain(native, oracle, monkeypatch, env, kernel):
    """n = LP.N_LONG = 12000 samples: the n at which a walk that lands one topic late for 3 % of the tokens is rejected in the
    pcgs sampler (tests/test_posterior_model.py; n = 4000 does not see it there), for both pcgs kernels."""
    run_case(native, monkeypatch, A, native.FLAG_PCGS, env, kernel, "pcgs", parity=True, n=LP.N_LONG)


@pytest.mark.parametrize("K,parity", [(3, True), (1024, False)], ids=["A", "B1024"])
def test_spalias(native, oracle, monkeypatch, K, parity):
    """The one-token document has an empty list of non-zero topics: every draw of its token comes from the alias table."""
    run_case(native, monkeypatch, A if K == 3 else LP.fixture_b(K), native.FLAG_SPALIAS, {}, SPALIAS, "spalias", parity)


def test_serial_collapsed_chain(native, oracle, monkeypatch):
    run_case(native, monkeypatch, A, native.FLAG_COLLAPSED, {}, None, "collapsed", parity=True)


def test_ggs_device_side_means_of_phi_and_theta(native, monkeypatch):
    """GGS_FLAG_SAVE_PHI_MEAN: the running mean the Phi kernel keeps, read every 500 sweeps and differenced into 40 batch
    means, against the enumerated E[phi | w]; theta read every sweep, against E[theta | w].  18 entries: |z| < 4.5 holds for
    a correct chain with probability 1 - 1e-4 (tests/test_posterior_model.py shows a doubled beta fails it)."""
    batches, per = 40, 500
    g = make_handle(native, monkeypatch, A, native.FLAG_SAVE_PHI_MEAN, {}, SLICED)
    g.sweep(BURN_IN)                                                # the phi mean starts behind phi_burn_in = BURN_IN
    assert g.get_phi_mean()[1] == 0
    theta, phi_bm, before = [], [], np.zeros((A.K, A.V))
    for b in range(batches):
        for _ in range(per):
            g.sweep(1)
            theta.append(g.get_theta())
        mean, n = g.get_phi_mean()
        assert n == (b + 1) * per
        phi_bm.append((mean * n - before) / per)
        before = mean * n
    g.close()
    post = posterior()
    zt = LP.batch_means_z(theta, post.e_theta, batches)
    zp = LP.batch_means_z(phi_bm, post.e_phi, batches)
    print("device ggs: max |z| of the theta means %.2f, of the phi means %.2f" % (np.abs(zt).max(), np.abs(zp).max()))
    assert np.abs(zp).max() < Z_BAR, zp
    assert np.abs(zt).max() < Z_BAR, zt
