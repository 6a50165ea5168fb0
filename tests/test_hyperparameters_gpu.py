"""Mutable hyperparameters and the optimisation step on the device: ggs_set_hyperparameters makes a handle the handle of other
alpha, beta and betaSum (for every row of the scheme table: bit-identical to a fresh handle of the new values given the exported
state), refuses what it must and changes nothing when it refuses; the drivers (Python, C++, doc-sharded) run the step of
UPLDA:891-894 and end on the bits of a loop written out here over a bare handle, numpy histograms and the Python restatement of the
estimators."""
import os
import subprocess

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.sharded import NativeExchange, ShardedGGS
from tests import handle_lifecycle as HL
from tests import hyperparameter_restatement as R
from tests.ranks import Transport, assert_bit_equal, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 8
# the rows of kSchemes (tests/scheme_table_cases.py lists the schemes; tests/handle_lifecycle.py says what each one's state is), spalias
# with priors, and the twelfth flag, lightpcldaw2: Phi is drawn, the tables and lists are over the counts
ROWS = HL.ROWS + (HL.Row("lightpcldaw2", "lightpcldaw2", 0.05, "phi", "", HL.PHI, tables=True, lists=True, mh=True),)
ROW = {r.name: r for r in ROWS}


def _flags(native, row):
    return native.FLAG_LIGHTPCLDAW2 if row.scheme == "lightpcldaw2" else native.SCHEME_FLAGS[row.scheme]


def create(native, row, alpha, beta, k=K):
    """HL.create with the hyperparameters of the caller's choice"""
    h = native.GGSHandle(k, HL.V, alpha, beta, HL.SEED, flags=_flags(native, row) | native.FLAG_SAVE_PHI_MEAN, phi_burn_in=HL.BURN_IN, phi_mean_thin=HL.THIN)
    try:
        if row.priors:
            h.set_topic_priors(*HL.prior_cells(k))
        if row.vs:
            h.set_variable_selection_prior(HL.VS_PI)
    except BaseException:
        h.close()
        raise
    return h


def small_corpus():
    """a few hundred tokens: 48 documents of 0 .. 19 tokens, more documents than the score-register kernels' D >= V asks for is not
    needed (GGS_DEBUG_THETA_MAIN=2 takes the theta draw to the handle's stream whatever D and V are)"""
    c = HL._corpus(np.random.default_rng(21).permutation(np.arange(48) % 20), 22)
    assert 300 < c.num_tokens < 600 and (np.diff(c.doc_ptr) == 0).any()
    return c


def new_values(row, k=K):
    return np.linspace(0.03, 0.45, k) * (1.0 + 0.1 * (np.arange(k) % 3)), row.beta * 1.75


def counters_of(snap):
    return {n: np.asarray(snap[n], np.int64) for n in HL.CUMULATIVE if n in snap}


CASES = [(r.name, K, None) for r in ROWS] + [("ggs", K, "2"), ("ggs", K, "0"), ("ggs", 200, None), ("pcgs", 200, None)]


@pytest.mark.parametrize("name,k,theta_main", CASES)
def test_setter_equals_a_fresh_handle_of_the_new_values(native, oracle, monkeypatch, name, k, theta_main):
    """A: (a0, b0), two sweeps, the setter, two sweeps.  B: created with (a1, b1), given A's z, Phi and iteration at the switch, two
    sweeps.  Everything the getters return is the same, bit for bit; the cumulative counters by what they grew since the switch.
    scheme ggs: a theta for the next iteration was drawn ahead under a0 when the setter came (on the side stream; with
    GGS_DEBUG_THETA_MAIN=2 on the handle's own): it must be dropped."""
    row = ROW[name]
    monkeypatch.delenv("GGS_DEBUG_THETA_MAIN", raising=False)
    if theta_main is not None:
        monkeypatch.setenv("GGS_DEBUG_THETA_MAIN", theta_main)
    c = small_corpus()
    a1, b1 = new_values(row, k)
    A = create(native, row, HL.ALPHA, row.beta, k)
    B = create(native, row, a1, b1, k)
    try:
        HL.start(A, c, HL.initial_z(c, k))
        A.sweep(2)
        state = HL.export_state(A, row)
        before = counters_of(HL.snapshot(A, row))
        a_old, b_old, bs_old = A.hyperparameters()
        assert_bit_equal(a_old, np.full(k, HL.ALPHA), "alpha at creation")
        assert b_old == row.beta and bs_old == row.beta * HL.V
        A.set_hyperparameters(a1, b1, 0.0)
        a_now, b_now, bs_now = A.hyperparameters()
        assert_bit_equal(a_now, a1, "alpha after the setter")
        assert b_now == b1 and bs_now == b1 * HL.V
        A.sweep(2)
        B.set_corpus(c.doc_ptr, c.tokens)
        HL.restore(B, row, state)
        B.sweep(2)
        sa, sb = HL.snapshot(A, row), HL.snapshot(B, row)
        HL.assert_same(sa, sb, "%s K=%d" % (name, k), skip=HL.CUMULATIVE + HL.OWN)
        for n, at_switch in before.items():
            assert_bit_equal(np.asarray(sa[n], np.int64) - at_switch, np.asarray(sb[n], np.int64), "%s: %s since the switch" % (name, n))
        assert sa["iteration"] == 4
        # ... and the new values did change the chain: the uninterrupted one is another
        U = create(native, row, HL.ALPHA, row.beta, k)
        try:
            HL.start(U, c, HL.initial_z(c, k))
            U.sweep(4)
            assert not np.array_equal(U.get_z(), sa["z"])
        finally:
            U.close()
    finally:
        A.close()
        B.close()


@pytest.mark.parametrize("name", [r.name for r in ROWS])
def test_setter_at_birth_changes_nothing(native, oracle, name):
    """the creation values set again directly after ggs_create: the run of a handle that was never told"""
    row = ROW[name]
    c = small_corpus()
    snaps = []
    for told in (True, False):
        h = create(native, row, HL.ALPHA, row.beta)
        try:
            if told:
                h.set_hyperparameters(np.full(K, HL.ALPHA), row.beta, 0.0)
            HL.start(h, c, HL.initial_z(c, K))
            h.sweep(3)
            snaps.append(HL.snapshot(h, row))
            a, b, bs = h.hyperparameters()
            assert_bit_equal(a, np.full(K, HL.ALPHA), "alpha")
            assert b == row.beta and bs == row.beta * HL.V
        finally:
            h.close()
    HL.assert_same(snaps[0], snaps[1], name)


def test_beta_sum_is_the_java_field(native, oracle):
    """collapsed: ggs_get_phi is (beta + n_wk) / (betaSum + n_k) with the betaSum that was set, not beta * V"""
    row = ROW["collapsed"]
    c = small_corpus()
    h = create(native, row, HL.ALPHA, row.beta)
    try:
        HL.start(h, c, HL.initial_z(c, K))
        h.sweep(1)
        beta = 0.07
        bs = beta * HL.V * 1.0000001 + 0.003
        assert bs != beta * HL.V
        h.set_hyperparameters(None, beta, bs)
        a, b, got_bs = h.hyperparameters()
        assert_bit_equal(a, np.full(K, HL.ALPHA), "alpha kept")
        assert b == beta and got_bs == bs
        n_wk, n_k = h.get_type_topic_counts().astype(np.float64), h.get_topic_totals().astype(np.float64)
        assert_bit_equal(h.get_phi(), np.ascontiguousarray(((beta + n_wk) / (bs + n_k)).T), "phi")
        h.set_hyperparameters(None, beta, 0.0)                                   # 0.0: beta * V again
        assert h.hyperparameters()[2] == beta * HL.V
        assert_bit_equal(h.get_phi(), np.ascontiguousarray(((beta + n_wk) / (beta * HL.V + n_k)).T), "phi, beta * V")
        h.sweep(1)
    finally:
        h.close()


BAD = [("alpha", np.nan), ("alpha", np.inf), ("alpha", 0.0), ("alpha", -0.1), ("beta", np.nan), ("beta", np.inf), ("beta", 0.0), ("beta", -1.0),
       ("beta_sum", np.nan), ("beta_sum", np.inf), ("beta_sum", -2.0)]


@pytest.mark.parametrize("name", ["ggs", "polyaurn_sparse", "adlda"])
def test_refusals_leave_the_handle_untouched(native, oracle, name):
    row = ROW[name]
    c = small_corpus()
    snaps = []
    for molested in (True, False):
        h = create(native, row, HL.ALPHA, row.beta)
        try:
            HL.start(h, c, HL.initial_z(c, K))
            h.sweep(1)
            if molested:
                for what, v in BAD:
                    alpha = np.full(K, 0.3)
                    if what == "alpha":
                        alpha[K - 2] = v
                    with pytest.raises(native.GGSError) as e:
                        h.set_hyperparameters(alpha, v if what == "beta" else 0.2, v if what == "beta_sum" else 0.0)
                    assert e.value.code == native.ERR_BAD_ARG, (what, v)
                    a, b, bs = h.hyperparameters()
                    assert_bit_equal(a, np.full(K, HL.ALPHA), "alpha after a refused %s=%r" % (what, v))
                    assert b == row.beta and bs == row.beta * HL.V
            h.sweep_begin()
            if molested:
                with pytest.raises(native.GGSError) as e:
                    h.set_hyperparameters(np.full(K, 0.3), 0.2, 0.0)
                assert e.value.code == native.ERR_STATE
                assert h.hyperparameters()[1] == row.beta
            h.sweep_end()
            h.sweep(1)
            snaps.append(HL.snapshot(h, row))
        finally:
            h.close()
    HL.assert_same(snaps[0], snaps[1], name)


# ---- the driver -------------------------------------------------------------------------------------------------------------------
def bare_loop(native, scheme, c, k, alpha0, beta0, seed, iterations, interval, symmetric):
    """UPLDA:645-930 with the step of :891-894, written out: the sweep, numpy histograms of get_z() and the counts, the Python
    restatement of the estimators, the setter."""
    h = native.GGSHandle(k, c.num_types, np.full(k, alpha0), beta0, seed, flags=native.SCHEME_FLAGS[scheme])
    try:
        h.set_corpus(c.doc_ptr, c.tokens)
        h.init_z_java_lcg(seed)
        h.init_phi()
        alpha, alpha_sum, beta, beta_sum = [alpha0] * k, alpha0 * k, beta0, h.hyperparameters()[2]
        for it in range(1, iterations + 1):
            h.sweep_begin()
            h.sweep_end()
            if interval > 1 and it % interval == 0:
                alpha, alpha_sum, beta, beta_sum = R.optimize(alpha, alpha_sum, beta_sum, symmetric, c.doc_ptr, c.tokens, c.num_types, h.get_z(),
                                                              h.get_type_topic_counts(), h.get_topic_totals())
                h.set_hyperparameters(np.asarray(alpha), beta, beta_sum)
        return dict(alpha=np.asarray(alpha), alpha_sum=alpha_sum, beta=beta, beta_sum=beta_sum, z=h.get_z(), phi=h.get_phi())
    finally:
        h.close()


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("k", [3, 20])
@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "polyaurn"])
def test_driver_runs_the_step_of_the_reference(native, cats, scheme, k, symmetric):
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    alpha0, beta0, seed = 0.5, 0.05, 4711
    m = create_model(SimpleLDAConfiguration(scheme=scheme, topics=k, alpha=alpha0, beta=beta0, seed=seed, iterations=6, exec_time=1800,
                                            hyperparam_optim_interval=2, symmetric_alpha=symmetric))
    m.setRandomSeed(seed)
    m.addInstances(cats)
    m.sample(6)
    want = bare_loop(native, scheme, cats, k, alpha0, beta0, seed, 6, 2, symmetric)
    assert_bit_equal(m.getAlpha(), want["alpha"], "alpha")
    assert_bit_equal(np.float64(m.alphaSum), np.float64(want["alpha_sum"]), "alphaSum")
    assert_bit_equal(np.float64(m.getBeta()), np.float64(want["beta"]), "beta")
    assert_bit_equal(np.float64(m.betaSum), np.float64(want["beta_sum"]), "betaSum")
    a, b, bs = m._h.hyperparameters()                                            # and the handle's are the sampler's
    assert_bit_equal(a, want["alpha"], "the handle's alpha")
    assert b == want["beta"] and bs == want["beta_sum"]
    assert_bit_equal(np.concatenate(m.getZIndicators()), want["z"], "z")
    assert_bit_equal(m.getPhi(), want["phi"], "phi")
    assert not np.any(want["alpha"] == alpha0) and want["beta"] != beta0, "alpha and beta must have moved"
    if symmetric:
        assert np.unique(want["alpha"]).size == 1
    else:
        assert np.unique(want["alpha"]).size > 1
    est = m.getThetaEstimate()                                                   # the getters see the new alpha
    n_d0 = np.bincount(m.getZIndicators()[0], minlength=k)
    assert_bit_equal(est[0], (n_d0 + want["alpha"]) / float(np.cumsum(n_d0 + want["alpha"])[-1]), "theta estimate")


def test_interval_one_and_the_count_form_classes_never_optimise(native, cats):
    from ldagroupedgibbssampler_amd.sampler import ADLDA, SimpleLDAConfiguration, create_model
    for scheme, interval in (("ggs", 1), ("ggs", 0), ("ggs", -1), ("collapsed", 2), ("lightcollapsed", 2), ("adlda", 2)):
        cfg = SimpleLDAConfiguration(scheme=scheme if scheme != "adlda" else "ggs", topics=3, alpha=0.5, beta=0.05, seed=5, iterations=4, exec_time=1800,
                                     hyperparam_optim_interval=interval)
        m = ADLDA(cfg) if scheme == "adlda" else create_model(cfg)
        m.setRandomSeed(5)
        m.addInstances(cats)
        m.sample(4)
        a, b, bs = m._h.hyperparameters()
        assert (a == 0.5).all() and b == 0.05 and bs == 0.05 * cats.num_types and (m.getAlpha() == 0.5).all() and m.getBeta() == 0.05, (scheme, interval)


# ---- two ranks --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,symmetric", [("ggs", False), ("pcgs", True), ("adlda", False)])
def test_two_ranks_equal_one_handle(native, oracle, name, symmetric):
    """The ranks' document histograms summed, and each rank's cell histogram, are one handle's over the whole corpus; after the same
    setter call on both ranks two sweeps are one handle's; and ShardedGGS.optimize_hyperparameters ends on one handle's step."""
    row = ROW[name]
    whole = HL.corpus("A")
    z0 = HL.initial_z(whole, K)
    a1, b1 = new_values(row)
    bs1 = b1 * HL.V * 1.01
    n_bins = int(np.diff(whole.doc_ptr).max()) + 1
    m = R.max_type_count(whole.tokens, HL.V)
    side = Transport(2)                                                          # the `gather` of ShardedGGS among the ranks' threads
    sharded = {}

    def through(h, attach, rank):
        def exchange_factory(engine):
            attach(engine)
            return NativeExchange()
        sharded[rank] = ShardedGGS(h, exchange_factory, whole, rank, 2)

    def body(h, rank, sub, tok_base):
        sh = sharded[rank]
        sh.set_z_global(z0)
        sh.sweep(1)
        out = dict(doc=h.doc_topic_histogram(symmetric, n_bins), cell=h.type_topic_count_histogram(m + 1))
        h.set_hyperparameters(a1, b1, bs1)
        sh.sweep(2)
        out["mid"] = dict(z=h.get_z(), phi=h.get_phi(), n_wk=h.get_type_topic_counts())
        out["learned"] = sh.optimize_hyperparameters(symmetric, gather=lambda a: side.exchange(rank, a))
        out["handle"] = h.hyperparameters()
        sh.sweep(1)
        out["end"] = dict(z=h.get_z(), phi=h.get_phi())
        return out

    out = run_ranks(2, whole, lambda rank: HL.create(native, row, K), body, mode="dense", through=through)
    h = HL.create(native, row, K)
    try:
        HL.start(h, whole, z0)
        h.sweep(1)
        doc, lengths = h.doc_topic_histogram(symmetric, n_bins)
        assert_bit_equal(out[0]["doc"][0].astype(np.int64) + out[1]["doc"][0], doc.astype(np.int64), "document histograms, summed")
        assert_bit_equal(out[0]["doc"][1] + out[1]["doc"][1], lengths, "length histograms, summed")
        assert_bit_equal(doc, R.doc_topic_histogram(whole.doc_ptr, h.get_z(), K, symmetric, n_bins), "one handle against numpy")
        cell = h.type_topic_count_histogram(m + 1)
        for r in range(2):
            assert_bit_equal(out[r]["cell"], cell, "cell histogram of rank %d" % r)
        h.set_hyperparameters(a1, b1, bs1)
        h.sweep(2)
        assert_bit_equal(np.concatenate([out[r]["mid"]["z"] for r in range(2)]), h.get_z(), "z two sweeps after the setter")
        for r in range(2):
            assert_bit_equal(out[r]["mid"]["phi"], h.get_phi(), "phi of rank %d" % r)
            assert_bit_equal(out[r]["mid"]["n_wk"], h.get_type_topic_counts(), "counts of rank %d" % r)
        alpha_sum = 0.0
        for a in a1.tolist():
            alpha_sum += a
        alpha, _, beta, beta_sum = R.optimize(a1, alpha_sum, bs1, symmetric, whole.doc_ptr, whole.tokens, HL.V, h.get_z(), h.get_type_topic_counts(),
                                              h.get_topic_totals())
        h.set_hyperparameters(np.asarray(alpha), beta, beta_sum)
        h.sweep(1)
        for r in range(2):
            la, lb, lbs = out[r]["learned"]
            assert_bit_equal(la, np.asarray(alpha), "alpha learned on rank %d" % r)
            assert lb == beta and lbs == beta_sum
            ha, hb, hbs = out[r]["handle"]
            assert_bit_equal(ha, np.asarray(alpha), "alpha of rank %d's handle" % r)
            assert hb == beta and hbs == beta_sum
            assert_bit_equal(out[r]["end"]["phi"], h.get_phi(), "phi after the learned values, rank %d" % r)
        assert_bit_equal(np.concatenate([out[r]["end"]["z"] for r in range(2)]), h.get_z(), "z after the learned values")
    finally:
        h.close()


# ---- the C++ mirror ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,symmetric", [("ggs", False), ("pcgs", True), ("polyaurn", False)])
def test_cpp_mirror_learns_the_python_samplers_bits(native, cats, tmp_path, scheme, symmetric):
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    exe = os.path.join(ROOT, "examples", "ggs_host_demo")
    if not os.path.exists(exe):
        pytest.fail("examples/ggs_host_demo is not built: run __graft_entry__.build()")
    path = os.path.join(str(tmp_path), "corpus.txt")
    with open(path, "w") as f:
        f.write("%d %d\n" % (cats.num_docs, cats.num_types))
        for d in range(cats.num_docs):
            t = cats.tokens[cats.doc_ptr[d]:cats.doc_ptr[d + 1]]
            f.write(" ".join([str(len(t))] + [str(int(x)) for x in t]) + "\n")
    k, alpha0, beta0, seed, its, interval = 5, 0.5, 0.1, 99, 4, 2
    out = subprocess.run([exe, path, str(k), str(alpha0), str(beta0), str(seed), str(its), "", scheme, str(interval), "1" if symmetric else "0"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = dict(l.split(" ", 1) for l in out.stdout.strip().splitlines())
    m = create_model(SimpleLDAConfiguration(scheme=scheme, topics=k, alpha=alpha0, beta=beta0, seed=seed, iterations=its, exec_time=1800, paranoid=True,
                                            hyperparam_optim_interval=interval, symmetric_alpha=symmetric))
    m.setRandomSeed(seed)
    m.addInstances(cats)
    m.sample(its)
    assert_bit_equal(np.array([float.fromhex(x) for x in lines["alpha"].split()]), m.getAlpha(), "alpha")
    assert_bit_equal(np.float64(float.fromhex(lines["alphasum"])), np.float64(m.alphaSum), "alphaSum")
    assert_bit_equal(np.float64(float.fromhex(lines["beta"])), np.float64(m.getBeta()), "beta")
    assert_bit_equal(np.float64(float.fromhex(lines["betasum"])), np.float64(m.betaSum), "betaSum")
    assert np.array_equal(np.array(lines["z"].split(), np.int32), np.concatenate(m.getZIndicators()))
    assert not np.any(m.getAlpha() == alpha0) and m.getBeta() != beta0
    assert lines["iteration"] == "%d hooks %d %d" % (its, its, its)


# ---- the example ------------------------------------------------------------------------------------------------------------------
def test_run_dataset_learns_and_writes_the_hyperparameters(tmp_path):
    """examples/run_dataset.py --optimize-interval N --symmetric-alpha: the final alpha and beta are printed and written beside the
    other outputs"""
    import sys
    out = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt"),
                        "--scheme", "pcgs", "--topics", "4", "--alpha", "0.5", "--beta", "0.05", "--iterations", "4", "--optimize-interval", "2",
                        "--symmetric-alpha", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "alpha: " in r.stdout and "beta: " in r.stdout
    rows = [l.split("\t") for l in open(os.path.join(out, "hyperparameters.txt")).read().splitlines()]
    alpha = [float(x[2]) for x in rows if x[0] == "alpha"]
    beta = [float(x[1]) for x in rows if x[0] == "beta"][0]
    beta_sum = [float(x[1]) for x in rows if x[0] == "betaSum"][0]
    assert len(alpha) == 4 and len(set(alpha)) == 1 and alpha[0] != 0.5 and alpha[0] > 0       # symmetric, and it moved
    assert beta != 0.05 and beta > 0 and beta_sum > beta
