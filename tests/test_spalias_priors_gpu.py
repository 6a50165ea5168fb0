"""scheme=spalias_priors on the device (ggs_set_topic_priors on a GGS_FLAG_SPALIAS handle): whole runs bit for bit against the CPU
restatement (tests/spalias_priors_restatement.py) -- z after every sweep, then counts, Phi, alias tables and the priors read back
-- on cats, on the reference test's own fixture, at the 1e-4 clamp, at the shape edges of the masked draw, with the phi mean,
through ggs_set_phi, sharded over an exchange, and the misuse the C-ABI refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import priors
from ldagroupedgibbssampler_amd.corpus import random_corpus
from ldagroupedgibbssampler_amd.sharded import NativeExchange, ShardedGGS, java_lcg_initial_z
from tests import spalias_priors_restatement as PR
from tests.ranks import assert_bit_equal, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "datasets")
PRIORS = os.path.join(ROOT, "tests", "golden", "priors")
SEED = 777
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32))


def run_pair(native, c, K, alpha, beta, sweeps, cells, zseed=5, flags=0, burn_in=0, thin=1, each_sweep=None):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_SPALIAS | native.FLAG_PARANOID | flags, phi_burn_in=burn_in,
                         phi_mean_thin=thin)
    g.set_topic_priors(*cells)                                      # before the corpus: either order is legal
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = PR.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, cells=cells, save_phi_mean=bool(flags & native.FLAG_SAVE_PHI_MEAN),
                 phi_burn_in=burn_in, phi_thin=thin)
    m.init_phi()
    assert_bit_equal(g.get_topic_priors(), m.P, "topic priors")
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
        if each_sweep:
            each_sweep(g, m, s + 1)
    assert g.launch_info()["z_kernel"].startswith("spalias_wave_kernel")
    assert_bit_equal(g.get_type_topic_counts(), m.counts(), "n_wk")
    phi = g.get_phi()
    assert_bit_equal(phi, m.phi, "phi")
    assert (phi[m.P == 0.0] == 0.0).all() and not np.signbit(phi[m.P == 0.0]).any()
    ps, a, tn = g.alias_tables()
    assert_bit_equal(tn, m.tables[2], "typeNorm after the last sweep")
    assert_bit_equal(a, m.tables[1], "a after the last sweep")
    assert_bit_equal(ps, m.tables[0], "ps after the last sweep")
    assert_bit_equal(g.get_topic_priors(), m.P, "topic priors after the run")
    return g, m


# ---- (a) cats -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, K, alpha, beta):
    cells = PR.random_cells(np.random.default_rng(K), K, cats.num_types, 10, 20, np.bincount(cats.tokens, minlength=cats.num_types))
    g, m = run_pair(native, cats, K, alpha, beta, 4, cells)
    assert 0 < m.n_prior < 4 * cats.num_tokens                      # both branches of the z step are taken
    g.close()


def test_an_empty_cell_list_takes_the_conditional_draw(native, oracle):
    """n_zero == 0: an all-ones matrix, the restatement's conditional Phi -- not plain spalias's"""
    c = random_corpus(80, 130, 40, seed=2, empty_every=9)
    g, m = run_pair(native, c, 7, 0.1, 0.01, 2, NONE)
    assert (g.get_topic_priors() == 1.0).all()
    p = native.GGSHandle(7, c.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS)
    assert (p.get_topic_priors() == 1.0).all()                      # without the call: all 1.0
    p.set_corpus(c.doc_ptr, c.tokens)
    p.init_z_java_lcg(5)
    p.init_phi()
    p.sweep(2)
    assert not np.array_equal(p.get_phi().view(np.int64), g.get_phi().view(np.int64))
    p.close()
    g.close()


# ---- (b) the reference test's fixture ---------------------------------------------------------------------------------------
def test_small_texts_through_create_model(native, oracle):
    """SpaliasUncollapsedTestPhiPriors.testSetPriors: K = 4, alpha 0.1, beta 0.01, seed 4711, 100 iterations"""
    from ldagroupedgibbssampler_amd import sampler
    from ldagroupedgibbssampler_amd.frontend import load_dataset
    c = load_dataset(os.path.join(DATA, "SmallTexts.txt"), stoplist=os.path.join(DATA, "stoplist.txt")).corpus
    path = os.path.join(PRIORS, "topic_priors_SmallTexts.txt")
    cfg = sampler.SimpleLDAConfiguration(scheme="spalias_priors", topics=4, alpha=0.1, beta=0.01, iterations=100, seed=4711, exec_time=None,
                                         topic_prior_filename=path)
    model = sampler.create_model(cfg)
    assert type(model) is sampler.SpaliasUncollapsedParallelWithPriors and isinstance(model, sampler.SpaliasUncollapsedParallelLDA)
    model.setRandomSeed(cfg.get_seed())
    model.addInstances(c)
    v = {w: i for i, w in enumerate(c.vocab)}
    P = model.getTopicPriors()
    for w, keep in (("mother", 0), ("slip", 0), ("disk", 3), ("drive", 3)):
        assert P[keep, v[w]] == 1.0 and (np.delete(P[:, v[w]], keep) == 0.0).all()
    m = PR.Model(4, c.num_types, 0.1, 0.01, 4711, c.doc_ptr, c.tokens, java_lcg_initial_z(c.num_tokens, 4, 4711),
                 cells=priors.load_zero_cells(path, 4, c.vocab))
    m.init_phi()
    assert_bit_equal(model.getPhi(), m.phi, "initial phi")
    model.sample(100)
    m.sweep(100)
    assert model.getCurrentIteration() == 100
    phi = np.asarray(model.getPhi())
    z = np.concatenate(model.getZIndicators())
    for w, keep in (("mother", 0), ("slip", 0), ("disk", 3), ("drive", 3)):
        zeros = np.delete(phi[:, v[w]], keep)
        assert (zeros == 0.0).all() and not np.signbit(zeros).any()  # the reference test's twelve posterior cells, exactly
        assert (z[c.tokens == v[w]] == keep).all(), "a token of %r outside topic %d" % (w, keep)
    assert_bit_equal(z, m.z.astype(np.int32), "z")
    assert_bit_equal(phi, m.phi, "phi")
    # no file named: spalias
    cfg2 = sampler.SimpleLDAConfiguration(scheme="spalias_priors", topics=4, alpha=0.1, beta=0.01, iterations=3, seed=4711, exec_time=None)
    plain, ref = sampler.create_model(cfg2), sampler.create_model(cfg2, "spalias")
    for s in (plain, ref):
        s.setRandomSeed(4711)
        s.addInstances(c)
        s.sample(3)
    assert (plain.getTopicPriors() == 1.0).all()
    assert_bit_equal(plain.getPhi(), ref.getPhi(), "phi without a priors file")


# ---- (c) the clamp ------------------------------------------------------------------------------------------------------
def test_the_clamp_at_a_tiny_beta(native, oracle):
    """beta = 0.001: about half of a topic's empty cells draw a gamma of exactly 0 and are set to 1e-4 before the sums -- the
    gammas' sums run far ahead of the magnitudes' running sums that guess them, so the exact sum takes its fallback"""
    K, V = 8, 130
    c = random_corpus(50, V, 30, seed=4, empty_every=8)
    cells = PR.random_cells(np.random.default_rng(4), K, V, 6, 12)

    def both_kinds(g, m, sweep):
        assert (m.clamped > 0).all() and (m.unclamped > 0).all(), "sweep %d: clamped %s, unclamped %s" % (sweep, m.clamped, m.unclamped)
        assert_bit_equal(g.get_phi(), m.phi, "phi after sweep %d" % sweep)

    g, m = run_pair(native, c, K, 0.1, 0.001, 3, cells, each_sweep=both_kinds)
    g.close()


# ---- (d) shape edges of the masked draw -------------------------------------------------------------------------------------
def edge_cells(K, V=130):
    """V = 130: segments of 64, 64 and 2 rows"""
    cells = set()
    cells.update((0, v) for v in range(0, 64))                     # a column with its whole first segment masked
    cells.update((1, v) for v in range(64, 128))                   # ... a whole middle segment
    cells.update((2, v) for v in (128, 129))                       # ... the 2-row tail
    cells.update((3, v) for v in (0, 63, 64, 127, 128))            # the first and the last row of a segment
    cells.update((4, v) for v in range(V) if v != 70)              # a topic with a single allowed word
    cells.update((k, 100) for k in range(K) if k != 5)             # a word allowed in a single topic
    for k in (30, 31, 32, 33, 62, 63, 64):                         # both sides of the bit mask's word boundaries
        if 6 < k < K:
            cells.update((k, v) for v in (5, 63, 129))
    cells = sorted(cells)
    return np.asarray([c[0] for c in cells], np.int32), np.asarray([c[1] for c in cells], np.int32)


@pytest.mark.parametrize("K", [7, 13, 33, 64, 65])
def test_shape_edges_of_the_masked_draw(native, oracle, K):
    """K at the edges of the draw's <= 6-column tiles and of the mask's 32-bit words"""
    c = random_corpus(60, 130, 40, seed=K, empty_every=7)
    g, m = run_pair(native, c, K, 0.1, 0.01, 3, edge_cells(K), each_sweep=lambda g, m, s: assert_bit_equal(g.get_phi(), m.phi, "phi after sweep %d" % s))
    assert (m.P[4] != 0.0).sum() == 1 and (m.P[:, 100] != 0.0).sum() == 1
    g.close()


# ---- (e) the phi mean ---------------------------------------------------------------------------------------------------
def test_phi_mean_with_burn_in_and_thin(native, oracle):
    K, V = 13, 130
    c = random_corpus(60, V, 40, seed=6, empty_every=7)
    g, m = run_pair(native, c, K, 0.1, 0.01, 6, edge_cells(K), flags=native.FLAG_SAVE_PHI_MEAN, burn_in=2, thin=2)
    mean, n = g.get_phi_mean()
    wmean, wn = m.phi_mean()
    assert n == wn == 2
    assert_bit_equal(mean, wmean, "phi mean")
    assert (mean[m.P == 0.0] == 0.0).all()                          # the new rows are added zeros included
    g.close()


# ---- (f) ggs_set_phi ------------------------------------------------------------------------------------------------------
def test_sample_z_given_phi_after_set_phi(native, oracle):
    K, V = 13, 130
    c = random_corpus(60, V, 40, seed=8, empty_every=7)
    cells = edge_cells(K)
    g = native.GGSHandle(K, V, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.set_topic_priors(*cells)                                      # after the corpus
    z0 = java_lcg_initial_z(c.num_tokens, K, 3)
    g.set_z(z0, redraw_phi=False)
    m = PR.Model(K, V, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, z0, cells=cells)
    rng = np.random.default_rng(8)
    phi = rng.gamma(0.3, 1.0, (K, V)) * m.P
    phi /= phi.sum(axis=1, keepdims=True)
    bad = phi.copy()
    bad[1, 64] = 1e-300                                             # a masked cell
    assert m.P[1, 64] == 0.0
    with pytest.raises(native.GGSError) as e:
        g.set_phi(bad)
    assert e.value.code == native.ERR_BAD_ARG
    g.set_phi(phi)
    m.set_phi(phi)
    with pytest.raises(native.GGSError) as e:                       # the handle has a Phi now
        g.set_topic_priors(*cells)
    assert e.value.code == native.ERR_STATE
    g.sample_z_given_phi(2)
    m.sample_z_given_phi(2)
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z given phi")
    assert_bit_equal(g.get_phi(), phi, "phi is the caller's")
    g.close()


# ---- (g) sharded: bit-identical to one handle -------------------------------------------------------------------------------
FLAGS_SHARDED = dict(phi_burn_in=1, phi_mean_thin=2)


def _rank(native, world, whole, K, sweeps, cells):
    """(make_handle, through, body) of a rank for tests/ranks.py's run_ranks: ShardedGGS cuts the shard, attaches through the
    engine it is handed and sets the corpus"""
    sharded = {}

    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)

    def through(h, attach, rank):
        def exchange_factory(engine):
            attach(engine)
            return NativeExchange()
        sharded[rank] = ShardedGGS(h, exchange_factory, whole, rank, world, topic_priors=cells)     # sharded.py hands every rank the same cells

    def body(h, rank, sub, tok_base):
        sh = sharded[rank]
        sh.set_z_global(java_lcg_initial_z(whole.num_tokens, K, 17))
        sh.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(),
                    how=h.count_exchange(), tables=h.alias_tables(), priors=h.get_topic_priors(), info=h.exchange_info())
    return make_handle, through, body


def one_handle(native, whole, K, sweeps, cells):
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_topic_priors(*cells)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    r = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), tables=h.alias_tables(),
             priors=h.get_topic_priors())
    h.close()
    return r


def sharded_case(K, V):
    whole = random_corpus(200, V, 60, seed=K + V, empty_every=9)
    cells = PR.random_cells(np.random.default_rng(K + V), K, V, 10, 20, np.bincount(whole.tokens, minlength=V))
    return whole, cells


# world 2, K = 7: slices of 4 and 3 topics (a padded column), V = 1500: the vocabulary travels in two halves;
# world 3, K = 100, V = 900: one all-gather call; the sparse count exchange
@pytest.mark.parametrize("world,mode,K,V", [(2, "dense", 7, 1500), (3, "dense", 100, 900), (2, "sparse", 40, 1000)])
def test_sharded_runs_equal_one_handle(native, oracle, world, mode, K, V):
    whole, cells = sharded_case(K, V)
    sweeps = 4
    make_handle, through, body = _rank(native, world, whole, K, sweeps, cells)
    out = run_ranks(world, whole, make_handle, body, mode=mode, through=through)
    ref = one_handle(native, whole, K, sweeps, cells)
    masked = ref["priors"] == 0.0
    assert masked.any() and (ref["phi"][masked] == 0.0).all() and ref["phi"][~masked].any()
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert_bit_equal(z, ref["z"], "z")
    if K == 7:
        assert [out[r]["info"]["k_end"] - out[r]["info"]["k_begin"] for r in range(world)] == [4, 3]
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        for key in ("nwk", "nk", "phi", "priors"):
            assert_bit_equal(out[r][key], ref[key], "%s rank %d" % (key, r))
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))


def test_one_rank_through_rccl_and_a_group_of_one(native, oracle):
    K, V, sweeps = 24, 1100, 3
    whole, cells = sharded_case(K, V)
    ref = one_handle(native, whole, K, sweeps, cells)
    z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
    h = native.GGSHandle(K, V, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.attach_rccl(0, 1, native.rccl_unique_id())
    h.set_topic_priors(*cells)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(z0, redraw_phi=True)
    h.sweep(sweeps)
    got = dict(z=h.get_z(), phi=h.get_phi(), nwk=h.get_type_topic_counts(), mean=h.get_phi_mean()[0])
    h.close()
    for k in got:
        assert_bit_equal(got[k], ref[k] if k != "mean" else ref["mean"][0], k)
    # the one-process group entry points go through the same steps
    g = native.GGSGroup(K, V, 0.1, 0.01, SEED, device_ids=[0], flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h = g.handles[0]
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_topic_priors(*cells)
    g.set_z([z0], redraw_phi=True)
    g.sweep(sweeps)
    got = dict(z=h.get_z(), phi=h.get_phi(), nwk=h.get_type_topic_counts(), mean=h.get_phi_mean()[0])
    g.close()
    for k in got:
        assert_bit_equal(got[k], ref[k] if k != "mean" else ref["mean"][0], "group " + k)


# ---- (h) misuse ---------------------------------------------------------------------------------------------------------
def test_misuse_is_rejected(native, oracle):
    K, V = 5, 10
    for flags in (0, native.FLAG_PCGS, native.FLAG_LIGHTPCLDA, native.FLAG_POLYAURN_SPARSE):
        h = native.GGSHandle(K, V, 0.1, 0.01, 1, flags=flags)
        with pytest.raises(native.GGSError) as e:
            h.set_topic_priors([0], [0])
        assert e.value.code == native.ERR_STATE
        with pytest.raises(native.GGSError) as e:
            h.get_topic_priors()
        assert e.value.code == native.ERR_STATE
        h.close()
    c = random_corpus(30, V, 20, seed=1)
    h = native.GGSHandle(K, V, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS)
    good = (np.asarray([0, 0, 4], np.int32), np.asarray([1, 1, 9], np.int32))       # a duplicate is allowed
    h.set_topic_priors(*good)
    want = PR.priors_matrix(K, V, good)
    for t, w in (([K], [0]), ([-1], [0]), ([0], [V]), ([0], [-1]),          # out of range
                 ([2] * V, list(range(V))),                                 # a topic with all V words zero
                 (list(range(K)), [3] * K)):                                # a word with all K topics zero
        with pytest.raises(native.GGSError) as e:
            h.set_topic_priors(t, w)
        assert e.value.code == native.ERR_BAD_ARG
        assert_bit_equal(h.get_topic_priors(), want, "the handle is left as it was")
    later = (np.asarray([1], np.int32), np.asarray([2], np.int32))
    h.set_topic_priors(*later)                                      # a later call replaces the earlier one
    assert_bit_equal(h.get_topic_priors(), PR.priors_matrix(K, V, later), "replaced")
    h.set_topic_priors(*good)
    h.set_corpus(c.doc_ptr, c.tokens)
    h.init_z_java_lcg(5)
    z0 = h.get_z()
    h.init_phi()
    with pytest.raises(native.GGSError) as e:                       # after init_phi
        h.set_topic_priors(*good)
    assert e.value.code == native.ERR_STATE
    h.sweep(2)                                                      # still usable, and still the run the accepted call defines
    m = PR.Model(K, V, 0.1, 0.01, SEED, c.doc_ptr, c.tokens, z0, cells=good)
    m.init_phi()
    m.sweep(2)
    assert_bit_equal(h.get_z(), m.z.astype(np.int32), "z")
    assert_bit_equal(h.get_phi(), m.phi, "phi")
    h.close()


# ---- (i) the driver -----------------------------------------------------------------------------------------------------
def test_run_dataset_writes_the_driver_files(tmp_path):
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), os.path.join(DATA, "SmallTexts.txt"), "--stoplist",
                        os.path.join(DATA, "stoplist.txt"), "--scheme", "spalias_priors", "--topic-priors", os.path.join(PRIORS, "topic_priors_SmallTexts.txt"),
                        "--topics", "4", "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files
