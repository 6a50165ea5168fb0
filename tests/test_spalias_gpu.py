"""scheme=spalias on the device (GGS_FLAG_SPALIAS): the alias tables, whole sweeps, the sparse z step on knife-edge rows
and sharded runs bit for bit against the CPU restatement (tests/spalias_restatement.py) or one handle; the held-out
likelihood against pcgs; the driver and the host mirror end to end.

There is one z kernel, spalias_wave_kernel (a wave per document; DESIGN.md 6c says why no second one), with two ways
through it: the wave scans' proposal, decided outside its margins, and the exact chain that replays what the proposal
leaves open.  GGS_DEBUG_MARGIN=1e30 (FORMS) sends every token through the replay; the tests that force forms run both and
launch_info() names the kernel in every one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus, synthetic_lda_corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import spalias_knife_edge as KE
from tests import spalias_restatement as R
from tests.ranks import assert_bit_equal, run_ranks, z_kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777
DBL_MIN = 2.2250738585072014e-308


FORMS = [None, "1e30"]                  # GGS_DEBUG_MARGIN: the proposal with its margins / every token replayed exactly


def force_form(monkeypatch, margin):
    if margin is None:
        monkeypatch.delenv("GGS_DEBUG_MARGIN", raising=False)
    else:
        monkeypatch.setenv("GGS_DEBUG_MARGIN", margin)


# ---- the tables ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,V", [(3, 300), (20, 300), (100, 250), (1024, 200)])
def test_debug_alias_equals_the_restatement(native, oracle, K, V):
    rng = np.random.default_rng(K)
    phi = rng.gamma(0.3, 1.0, (K, V))
    phi /= phi.sum(axis=1, keepdims=True)
    phi[:, 5:40] *= rng.random((K, 35)) < 0.5                        # columns with zeros
    phi[:, 40:60] = rng.random((K, 20)) * 50 * 4.9e-324 * rng.integers(0, 3, (K, 20))   # sub-DBL_MIN columns, zeros among them
    phi[:, 60:70] = rng.random((K, 10)) * DBL_MIN
    phi[:, 70] = 1e-320                                             # times alpha = 1e-5: the whole column underflows to 0
    phi[0, 71] = 1.0
    phi[1:, 71] = 0.0                                               # a one-hot column
    alpha = np.full(K, 0.1)
    alpha[0] = 1e-5
    phi[1:, 70] = 0.0
    phi[0, 70] = 1e-320
    ps, a, tn = native.debug_alias(phi, alpha)
    wps, wa, wtn = R.alias_tables(phi, alpha)
    assert wtn[70] == 0.0 and (wa[70] == np.arange(K)).all()
    assert_bit_equal(tn, wtn, "typeNorm")
    assert_bit_equal(a, wa, "a")
    assert_bit_equal(ps, wps, "ps")


# ---- whole runs ---------------------------------------------------------------------------------------------------
def run_pair(native, c, K, alpha, beta, sweeps, zseed=5, flags=0, burn_in=0, thin=1):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_SPALIAS | native.FLAG_PARANOID | flags, phi_burn_in=burn_in,
                         phi_mean_thin=thin)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(zseed)
    z0 = g.get_z()
    g.init_phi()
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0, save_phi_mean=bool(flags & native.FLAG_SAVE_PHI_MEAN),
                phi_burn_in=burn_in, phi_thin=thin)
    m.init_phi()
    assert_bit_equal(g.get_phi(), m.phi, "initial phi")
    for s in range(sweeps):
        g.sweep(1)
        m.sweep(1)
        assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after sweep %d" % (s + 1))
    assert z_kernel(g).startswith("spalias_wave_kernel")
    assert_bit_equal(g.get_type_topic_counts(), m.counts(), "n_wk")
    assert_bit_equal(g.get_phi(), m.phi, "phi")
    ps, a, tn = g.alias_tables()
    assert_bit_equal(tn, m.tables[2], "typeNorm after the last sweep")
    assert_bit_equal(a, m.tables[1], "a after the last sweep")
    assert_bit_equal(ps, m.tables[0], "ps after the last sweep")
    return g, m


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, monkeypatch, K, alpha, beta, margin):
    force_form(monkeypatch, margin)
    g, m = run_pair(native, cats, K, alpha, beta, 4)
    assert m.n_prior > 0 and m.n_prior < 4 * cats.num_tokens        # both branches are taken
    g.close()


def test_phi_mean_with_burn_in_and_thin(native, oracle, cats):
    g, m = run_pair(native, cats, 20, 0.1, 0.01, 6, flags=native.FLAG_SAVE_PHI_MEAN, burn_in=2, thin=2)
    mean, n = g.get_phi_mean()
    wmean, wn = m.phi_mean()
    assert n == wn == 2
    assert_bit_equal(mean, wmean, "phi mean")
    g.close()


@pytest.mark.parametrize("margin", FORMS)
def test_empty_and_one_token_documents(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    c = random_corpus(300, 700, 60, seed=9, empty_every=7)
    lens = np.diff(c.doc_ptr)
    assert (lens == 0).any() and (lens == 1).any()
    g, m = run_pair(native, c, 100, 0.1, 0.01, 3)
    g.close()


@pytest.mark.parametrize("margin", FORMS)
def test_lists_longer_than_a_wave_and_than_half_the_topics(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    rng = np.random.default_rng(3)
    lens = np.array([2000, 1, 2000, 0, 70, 2000, 130], np.int64)
    tokens = rng.integers(0, 400, lens.sum()).astype(np.int32)
    c = Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, 400)
    K = 300
    g, m = run_pair(native, c, K, 0.1, 0.01, 2)
    nnz0 = len(set(java_lcg_initial_z(c.num_tokens, K, 5)[:2000].tolist()))
    assert nnz0 > 64 and nnz0 > K // 2                              # the first document's list at the start
    assert m.nnz_sum / (2.0 * c.num_tokens) > 64
    g.close()


@pytest.mark.parametrize("margin", FORMS)
@pytest.mark.parametrize("K", [1024, 4096])
def test_wide_topic_rows_on_a_small_vocabulary(native, oracle, monkeypatch, K, margin):
    force_form(monkeypatch, margin)
    c = random_corpus(40, 60, 150, seed=K, empty_every=11)
    g, m = run_pair(native, c, K, 0.05, 0.01, 2)
    g.close()


def test_one_token_documents_draw_from_the_alias_table(native, oracle):
    K = 9
    c = Corpus(np.arange(41, dtype=np.int64), (np.arange(40) % 6).astype(np.int32), 6)   # 40 documents of one token
    g = native.GGSHandle(K, 6, 0.5, 0.1, SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(1)
    g.init_phi()
    ps, a, tn = g.alias_tables()
    g.sweep(1)
    U = oracle.uniforms(SEED, 1, R.PURPOSE_Z, 0, 40)
    want = np.array([R.alias_sample(ps[w], a[w], float(u)) for w, u in zip(c.tokens, U)], np.int32)   # x = U: the list is empty
    assert_bit_equal(g.get_z(), want, "z of one-token documents")
    g.close()


@pytest.mark.parametrize("margin", FORMS)
def test_one_token_documents_of_a_zeroed_column_keep_their_topic(native, oracle, monkeypatch, margin):
    """The empty list at both typeNorms, K = 3: word 0's Phi column is all zero (typeNorm 0.0: 0 / 0 fails the comparison,
    the token keeps its topic, in the replay whatever the margin), word 1's is not (threshold 1.0: the alias draw at x = U)."""
    force_form(monkeypatch, margin)
    K = 3
    c = Corpus(np.arange(13, dtype=np.int64), (np.arange(12) % 2).astype(np.int32), 2)   # 12 documents of one token
    z0 = (np.arange(12) // 2 % K).astype(np.int32)
    g = native.GGSHandle(K, 2, 0.5, 0.1, SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.set_z(z0, redraw_phi=True)
    phi = g.get_phi()
    phi[:, 0] = 0.0
    g.set_phi(phi)
    g.set_iteration(0)
    g.sample_z_given_phi(1)
    tables = R.alias_tables(phi, 0.5)
    assert tables[2][0] == 0.0 and tables[2][1] > 0.0
    want = z0.astype(np.int64)
    n_prior, nnz_sum = R.z_step(c.doc_ptr, c.tokens, want, phi, tables, SEED, 1)
    assert n_prior == 6 and nnz_sum == 0                            # word 1's six tokens draw from the table, no list has an entry
    z = g.get_z()
    assert_bit_equal(z, want.astype(np.int32), "z of one-token documents")
    assert (z[0::2] == z0[0::2]).all()
    assert z_kernel(g).startswith("spalias_wave_kernel")
    g.close()


# ---- knife-edge rows ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("margin", FORMS)
def test_knife_edge_rows(native, oracle, monkeypatch, margin):
    force_form(monkeypatch, margin)
    ke = KE.KnifeEdge()
    counts, expect, pairs = ke.survey()
    g = native.GGSHandle(KE.K, ke.V, KE.ALPHA, KE.BETA, KE.SEED, flags=native.FLAG_SPALIAS)
    g.set_corpus(ke.doc_ptr, ke.tokens)
    g.set_z(ke.z0, redraw_phi=True)
    by_j = {}
    for j, tok, want, kind, cat in expect:
        by_j.setdefault(j, []).append((tok, want, kind, cat))
    wrong, raised = {}, 0
    for j in range(2 * KE.SCAN + 1):
        g.set_phi(ke.phi(j))
        g.set_z(ke.z0, redraw_phi=False)
        g.set_iteration(KE.ITERATION - 1)
        want_z = ke.restatement_z(j)
        if want_z is None:                                          # x rounds to 1.0 right under the branch's edge
            with pytest.raises(native.GGSError) as e:
                g.sample_z_given_phi(1)
            assert e.value.code == native.ERR_INVALID_TOPIC
            raised += 1
            continue
        g.sample_z_given_phi(1)
        z = g.get_z()
        row_of = {row.target: row for row in ke.rows}
        for tok in np.flatnonzero(z != want_z):
            row = row_of.get(int(tok))
            key = (row.kind, ke.classify(row, j)[0]) if row is not None else ("prefix", "-")
            wrong[key] = wrong.get(key, 0) + 1
        for tok, want, kind, cat in by_j.get(j, ()):
            if z[tok] != want:
                wrong[(kind, cat, "builder")] = wrong.get((kind, cat, "builder"), 0) + 1
    assert z_kernel(g).startswith("spalias_wave_kernel")
    g.close()
    print("knife-edge rows: %s; branch pairs %d; scan values that raise INVALID_TOPIC: %d" % (sorted(counts.items()), pairs, raised))
    assert not wrong, "mismatches by (position, category): %s" % sorted(wrong.items())


# ---- sharded: bit-identical to one handle -------------------------------------------------------------------------
FLAGS_SHARDED = dict(phi_burn_in=1, phi_mean_thin=2)


def _rank(native, whole, K, sweeps):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(sweeps)
        h.check_invariants()
        return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(),
                    how=h.count_exchange(), tables=h.alias_tables(), kernel=z_kernel(h))
    return make_handle, body


def one_handle(native, whole, K, sweeps):
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(sweeps)
    r = dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), tables=h.alias_tables())
    h.close()
    return r


@pytest.mark.parametrize("world,mode,K,V", [(2, "dense", 40, 900), (3, "dense", 100, 2100), (3, "sparse", 100, 900), (2, "sparse", 7, 1500)])
def test_sharded_runs_equal_one_handle(native, oracle, world, mode, K, V):
    whole = random_corpus(310, V, 90, seed=K + V, empty_every=9)
    sweeps = 5
    out = run_ranks(world, whole, *_rank(native, whole, K, sweeps), mode=mode)
    ref = one_handle(native, whole, K, sweeps)
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert z.size == whole.num_tokens
    assert_bit_equal(z, ref["z"], "z")
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        assert out[r]["kernel"].startswith("spalias_wave_kernel")
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], ref["nk"], "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))


def test_one_rank_through_rccl(native, oracle):
    whole = random_corpus(200, 600, 60, seed=31, empty_every=6)
    K = 24
    h = native.GGSHandle(K, whole.num_types, 0.1, 0.01, SEED, flags=native.FLAG_SPALIAS | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.attach_rccl(0, 1, native.rccl_unique_id())
    h.set_corpus(whole.doc_ptr, whole.tokens)
    h.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    h.sweep(3)
    got = dict(z=h.get_z(), phi=h.get_phi(), nwk=h.get_type_topic_counts())
    h.close()
    ref = one_handle(native, whole, K, 3)
    for k in got:
        assert_bit_equal(got[k], ref[k], k)


# ---- statistics ---------------------------------------------------------------------------------------------------
def heldout_after(native, flags, train, test, K, sweeps):
    h = native.GGSHandle(K, train.num_types, 0.1, 0.01, 4711, flags=flags)
    h.set_corpus(train.doc_ptr, train.tokens)
    h.init_z_java_lcg(4711)
    h.init_phi()
    h.sweep(sweeps)
    h.set_test_corpus(test.doc_ptr, test.tokens)
    ll, _ = h.heldout_log_likelihood(100)
    h.close()
    return ll


def test_heldout_likelihood_matches_pcgs(native):
    """spalias and pcgs target the same posterior: the held-out log likelihood after 300 sweeps within 1 % (the bar of
    DESIGN.md 6b).  A wrong split of U between the two branches would show here."""
    full = synthetic_lda_corpus(2200, 2000, 60, true_topics=20, seed=99)
    train, _, _ = full.shard(0, 2000)
    test, _, _ = full.shard(2000, 2200)
    K, sweeps = 20, 300
    sa = heldout_after(native, native.FLAG_SPALIAS, train, test, K, sweeps)
    pc = heldout_after(native, native.FLAG_PCGS, train, test, K, sweeps)
    gap = abs(sa - pc) / abs(pc)
    print("held-out log likelihood after %d sweeps: spalias %.2f, pcgs %.2f, gap %.4f" % (sweeps, sa, pc, gap))
    assert gap < 0.01


# ---- the host mirror and the driver -------------------------------------------------------------------------------
def test_host_mirror_end_to_end(native, cats):
    from ldagroupedgibbssampler_amd import sampler
    cfg = sampler.SimpleLDAConfiguration(scheme="spalias", topics=20, alpha=0.1, beta=0.01, iterations=5, seed=42, exec_time=None)
    m = sampler.create_model(cfg)
    assert type(m) is sampler.SpaliasUncollapsedParallelLDA
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(cats)
    m.sample(5)
    assert m.getCurrentIteration() == 5
    phi = np.asarray(m.getPhi())
    assert phi.shape == (20, cats.num_types) and not np.isnan(phi).any()
    assert np.allclose(phi.sum(axis=1), 1.0)
    assert np.asarray(m.getTypeTopicMatrix()).sum() == cats.num_tokens
    ps, a, tn = m.getAliasTables()
    assert_bit_equal(tn, R.alias_tables(phi, 0.1)[2], "typeNorm of the model's Phi")
    with pytest.raises(NotImplementedError):
        m.getTheta()


def test_run_dataset_writes_the_driver_files(tmp_path):
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--scheme", "spalias", "--topics", "5",
                        "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files


# ---- misuse -------------------------------------------------------------------------------------------------------
def test_misuse_is_rejected(native):
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_SPALIAS | other)
        assert e.value.code == native.ERR_BAD_ARG
    h = native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_PCGS)
    with pytest.raises(native.GGSError) as e:
        h.alias_tables()
    assert e.value.code == native.ERR_STATE
    h.close()
