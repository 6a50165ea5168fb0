"""scheme=lightpcldaw2 on the device (GGS_FLAG_LIGHTPCLDAW2): whole sweeps bit for bit against the CPU restatement
(tests/lightpcldaw2_restatement.py) -- before every sweep the tables (ps / a, type_norm), the words' lists, their lengths and
tokensPerType; after it z, n_wk, n_k, Phi and the three Metropolis-Hastings counters -- on cats and on one synthetic corpus at
every topic count where the kernels take another path; the persistent grids on one CU; sharded runs against one handle;
ggs_set_z to a stored state; the interface.

There are two kernels, count_alias_build_kernel (the lists and tables over the sweep-start counts, at the head of every z step,
unchanged from scheme=lightcollapsed) and lightpcw2_wave_kernel (a wave per document), each with one way through it: no margins,
no replay.  The corpora here are random; every comparison of the token step with its two sides equal or one double apart is in
tests/test_lightpcldaw2_knife_edge_gpu.py."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import lightpcldaw2_restatement as R
from tests import persistent_grid as PG
from tests.ranks import assert_bit_equal, run_ranks, z_kernel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 777
KERNEL = "lightpcw2_wave_kernel"
SWEEPS = 3


def assert_tables_equal(g, tables, what=""):
    """the tables and lists of the current counts: what the next z step builds at its head"""
    ps, a, tn, nw, lists, tpt = tables
    gps, ga, gtn = g.alias_tables()
    gnw, glists = g.word_topic_lists()
    assert_bit_equal(gnw, nw, "nw " + what)
    assert_bit_equal(glists, lists, "lists " + what)
    assert_bit_equal(gtn, tn, "type_norm " + what)
    assert_bit_equal(ga, a, "a " + what)
    assert_bit_equal(gps, ps, "ps " + what)
    # tokensPerType has no getter of its own: it is the row sum of the counts the tables were built from
    assert_bit_equal(g.get_type_topic_counts().sum(axis=1).astype(np.int64), tpt, "tokensPerType " + what)


def snapshot(m):
    return dict(z=m.z.astype(np.int32), nwk=m.counts(), nk=m.topic_totals(), phi=m.phi.copy(), mh=m.stats.copy())


def assert_state_equal(g, want, what=""):
    assert_bit_equal(g.get_z(), want["z"], "z " + what)
    assert_bit_equal(g.mh_stats(), want["mh"], "MH counters " + what)
    assert_bit_equal(g.get_type_topic_counts(), want["nwk"], "n_wk " + what)
    assert_bit_equal(g.get_topic_totals(), want["nk"], "n_k " + what)
    assert_bit_equal(g.get_phi(), want["phi"], "phi " + what)


def reference(c, K, alpha, beta, z0, sweeps=SWEEPS):
    """the restatement's run from z0: (initial Phi, [tables before sweep i], [state after sweep i], the model)"""
    m = R.Model(K, c.num_types, alpha, beta, SEED, c.doc_ptr, c.tokens, z0)
    m.init_phi()
    phi0, before, after = m.phi.copy(), [], []
    for _ in range(sweeps):
        before.append(m.tables())
        m.sweep(1)
        after.append(snapshot(m))
    before.append(m.tables())
    return phi0, before, after, m


def run_against(g, ref, sweeps=SWEEPS):
    """a handle with its corpus, z and initial Phi set, sweep by sweep against a reference()"""
    phi0, before, after, m = ref
    assert_bit_equal(g.get_phi(), phi0, "initial phi")
    for s in range(sweeps):
        assert_tables_equal(g, before[s], "before sweep %d" % (s + 1))
        g.sweep(1)
        assert_state_equal(g, after[s], "after sweep %d" % (s + 1))
    assert_tables_equal(g, before[sweeps], "after the last sweep")
    assert z_kernel(g).startswith(KERNEL)
    assert int(m.stats.sum()) == sweeps * m.tokens.size


# ---- cats ---------------------------------------------------------------------------------------------------------
def run_cats(native, cats, K, alpha, beta):
    g = native.GGSHandle(K, cats.num_types, alpha, beta, SEED, flags=native.FLAG_LIGHTPCLDAW2 | native.FLAG_PARANOID)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    g.init_z_java_lcg(5)
    z0 = g.get_z()
    assert_bit_equal(z0, java_lcg_initial_z(cats.num_tokens, K, 5), "initial z")
    g.init_phi()
    ref = reference(cats, K, alpha, beta, z0)
    run_against(g, ref)
    g.close()
    return ref[3]


@pytest.mark.parametrize("K,alpha,beta", [(3, 5.0, 7.0), (20, 0.1, 0.01)])
def test_cats_sweeps_equal_the_restatement(native, oracle, cats, K, alpha, beta):
    m = run_cats(native, cats, K, alpha, beta)
    print("MH counters %s, word-proposal branches (table, beta) %s" % (m.stats.tolist(), m.branches.tolist()))
    assert (m.stats > 0).all()                                      # all three outcomes occur
    assert (m.branches > 0).all()                                   # and both branches of the word proposal


def test_cats_with_asymmetric_alpha(native, oracle, cats):
    run_cats(native, cats, 20, 0.02 + 0.07 * np.arange(20), 0.01)   # alpha[s] stands where alpha[t] belongs: a wrong index shows


# ---- the synthetic corpus -------------------------------------------------------------------------------------------
V_SYN, ALPHA_SYN, BETA_SYN = 200, 0.05, 0.01
WORD_ONE, WORD_SEAM, WORD_ABSENT = 197, 198, 199                    # one non-zero topic; a list across the 63 / 64 seam; no token
WIDTHS = (1, 2, 64, 65, 130, 1024)


@functools.lru_cache(maxsize=None)
def synthetic():
    """300 documents over V = 200: lengths 0, 1, 63, 64, 65, 129 and 700 (chunk seams; in the long one a document proposal
    reaches an earlier chunk) among 293 of 0 to 30 tokens.  Word 197 has four tokens, word 198 has 150 of the long document's
    tokens and 30 more, word 199 none."""
    rng = np.random.default_rng(2026)
    lens = rng.integers(0, 31, 300)
    lens[[3, 10, 50, 120, 200, 250, 299]] = [700, 0, 1, 63, 64, 65, 129]
    doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    tokens = rng.integers(0, WORD_ONE, int(lens.sum())).astype(np.int32)
    long_doc = np.arange(doc_ptr[3], doc_ptr[4])
    tokens[rng.permutation(long_doc)[:150]] = WORD_SEAM
    others = np.setdiff1d(np.arange(tokens.size), long_doc)
    pick = rng.permutation(others)
    tokens[pick[:30]] = WORD_SEAM
    tokens[pick[30:34]] = WORD_ONE
    c = Corpus(doc_ptr, tokens, V_SYN)
    assert c.num_docs == 300 and (np.bincount(tokens, minlength=V_SYN)[[WORD_ONE, WORD_SEAM, WORD_ABSENT]] == [4, 180, 0]).all()
    return c


def synthetic_z0(K):
    """random topics; word 197 on one topic; word 198 round-robin over min(K, 100) topics"""
    c = synthetic()
    rng = np.random.default_rng(K)
    z = rng.integers(0, K, c.num_tokens).astype(np.int32)
    z[c.tokens == WORD_ONE] = K // 2
    seam = np.flatnonzero(c.tokens == WORD_SEAM)
    z[seam] = (np.arange(seam.size) * 7) % min(K, 100)
    return z


@functools.lru_cache(maxsize=None)
def synthetic_reference(K):
    """computed once per K, shared by the tests below, never written to"""
    c = synthetic()
    ref = reference(c, K, ALPHA_SYN, BETA_SYN, synthetic_z0(K))
    nw0 = ref[1][0][3]
    assert nw0[WORD_ONE] == 1 and nw0[WORD_ABSENT] == 0 and nw0[WORD_SEAM] == min(K, 100)
    if K > 64:
        assert nw0[WORD_SEAM] > 64 and (K <= 100 or nw0[WORD_SEAM] < K)              # more than one ballot; in the wider rows the list does not fill the row
    return ref


def synthetic_handle(native, K, flags=0):
    c = synthetic()
    g = native.GGSHandle(K, c.num_types, ALPHA_SYN, BETA_SYN, SEED, flags=native.FLAG_LIGHTPCLDAW2 | flags)
    g.set_corpus(c.doc_ptr, c.tokens)
    g.set_z(synthetic_z0(K), redraw_phi=True)
    return g


@pytest.mark.parametrize("K", WIDTHS)
def test_synthetic_corpus_at_every_width(native, oracle, K):
    """K = 1 and 2 (every proposal is the current topic, or the other one), 64 / 65 (one ballot of the list build, and one
    topic more), 130 (a third block), 1024 (wide rows: beta * K is about 10 against word frequencies of about 27)."""
    ref = synthetic_reference(K)
    m = ref[3]
    g = synthetic_handle(native, K, native.FLAG_PARANOID)
    info = g.launch_info()
    assert info["z_kernel"].startswith(KERNEL) and info["num_chunks"] == synthetic().num_docs and info["lds_bytes_z"] == 4 * K
    run_against(g, ref)
    g.close()
    print("K = %d: MH counters %s, word-proposal branches (table, beta) %s" % (K, m.stats.tolist(), m.branches.tolist()))
    if K >= 64:
        assert (m.stats > 0).all() and (m.branches >= 20).all()
    if K == 1:
        assert m.stats.tolist() == [0, 0, SWEEPS * synthetic().num_tokens]


def test_document_proposals_come_from_every_source(oracle):
    """Counted from the restatement at K = 64 on the chain the device is compared with: at least 20 tokens draw their document
    proposal from an earlier position of the same 64-token chunk (the register), from an earlier chunk (memory, behind the
    chunk's store), from the token's own position and from the alpha branch."""
    c = synthetic()
    counts = {}

    def on_token(d, pos, det):
        idx = det["idx"]
        src = "alpha" if idx is None else "own" if idx == pos else "later" if idx > pos else "chunk" if idx >= pos - pos % 64 else "earlier"
        counts[src] = counts.get(src, 0) + 1

    m = R.Model(64, c.num_types, ALPHA_SYN, BETA_SYN, SEED, c.doc_ptr, c.tokens, synthetic_z0(64))
    m.init_phi()
    m.on_token = on_token
    m.sweep(SWEEPS)
    assert_bit_equal(m.z.astype(np.int32), synthetic_reference(64)[2][-1]["z"], "the counted chain")
    print("document proposals by source: %s" % sorted(counts.items()))
    for src in ("chunk", "earlier", "own", "alpha", "later"):
        assert counts.get(src, 0) >= 20, (src, counts)


def test_one_cu_takes_every_workgroup_through_later_documents(native, oracle, monkeypatch):
    """GGS_DEBUG_NUM_CUS=1: the z kernel's grid is at most 32 workgroups for 300 documents, the build's at most 16 for 50 groups
    of 4 words at K = 1024 -- some workgroup of each takes at least 3 items, asserted before anything is compared."""
    K = 1024
    monkeypatch.setenv(PG.KNOB, "1")
    g = synthetic_handle(native, K)
    info = g.launch_info()
    assert info["z_kernel"].startswith(KERNEL) and info["num_chunks"] == 300
    PG.assert_trips(info["num_chunks"], 1, PG.CAP_WAVE, KERNEL)
    assert PG.alias_words_per_block(K) == 4
    PG.assert_trips(PG.alias_items(V_SYN, K), 1, PG.CAP_ALIAS, "count_alias_build_kernel")
    run_against(g, synthetic_reference(K))
    g.close()


# ---- sharded: bit-identical to one handle ---------------------------------------------------------------------------
K_SHARD = 65
FLAGS_SHARDED = dict(phi_burn_in=1, phi_mean_thin=1)


def _results(h):
    return dict(z=h.get_z(), nwk=h.get_type_topic_counts(), nk=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), tables=h.alias_tables(),
                lists=h.word_topic_lists(), mh=h.mh_stats(), kernel=z_kernel(h))


def _rank(native, whole):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K_SHARD, whole.num_types, ALPHA_SYN, BETA_SYN, SEED, flags=native.FLAG_LIGHTPCLDAW2 | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)

    def body(h, rank, sub, tok_base):
        h.set_z(synthetic_z0(K_SHARD)[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(SWEEPS)
        h.check_invariants()
        return dict(_results(h), how=h.count_exchange())
    return make_handle, body


@functools.lru_cache(maxsize=None)
def one_handle():
    from ldagroupedgibbssampler_amd import native
    c = synthetic()
    h = native.GGSHandle(K_SHARD, c.num_types, ALPHA_SYN, BETA_SYN, SEED, flags=native.FLAG_LIGHTPCLDAW2 | native.FLAG_SAVE_PHI_MEAN, **FLAGS_SHARDED)
    h.set_corpus(c.doc_ptr, c.tokens)
    h.set_z(synthetic_z0(K_SHARD), redraw_phi=True)
    h.sweep(SWEEPS)
    r = _results(h)
    h.close()
    return r


@pytest.mark.parametrize("world,mode", [(2, "dense"), (3, "sparse")])
def test_sharded_runs_equal_one_handle(native, oracle, world, mode):
    whole = synthetic()
    out = run_ranks(world, whole, *_rank(native, whole), mode=mode)
    ref = one_handle()
    assert_bit_equal(ref["z"], synthetic_reference(K_SHARD)[2][-1]["z"], "one handle against the restatement")
    z = np.concatenate([out[r]["z"] for r in range(world)])
    assert z.size == whole.num_tokens
    assert_bit_equal(z, ref["z"], "z")
    assert_bit_equal(np.sum([out[r]["mh"] for r in range(world)], axis=0), ref["mh"], "summed MH counters")
    assert int(ref["mh"].sum()) == SWEEPS * whole.num_tokens
    for r in range(world):
        assert out[r]["how"]["sparse"] == (mode == "sparse")
        assert out[r]["kernel"].startswith(KERNEL)
        assert_bit_equal(out[r]["nwk"], ref["nwk"], "n_wk rank %d" % r)
        assert_bit_equal(out[r]["nk"], ref["nk"], "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref["phi"], "phi rank %d" % r)
        assert out[r]["mean"][1] == ref["mean"][1] > 0
        assert_bit_equal(out[r]["mean"][0], ref["mean"][0], "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm")):
            assert_bit_equal(out[r]["tables"][i], ref["tables"][i], "%s rank %d" % (name, r))
        for i, name in enumerate(("nw", "lists")):
            assert_bit_equal(out[r]["lists"][i], ref["lists"][i], "%s rank %d" % (name, r))


def test_one_process_group_equals_one_handle(native, oracle):
    """ggs_group_create / ggs_group_set_z / ggs_group_sweep with the one device there is: the counts are gathered, grouped, at
    the head of every z step."""
    c = synthetic()
    g = native.GGSGroup(K_SHARD, c.num_types, ALPHA_SYN, BETA_SYN, SEED, device_ids=[0], flags=native.FLAG_LIGHTPCLDAW2 | native.FLAG_SAVE_PHI_MEAN,
                        **FLAGS_SHARDED)
    h = g.handles[0]
    h.set_corpus(c.doc_ptr, c.tokens)
    g.set_z([synthetic_z0(K_SHARD)], redraw_phi=True)
    g.sweep(SWEEPS)
    ref = one_handle()
    for name, got in (("z", h.get_z()), ("n_wk", h.get_type_topic_counts()), ("n_k", h.get_topic_totals()), ("phi", h.get_phi()), ("MH counters", h.mh_stats())):
        assert_bit_equal(got, ref[{"n_wk": "nwk", "n_k": "nk", "MH counters": "mh"}.get(name, name)], name)
    g.close()


# ---- ggs_set_z, ggs_sample_z_given_phi, the interface ---------------------------------------------------------------
def test_set_z_to_a_stored_state_against_a_fresh_handle(native, oracle):
    """A handle with a history (two sweeps) is put on a stored state with ggs_set_z and swept; a fresh handle put on the same
    state at the same iteration gives the same z, counts, Phi, tables and lists."""
    K = 64
    c = synthetic()
    stored = synthetic_reference(K)[2][0]["z"]                      # the state after the first sweep
    a = synthetic_handle(native, K)
    a.sweep(2)
    a.set_z(stored, redraw_phi=True)
    b = native.GGSHandle(K, c.num_types, ALPHA_SYN, BETA_SYN, SEED, flags=native.FLAG_LIGHTPCLDAW2)
    b.set_corpus(c.doc_ptr, c.tokens)
    b.set_iteration(2)
    b.set_z(stored, redraw_phi=True)
    for s in range(2):
        ra, rb = _results(a), _results(b)
        for key in ("z", "nwk", "nk", "phi"):
            assert_bit_equal(ra[key], rb[key], "%s after %d sweeps from the stored state" % (key, s))
        for i in range(3):
            assert_bit_equal(ra["tables"][i], rb["tables"][i], "table %d after %d sweeps" % (i, s))
        for i in range(2):
            assert_bit_equal(ra["lists"][i], rb["lists"][i], "list %d after %d sweeps" % (i, s))
        a.sweep(1)
        b.sweep(1)
    assert (a.get_z() != stored).any()
    a.close()
    b.close()


def test_sample_z_given_phi_rebuilds_the_tables_each_iteration(native, oracle, cats):
    """Phi set by hand, then two z steps given it: the tables of the second are those of the first one's counts."""
    K, alpha, beta = 20, 0.1, 0.01
    rng = np.random.default_rng(5)
    phi = rng.dirichlet(np.full(cats.num_types, 0.2), K)
    g = native.GGSHandle(K, cats.num_types, alpha, beta, SEED, flags=native.FLAG_LIGHTPCLDAW2)
    g.set_corpus(cats.doc_ptr, cats.tokens)
    g.init_z_java_lcg(3)
    m = R.Model(K, cats.num_types, alpha, beta, SEED, cats.doc_ptr, cats.tokens, g.get_z())
    g.set_phi(phi)
    m.set_phi(phi)
    g.sample_z_given_phi(2)
    m.sample_z_given_phi(2)
    assert_bit_equal(g.get_z(), m.z.astype(np.int32), "z after two z steps given Phi")
    assert_bit_equal(g.mh_stats(), m.stats, "MH counters")
    assert_bit_equal(g.get_phi(), m.phi, "Phi is left as it was set")
    assert_tables_equal(g, m.tables(), "after two z steps given Phi")
    g.close()


def test_interface(native, cats):
    g = native.GGSHandle(20, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_LIGHTPCLDAW2 | native.FLAG_PCGS)   # GGS_FLAG_PCGS beside it is accepted
    g.set_corpus(cats.doc_ptr, cats.tokens)
    assert (g.mh_stats() == 0).all()
    zk, zf, zc = C.c_int32(), C.c_int32(), C.c_int32()
    assert g._L.ggs_get_z_form(g._h, C.byref(zk), C.byref(zf), C.byref(zc)) == 0
    assert zk.value == 12 and zf.value == 0
    info = g.launch_info()
    assert info["z_kernel"] == "lightpcw2_wave_kernel (wave per document)" and info["lds_bytes_z"] == 4 * 20 and info["num_chunks"] == cats.num_docs
    g.init_z_java_lcg(1)
    g.init_phi()
    g.sweep(2)
    g.sweep_begin()                                                 # the two halves are one sweep
    g.sweep_end()
    g.check_invariants()
    s = g.mh_stats()
    assert s.dtype == np.int64 and s.sum() == 3 * cats.num_tokens and (s > 0).all()
    with pytest.raises(native.GGSError) as e:
        g.get_theta()
    assert e.value.code == native.ERR_UNSUPPORTED
    with pytest.raises(native.GGSError) as e:
        g.collapsed_serial_sweep(1, 1)
    assert e.value.code == native.ERR_STATE
    doc_side, topic_side = g.log_posterior()                        # draws its own theta, allocated now
    assert np.isfinite(doc_side) and np.isfinite(topic_side)
    doc_side, topic_side = g.model_log_likelihood()
    assert np.isfinite(doc_side) and np.isfinite(topic_side) and doc_side + topic_side < 0
    with pytest.raises(native.GGSError) as e:                       # still none to read
        g.get_theta()
    assert e.value.code == native.ERR_UNSUPPORTED
    h = native.GGSHandle(20, cats.num_types, 0.1, 0.01, SEED, flags=native.FLAG_LIGHTPCLDAW2)
    h.set_corpus(cats.doc_ptr, cats.tokens)
    h.init_z_java_lcg(1)
    h.init_phi()
    h.sweep(3)
    g.sweep(1)                                                      # the refusals and the diagnostics left the chain where it was
    h.sweep(1)
    assert_bit_equal(g.get_z(), h.get_z(), "z after 2 + 1 + 1 sweeps")
    g.set_corpus(cats.doc_ptr, cats.tokens)                         # cumulative since set_corpus
    assert (g.mh_stats() == 0).all()
    g.close()
    h.close()


def test_host_mirror_and_driver_end_to_end(native, cats, tmp_path):
    from ldagroupedgibbssampler_amd import sampler
    cfg = sampler.SimpleLDAConfiguration(scheme="lightpcldaw2", topics=20, alpha=0.1, beta=0.01, iterations=3, seed=42, exec_time=None)
    m = sampler.LightPCLDAtypeTopicProposal(cfg)
    m.setRandomSeed(cfg.get_seed())
    m.addInstances(cats)
    m.sample(3)
    assert m.getCurrentIteration() == 3
    phi = np.asarray(m.getPhi())
    assert phi.shape == (20, cats.num_types) and np.allclose(phi.sum(axis=1), 1.0)
    n_wk = np.asarray(m.getTypeTopicMatrix())
    assert n_wk.sum() == cats.num_tokens and m.getMHStats().sum() == 3 * cats.num_tokens
    want = R.build_tables(n_wk, n_wk.sum(axis=0), 0.01)
    assert_bit_equal(m.getAliasTables()[2], want[2], "typeMass of the model's counts")
    nw, lists = m.getWordTopicLists()
    assert_bit_equal(nw, want[3], "nw of the model's counts")
    assert_bit_equal(lists, want[4], "lists of the model's counts")
    m.sampleZGivenPhi(1)
    ds = os.path.join(ROOT, "tests", "golden", "datasets", "cats.txt")
    out = tmp_path / "run"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_dataset.py"), ds, "--scheme", "lightpcldaw2", "--topics", "5",
                        "--iterations", "3", "--seed", "7", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = os.listdir(out)
    assert "type_topic_counts.csv" in files and any(f.startswith("phi") for f in files), files
