"""Every persistent kernel on its second and later work items.

launch() (ggs_host_state.hpp) starts min(items, CUs x per_cu) workgroups and each strides its share; between two items a
workgroup has to bring its private state back to fresh -- LDS counts, the non-zero list with its back-map and nnz, cuml[],
the chunks loaded ahead, polyaurn_sparse's entries and Phi values of the next two tokens, lightpclda's proposal state, the
Poisson kernel's LDS totals, the alias builder's stacks.  On 256 CUs no bit-exact test of the per-document kernels is large
enough for a second item, so:

  * GGS_DEBUG_NUM_CUS=1 (read at ggs_create, behind GGS_DEBUG=1; it can only lower the count) gives the handle one CU's
    grid: with the corpora of tests/persistent_grid.py some workgroup of every z kernel takes at least three documents (or
    groups of 64), of different kinds one after the other -- long, short, one token, empty.  Two sweeps, bit for bit
    against the CPU authority of the scheme: the oracle for ggs, pcgs and collapsed, tests/*_restatement.py for the rest.
    Every case asserts its trip count (persistent_grid.assert_trips) before it compares anything.
  * the real grid, no knob: D = 2 x 32 x CUs + 37 documents of 0..5 tokens for each of the four wave-per-document
    kernels.  The lane-per-document kernels (64 documents per wave, 8 waves per CU) would need more than 131 072 documents
    for a second group on the real grid: they are left to the knob.

The Phi-phase kernels are covered through handles only (ggs_debug_alias has a fixed grid of its own and ggs_debug_poisson
runs debug_poisson_kernel, a thread per draw): alias_build_kernel by the K = 1024 rows (4 words per workgroup and trip,
V = 210: 53 trips over at most 16 workgroups, the last one of 2 words), word_list_build_kernel by the polyaurn_sparse rows,
phi_poisson_kernel by the polyaurn and polyaurn_sparse rows; each of those rows writes the inequality out from V and K.
nzvsspalias' two persistent Phi-phase kernels, vs_bits_kernel and word_list_mask_kernel, go through launch() with the handle's
CU count like its z kernel (ggs_host_phi.hpp: launch_vs_chain and the list build behind the alias tables): the K = 130 row gives
each of the three at least three trips on one CU, the last one ragged (the z kernel's 200 documents come as the padded
two-round order of 384 entries there: its last round is ragged by the entries that hold no document)."""
import os

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import priors
from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import lightpclda_restatement as LR
from tests import nzvs_restatement as NR
from tests import persistent_grid as PG
from tests import polyaurn_restatement as PR
from tests import polyaurn_sparse_restatement as PSR
from tests import spalias_priors_restatement as SPR
from tests import spalias_restatement as SR
from tests.ranks import assert_bit_equal, run_ranks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIORS_FILE = os.path.join(ROOT, "tests", "golden", "priors", "topic_priors_SmallTexts.txt")
SEED, ZSEED, ALPHA, BETA, SWEEPS = 777, 5, 0.1, 0.01, 2
ALIAS_SCHEMES = ("spalias", "spalias_priors", "lightpclda", "polyaurn_sparse", "nzvsspalias")
ORACLE_SCHEMES = ("ggs", "pcgs", "collapsed")


class Row:
    """one kernel at one K: the corpus kind ("wave": 200 documents, "lane": 1706), the knobs that force the kernel, the name
    launch_info() must report, the cap of its plan entry and the Phi-phase kernels whose trips the row asserts as well"""

    def __init__(self, scheme, K, kind, V, kernel, cap, env=None, waves=1, lists=1, phases=(), form=None):
        self.scheme, self.K, self.kind, self.V, self.kernel, self.cap = scheme, K, kind, V, kernel, cap
        self.env, self.waves, self.lists, self.phases, self.form = env or {}, waves, lists, phases, form

    @property
    def id(self):
        return "%s-K%d-%s%s" % (self.scheme, self.K, self.kernel.split(" ")[0], "".join("-%s=%s" % (k[10:], v) for k, v in sorted(self.env.items())))


LANE, WAVE = "lane per document", "wave per document"
SLICED = {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_HOT": "24", "GGS_DEBUG_WARM": "0"}
WARM = {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_WARM": "8", "GGS_DEBUG_WARM_ROWS": "16", "GGS_DEBUG_WARM_FILL": "1", "GGS_DEBUG_HOT": "8", "GGS_DEBUG_WARM_CPW": "0"}
ROWS = [
    Row("pcgs", 20, "lane", 500, LANE, PG.CAP_LANE),
    Row("pcgs", 40, "lane", 500, LANE, PG.CAP_LANE, {"GGS_DEBUG_PCGS_STREAM": "1"}),
    Row("pcgs", 200, "wave", 210, WAVE, PG.CAP_WAVE),
    Row("pcgs", 8, "wave", 210, WAVE, PG.CAP_WAVE, {"GGS_DEBUG_PCGS_WAVE": "1"}),
    Row("collapsed", 20, "lane", 500, LANE, PG.CAP_LANE),
    Row("collapsed", 130, "wave", 210, WAVE, PG.CAP_WAVE, {"GGS_DEBUG_PCGS_WAVE": "1"}),
    Row("polyaurn", 20, "lane", 500, LANE, PG.CAP_LANE, phases=("poisson",)),
    Row("polyaurn", 200, "wave", 210, WAVE, PG.CAP_WAVE, phases=("poisson",)),
    Row("spalias", 8, "wave", 210, "spalias_wave_kernel", PG.CAP_WAVE),
    Row("spalias", 100, "wave", 210, "spalias_wave_kernel", PG.CAP_WAVE),
    Row("spalias", 1024, "wave", 210, "spalias_wave_kernel", PG.CAP_WAVE, phases=("alias",)),
    Row("spalias_priors", 13, "wave", 210, "spalias_wave_kernel", PG.CAP_WAVE),
    Row("lightpclda", 8, "wave", 210, "lightpc_wave_kernel", PG.CAP_WAVE),
    Row("lightpclda", 100, "wave", 210, "lightpc_wave_kernel", PG.CAP_WAVE),
    Row("polyaurn_sparse", 8, "wave", 800, "polyaurn_sparse_wave_kernel", PG.CAP_WAVE, phases=("poisson", "wordlist")),
    Row("polyaurn_sparse", 160, "wave", 210, "polyaurn_sparse_wave_kernel", PG.CAP_WAVE, phases=("poisson", "wordlist")),
    # nzvsspalias: the z kernel on the wave corpus (K = 8: tokens without a candidate draw from the alias table); K = 130 and
    # V = 1030: 33 x 3 = 99 items of vs_bits_kernel on 32 workgroups, 258 groups of four words on 8 workgroups of word_list_mask_kernel
    Row("nzvsspalias", 8, "wave", 210, "nzvs_wave_kernel", PG.CAP_WAVE, phases=("no candidate",)),
    Row("nzvsspalias", 130, "wave", 1030, "nzvs_wave_kernel", PG.CAP_WAVE, phases=("vsbits", "wordmask", "ragged z")),
    # ggs is bit-compared at size elsewhere; these pin the knob.  The score-register kernels run one workgroup of four waves
    # per CU over up to three chunk lists (cold, hot, warm): the count asked of num_chunks is per list
    Row("ggs", 100, "wave", 210, "z_sliced_kernel", PG.CAP_SLICED, dict(SLICED, GGS_DEBUG_SPLIT="0"), waves=PG.SLICED_WAVES, lists=3, form="fused"),
    Row("ggs", 100, "wave", 210, "z_sliced_kernel", PG.CAP_SLICED, dict(SLICED, GGS_DEBUG_SPLIT="2"), waves=PG.SLICED_WAVES, lists=3, form="split"),
    Row("ggs", 100, "wave", 210, "z_warm_kernel", PG.CAP_SLICED, WARM, waves=PG.SLICED_WAVES, lists=3),
    Row("ggs", 40, "wave", 210, "z_kernel (whole-row tiles)", PG.CAP_LANE, {"GGS_DEBUG_ZKERNEL": "0"}),
    Row("ggs", 40, "wave", 210, "z_stream1_kernel", PG.CAP_LANE, {"GGS_DEBUG_ZKERNEL": "2"}),
    Row("ggs", 40, "wave", 210, "z_stream_kernel (two passes)", PG.CAP_LANE, {"GGS_DEBUG_ZKERNEL": "3"}),
    Row("ggs", 257, "wave", 210, "z_stream1_kernel", PG.CAP_LANE),
]
BY_ID = {r.id: r for r in ROWS}
assert len(BY_ID) == len(ROWS)
MARGIN_ROWS = [r.id for r in ROWS if (r.scheme, r.K) in (("spalias", 8), ("polyaurn_sparse", 8))]   # both GGS_DEBUG_MARGIN forms


def flags_of(native, scheme):
    return {"ggs": 0, "pcgs": native.FLAG_PCGS, "collapsed": native.FLAG_COLLAPSED, "polyaurn": native.FLAG_POLYAURN, "spalias": native.FLAG_SPALIAS,
            "spalias_priors": native.FLAG_SPALIAS, "lightpclda": native.FLAG_LIGHTPCLDA, "polyaurn_sparse": native.FLAG_POLYAURN_SPARSE,
            "nzvsspalias": native.FLAG_NZVSSPALIAS}[scheme]


def has_mean(scheme):
    return scheme not in ("collapsed", "nzvsspalias")               # counts only: Phi is a point estimate of them; nzvsspalias keeps no mean


_corpora = {}


def corpus_of(kind, V):
    if (kind, V) not in _corpora:
        c = PG.mixed_corpus(PG.WAVE_KINDS if kind == "wave" else PG.LANE_KINDS, V, seed=len(kind) + V)
        PG.assert_kinds(c)
        _corpora[(kind, V)] = c
    return _corpora[(kind, V)]


def vocabulary(V):
    """the priors file's words on frequent word ids"""
    vocab = ["w%d" % i for i in range(V)]
    vocab[0], vocab[1], vocab[2], vocab[5] = "mother", "disk", "slip", "drive"
    return vocab


def cells_of(row):
    cells = priors.load_zero_cells(PRIORS_FILE, row.K, vocabulary(row.V))
    assert len(cells[0]) == 4 * (row.K - 1)                         # four words, each kept in one topic
    return cells


# ---- the device ---------------------------------------------------------------------------------------------------------
def create(native, monkeypatch, cus, env, K, V, flags, **kw):
    """ggs_create under the knobs: set around the call, gone after it"""
    env = dict(env)
    if cus is not None:
        env[PG.KNOB] = str(cus)
    monkeypatch.delenv(PG.KNOB, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        return native.GGSHandle(K, V, ALPHA, BETA, SEED, flags=flags | native.FLAG_PARANOID, **kw)
    finally:
        for k in env:
            monkeypatch.delenv(k)


def snapshot(g, scheme, mean=True):
    s = dict(z=g.get_z(), n_wk=g.get_type_topic_counts(), n_k=g.get_topic_totals(), phi=g.get_phi(), n_dk=g.get_doc_topic_counts())
    if scheme == "ggs":
        s["theta"] = g.get_theta()
    if scheme in ALIAS_SCHEMES:
        s["ps"], s["a"], s["typeNorm"] = g.alias_tables()
    if scheme == "spalias_priors":
        s["priors"] = g.get_topic_priors()
    if scheme == "lightpclda":
        s["mh_stats"] = np.asarray(g.mh_stats(), np.int64)
    if scheme in ("polyaurn_sparse", "nzvsspalias"):
        s["nw"], s["word lists"] = g.word_topic_lists()
        s["sparse_stats"] = np.asarray(g.sparse_stats(), np.int64)
    if scheme == "nzvsspalias":
        s["vs_stats"] = np.asarray(g.vs_stats(), np.int64)[:2]      # undrawn cells of the last draw, zero cells of Phi
    if mean and has_mean(scheme):
        s["phi mean"], n = g.get_phi_mean()
        s["phi mean samples"] = np.array([n], np.int64)
    return s


def device_run(native, monkeypatch, row, cus, margin=None, trips=True):
    c = corpus_of(row.kind, row.V)
    env = dict(row.env)
    if margin is not None:
        env["GGS_DEBUG_MARGIN"] = margin
    mean = dict(phi_burn_in=1, phi_mean_thin=1) if has_mean(row.scheme) else {}
    g = create(native, monkeypatch, cus, env, row.K, row.V, flags_of(native, row.scheme) | (native.FLAG_SAVE_PHI_MEAN if mean else 0), **mean)
    if row.scheme == "spalias_priors":
        g.set_topic_priors(*cells_of(row))
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(ZSEED)
    g.init_phi()
    info = g.launch_info()
    assert row.kernel in info["z_kernel"], info
    if row.form:
        assert info["z_form"] == row.form, info
    if cus is not None and trips:                                   # the trips of this case, before anything is compared
        assert c.num_docs >= 3 * cus * row.cap * (1 if row.kind == "wave" else 64)
        PG.assert_trips(info["num_chunks"], cus, row.cap * row.lists, row.id, waves=row.waves)
        if "alias" in row.phases:
            PG.assert_trips(PG.alias_items(row.V, row.K), cus, PG.CAP_ALIAS, "alias_build_kernel")
            assert PG.alias_words_per_block(row.K) == 4 and row.V % 4 != 0                       # a ragged last trip
        if "wordlist" in row.phases:
            PG.assert_trips(row.V, cus, PG.CAP_WORDLIST, "word_list_build_kernel", waves=PG.WORDLIST_WAVES)
        if "poisson" in row.phases:
            PG.assert_trips(PG.poisson_tiles(row.V, row.K, cus), cus, PG.CAP_POISSON, "phi_poisson_kernel")
        if "vsbits" in row.phases:                                  # ceil(V / 32) words of 32 cells x ceil(K / 64) waves of topics
            PG.assert_trips(PG.vs_bits_items(row.V, row.K), cus, PG.CAP_VSBITS, "vs_bits_kernel")
            assert PG.vs_bits_items(row.V, row.K) == -(-row.V // 32) * -(-row.K // 64) and PG.vs_bits_items(row.V, row.K) % (cus * PG.CAP_VSBITS) != 0
        if "wordmask" in row.phases:                                # a word per wave, four waves a workgroup
            PG.assert_trips(row.V, cus, PG.CAP_WORDMASK, "word_list_mask_kernel", waves=PG.WORDLIST_WAVES)
            assert -(-row.V // PG.WORDLIST_WAVES) % (cus * PG.CAP_WORDMASK) != 0 and row.V % PG.WORDLIST_WAVES != 0
        if "ragged z" in row.phases:                                # the last round is not full: by its count, or by the padded order's -1 entries
            assert info["num_chunks"] % (cus * row.cap) != 0 or info["num_chunks"] > c.num_docs, info
    g.sweep(SWEEPS)
    s = snapshot(g, row.scheme)
    if "no candidate" in row.phases:                                # the first sweep draws every token from the alias tables (no list yet); the second some
        assert c.num_tokens < s["sparse_stats"][2] < 2 * c.num_tokens and s["sparse_stats"][:2].sum() > 0, s["sparse_stats"]
    g.check_invariants()
    g.close()
    return s


# ---- the CPU authority, once per row ------------------------------------------------------------------------------------
_authority = {}


def authority(oracle, row):
    if row.id in _authority:
        return _authority[row.id]
    c, K, V = corpus_of(row.kind, row.V), row.K, row.V
    z0 = java_lcg_initial_z(c.num_tokens, K, ZSEED)
    mean = dict(save_phi_mean=True, phi_burn_in=1, phi_thin=1)
    if row.scheme in ORACLE_SCHEMES:
        o = oracle.OracleSampler(K, V, ALPHA, BETA, SEED, threads=4)
        if row.scheme == "pcgs":
            o.set_scheme("pcgs")
        o.set_phi_mean_gating(has_mean(row.scheme), 1, 1)
        o.set_corpus(c.doc_ptr, c.tokens)
        o.init_z_java_lcg(ZSEED)
        o.init_phi()
        if row.scheme == "collapsed":
            o.collapsed_parallel_sweep(SWEEPS)
        else:
            o.sweep(SWEEPS)
        s = dict(z=o.get_z(), n_wk=o.get_type_topic_counts(), n_k=o.get_topic_totals(), n_dk=o.get_doc_topic_counts())
        if row.scheme == "collapsed":                               # the point estimate (beta + n_wk) / (betaSum + n_k)
            s["phi"] = ((BETA + s["n_wk"].astype(np.float64)) / (BETA * V + s["n_k"].astype(np.float64))).T
        else:
            s["phi"] = o.get_phi()
            s["phi mean"], n = o.get_phi_mean()
            s["phi mean samples"] = np.array([n], np.int64)
        if row.scheme == "ggs":
            s["theta"] = o.get_theta()
    else:
        if row.scheme == "spalias":
            m = SR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0, **mean)
        elif row.scheme == "spalias_priors":
            m = SPR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0, cells=cells_of(row), **mean)
        elif row.scheme == "lightpclda":
            m = LR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0, **mean)
        elif row.scheme == "polyaurn":
            m = PR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0, **mean)
        elif row.scheme == "nzvsspalias":
            m = NR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0)
        else:
            m = PSR.Model(K, V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0, **mean)
        m.init_phi()
        m.sweep(SWEEPS)
        n_wk = np.asarray(m.counts())
        if n_wk.shape != (V, K):                                    # the Polya-urn restatements keep [K][V]
            n_wk = n_wk.T
        n_wk = np.ascontiguousarray(n_wk).astype(np.int32)
        s = dict(z=m.z.astype(np.int32), n_wk=n_wk, n_k=n_wk.sum(axis=0).astype(np.int32), phi=m.phi, n_dk=PG.doc_topic_counts(c.doc_ptr, m.z, K))
        if row.scheme in ALIAS_SCHEMES:
            s["ps"], s["a"], s["typeNorm"] = m.tables
        if row.scheme == "spalias_priors":
            s["priors"] = m.P
        if row.scheme == "lightpclda":
            s["mh_stats"] = np.asarray(m.stats, np.int64)
            assert_bit_equal(np.asarray(m.topic_totals(), np.int32), s["n_k"], "the restatement's own n_k")
        if row.scheme in ("polyaurn_sparse", "nzvsspalias"):
            s["nw"], s["word lists"], s["sparse_stats"] = m.nw, PSR.padded(m.lists, K), np.asarray(m.stats, np.int64)
        if row.scheme == "nzvsspalias":
            s["vs_stats"] = np.asarray(m.vs_stats_first_two(), np.int64)
        if has_mean(row.scheme):
            pm = m.phi_mean()
            s["phi mean"], n = pm if isinstance(pm, tuple) else (pm, m.n_sampled)
            s["phi mean samples"] = np.array([n], np.int64)
    assert int(s["phi mean samples"][0]) == 1 if has_mean(row.scheme) else True
    _authority[row.id] = s
    return s


def assert_same(got, want, tag):
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    for name in ("z", "n_wk", "n_k", "n_dk") + tuple(k for k in sorted(got) if k not in ("z", "n_wk", "n_k", "n_dk")):
        a, b = np.asarray(got[name]), np.asarray(want[name])
        if a.dtype.kind != "f":
            a, b = a.astype(np.int64), b.astype(np.int64)
        assert_bit_equal(a, b, "%s: %s" % (tag, name))


# ---- one CU -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", list(BY_ID))
def test_one_cu_equals_the_cpu_authority(native, oracle, monkeypatch, rid):
    row = BY_ID[rid]
    assert_same(device_run(native, monkeypatch, row, 1), authority(oracle, row), rid + " on one CU")


@pytest.mark.parametrize("rid", MARGIN_ROWS)
def test_one_cu_with_every_token_replayed(native, oracle, monkeypatch, rid):
    """GGS_DEBUG_MARGIN=1e30: the exact chain of every token, whose cuml[] and running sums are the replay's own"""
    row = BY_ID[rid]
    assert_same(device_run(native, monkeypatch, row, 1, margin="1e30"), authority(oracle, row), rid + " on one CU, margin 1e30")


@pytest.mark.parametrize("rid", MARGIN_ROWS[:1])
def test_one_two_and_all_cus_agree(native, oracle, monkeypatch, rid):
    """the schedule-free claim itself: three grids, one result -- and the clamp (a count above the real one is the real one)"""
    row = BY_ID[rid]
    one, two, real = (device_run(native, monkeypatch, row, cus) for cus in (1, 2, None))
    assert_same(one, authority(oracle, row), rid + " on one CU")
    assert_same(two, one, rid + ": two CUs against one")
    assert_same(real, one, rid + ": the real grid against one CU")
    assert_same(device_run(native, monkeypatch, row, 1 << 20, trips=False), real, rid + ": a count above the device's")


def test_the_knob_reaches_the_corpus_lists(native, oracle, monkeypatch):
    """Where the knob shows outside a grid: with between one and two rounds of 64-document groups for the resident lane waves
    (CUs x at most 8) the document order becomes the padded two-round list (ggs_corpus_lists.hpp, pcgs_order), -1 where
    there is no document.  600 documents are ten groups: padded on one CU, plain on the device's own count -- and the wave
    kernel, which skips the padding, gives the same bits from either list."""
    row, D = BY_ID[MARGIN_ROWS[0]], 600
    c = PG.short_corpus(D, row.V, seed=3)
    runs = []
    for cus in (1, None):
        g = create(native, monkeypatch, cus, row.env, row.K, row.V, flags_of(native, row.scheme))
        g.set_corpus(c.doc_ptr, c.tokens)
        g.init_z_java_lcg(ZSEED)
        g.init_phi()
        items = g.launch_info()["num_chunks"]
        g.sweep(SWEEPS)
        runs.append((items, snapshot(g, row.scheme, mean=False)))
        g.check_invariants()
        g.close()
    assert runs[1][0] == D                                          # the plain order
    assert runs[0][0] > D and runs[0][0] % 128 == 0, runs[0][0]      # two rounds of W groups of 64
    PG.assert_trips(runs[0][0], 1, PG.CAP_WAVE, "the padded list")
    assert_same(runs[0][1], runs[1][1], "the padded list on one CU against the plain one")


# ---- an exchange: two ranks of one CU each against one handle -----------------------------------------------------------
def _rank(native, whole, K, flags, kw):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        assert os.environ.get(PG.KNOB) == "1"                       # set by the test body around both ranks' ggs_create
        h = native.GGSHandle(K, whole.num_types, ALPHA, BETA, SEED, flags=flags, **kw)
        return h

    def body(h, rank, sub, tok_base):
        z0 = java_lcg_initial_z(whole.num_tokens, K, 17)
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        info = h.launch_info()
        h.sweep(SWEEPS)
        h.check_invariants()
        return dict(z=h.get_z(), n_wk=h.get_type_topic_counts(), n_k=h.get_topic_totals(), phi=h.get_phi(), mean=h.get_phi_mean(), info=info,
                    docs=sub.num_docs, tables=h.alias_tables() if flags & native.FLAG_SPALIAS else None)
    return make_handle, body


@pytest.mark.parametrize("scheme,K,kernel", [("spalias", 40, "spalias_wave_kernel"), ("polyaurn", 200, "pcgs_wave_kernel")])
def test_two_ranks_of_one_cu_equal_one_handle(native, oracle, monkeypatch, scheme, K, kernel):
    """Over the thread transport of tests/ranks.py: each rank's z kernel walks its 100 documents on one CU's grid, its Poisson draw (polyaurn) the
    100 topics of its slice in 8 tiles on two workgroups; the reference is one handle on the real grid."""
    world, V = 2, 900
    whole = corpus_of("wave", V)
    flags = flags_of(native, scheme) | native.FLAG_SAVE_PHI_MEAN
    kw = dict(phi_burn_in=1, phi_mean_thin=1)
    monkeypatch.setenv(PG.KNOB, "1")
    out = run_ranks(world, whole, *_rank(native, whole, K, flags, kw), mode="dense")
    monkeypatch.delenv(PG.KNOB)
    for r in range(world):
        assert kernel in out[r]["info"]["z_kernel"], out[r]["info"]
        assert out[r]["docs"] >= 3 * PG.CAP_WAVE
        PG.assert_trips(out[r]["info"]["num_chunks"], 1, PG.CAP_WAVE, "%s rank %d" % (scheme, r))
    if scheme == "polyaurn":
        PG.assert_trips(PG.poisson_tiles(V, K // world, 1), 1, PG.CAP_POISSON, "phi_poisson_kernel of a rank's slice")
    ref = native.GGSHandle(K, V, ALPHA, BETA, SEED, flags=flags, **kw)
    ref.set_corpus(whole.doc_ptr, whole.tokens)
    ref.set_z(java_lcg_initial_z(whole.num_tokens, K, 17), redraw_phi=True)
    ref.sweep(SWEEPS)
    assert_bit_equal(np.concatenate([out[r]["z"] for r in range(world)]), ref.get_z(), "z")
    mean, n = ref.get_phi_mean()
    tables = ref.alias_tables() if scheme == "spalias" else None
    for r in range(world):
        assert_bit_equal(out[r]["n_wk"], ref.get_type_topic_counts(), "n_wk rank %d" % r)
        assert_bit_equal(out[r]["n_k"], ref.get_topic_totals(), "n_k rank %d" % r)
        assert_bit_equal(out[r]["phi"], ref.get_phi(), "phi rank %d" % r)
        assert out[r]["mean"][1] == n == 1
        assert_bit_equal(out[r]["mean"][0], mean, "phi mean rank %d" % r)
        for i, name in enumerate(("ps", "a", "typeNorm") if tables else ()):
            assert_bit_equal(out[r]["tables"][i], tables[i], "%s rank %d" % (name, r))
    ref.close()


# ---- the real grid ------------------------------------------------------------------------------------------------------
REAL = [Row("pcgs", 8, "real", 60, WAVE, PG.CAP_WAVE, {"GGS_DEBUG_PCGS_WAVE": "1"}), Row("spalias", 8, "real", 60, "spalias_wave_kernel", PG.CAP_WAVE),
        Row("polyaurn_sparse", 8, "real", 60, "polyaurn_sparse_wave_kernel", PG.CAP_WAVE), Row("lightpclda", 8, "real", 60, "lightpc_wave_kernel", PG.CAP_WAVE)]


@pytest.mark.parametrize("row", REAL, ids=[r.id for r in REAL])
def test_the_real_grid_takes_a_third_document(native, oracle, monkeypatch, row):
    """No knob: 2 x 32 x CUs + 37 documents of 0..5 tokens, one sweep.  A workgroup's third document exists whatever the
    plan's workgroups per CU (at most 32)."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    D = 2 * 32 * cus + 37
    c = PG.short_corpus(D, row.V, seed=cus)
    lens = np.diff(c.doc_ptr)
    assert lens.max() == 5 and (lens == 0).sum() > D // 12 and (lens == 1).sum() > D // 12
    g = create(native, monkeypatch, None, row.env, row.K, row.V, flags_of(native, row.scheme))
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(ZSEED)
    g.init_phi()
    info = g.launch_info()
    assert row.kernel in info["z_kernel"], info
    assert info["num_chunks"] >= 2 * 32 * cus and D > 2 * 32 * cus
    assert PG.min_trips(info["num_chunks"], cus, PG.CAP_WAVE) == 3
    z0 = java_lcg_initial_z(c.num_tokens, row.K, ZSEED)
    if row.scheme == "pcgs":
        o = oracle.OracleSampler(row.K, row.V, ALPHA, BETA, SEED, threads=4)
        o.set_scheme("pcgs")
        o.set_corpus(c.doc_ptr, c.tokens)
        o.init_z_java_lcg(ZSEED)
        o.init_phi()
        o.sweep(1)
        want = dict(z=o.get_z(), n_wk=o.get_type_topic_counts(), n_k=o.get_topic_totals(), phi=o.get_phi(), n_dk=o.get_doc_topic_counts())
    else:
        M = {"spalias": SR, "polyaurn_sparse": PSR, "lightpclda": LR}[row.scheme]
        m = M.Model(row.K, row.V, ALPHA, BETA, SEED, c.doc_ptr, c.tokens, z0)
        m.init_phi()
        m.sweep(1)
        n_wk = np.asarray(m.counts())
        n_wk = np.ascontiguousarray(n_wk if n_wk.shape == (row.V, row.K) else n_wk.T).astype(np.int32)
        want = dict(z=m.z.astype(np.int32), n_wk=n_wk, n_k=n_wk.sum(axis=0).astype(np.int32), phi=m.phi, n_dk=PG.doc_topic_counts(c.doc_ptr, m.z, row.K))
        want["ps"], want["a"], want["typeNorm"] = m.tables
        if row.scheme == "lightpclda":
            want["mh_stats"] = np.asarray(m.stats, np.int64)
        if row.scheme == "polyaurn_sparse":
            want["nw"], want["word lists"], want["sparse_stats"] = m.nw, PSR.padded(m.lists, row.K), np.asarray(m.stats, np.int64)
    g.sweep(1)
    got = snapshot(g, row.scheme, mean=False)
    g.check_invariants()
    g.close()
    assert_same(got, want, row.id + " on the real grid")
