"""A handle with a history: what tests/test_handle_lifecycle_gpu.py needs to resume a chain on a fresh handle, rewind a
handle to an earlier state of itself, reuse it for a second and a third corpus and continue across shards -- for all
eleven schemes from ONE table (ROWS, in the order of kSchemes in csrc/ggs_host_state.hpp plus spalias_priors), the way
tests/scheme_table_cases.py keeps the capabilities in one place.  Everything here runs without a device; the pure parts
are pinned by tests/test_handle_lifecycle_model.py.

The streams are counter-based, keyed by (seed, iteration, purpose, element), so every comparison is bit equality: with the
uninterrupted chain, with a fresh handle, and with the oracle (oracle/ for ggs, pcgs and collapsed's parallel schedule,
the tests/*_restatement.py models for the rest) run over the same script of calls.

The exported state (what a second handle needs to continue a chain), per scheme -- read from ggs_set_z, ggs_set_phi,
ggs_set_iteration and ggs_init_phi in csrc/ggs_api.hip, and stated in include/ggs_hip.h at ggs_set_iteration:

  ggs              z, Phi, iteration.  theta is not state: it is drawn from z at the head of the z step (or ahead, beside
                   the previous sweep's Phi draw, and then dropped by ggs_set_z / kept or not by the iteration number).  The
                   float32 rows the cold chunks of the K <= 160 z step score from are rewritten by ggs_set_phi.
  pcgs             z, Phi, iteration.  (Its z step scores from the fp64 rows: only scheme ggs reads the float32 ones.)
  polyaurn         z, Phi (with its exact zeros), iteration.
  spalias          z, Phi, iteration; the alias tables are rebuilt from the Phi that was set.
  spalias_priors   the same, and the priors, which are configuration: set on the new handle BEFORE it gets a Phi.  The
                   conditional draw of the next sweep takes sum_phi from the rows of the Phi that was set.
  lightpclda       z, Phi, iteration; tables as spalias.  The Metropolis-Hastings counters are not state.
  polyaurn_sparse  z, Phi, iteration; tables and the words' lists (phi != 0.0) are rebuilt from the Phi that was set.
  nzvsspalias      z, Phi, iteration, and pi (configuration).  After ggs_set_phi the words' lists are the cells with
                   phi != 0.0, after a sweep the DRAWN cells: the two agree, and the resumed chain is the same chain, exactly
                   when no drawn cell holds 0.0 (a gamma draw that underflowed).  The variable-selection chain itself reads
                   only which cells of the old row are 0.0, so Phi carries it.
  collapsed, lightcollapsed, adlda
                   z and iteration: there is no Phi.  ggs_set_z rebuilds the counts, ggs_init_phi is the magnitude launch
                   (tokensPerTopic; with an exchange the merge of the shards' counts), lightcollapsed's tables and lists are
                   built at the head of the next sweep.  ggs_set_phi is refused by lightcollapsed and adlda
                   (GGS_ERR_UNSUPPORTED) and is not part of collapsed's state (ggs_get_phi is the point estimate of the counts).

Not state, under every scheme: the phi mean and n_sampled (a resumed handle starts its own: ggs_set_phi restarts the sum,
n_sampled counts what the handle itself accepted), the cumulative counters (mh, sparse: since ggs_set_corpus), the timings.

No row is left out of resume, rewind or reuse.  Where a row lacks an entry point the case is not generated:
ggs_sample_z_given_phi does not exist for the three count-form rows (GGS_ERR_UNSUPPORTED: "no Phi to condition on"), and
ggs_collapsed_serial_sweep exists for collapsed alone (GGS_ERR_STATE elsewhere)."""
import functools
import itertools
from dataclasses import dataclass

import numpy as np

from ldagroupedgibbssampler_amd.corpus import Corpus
from oracle import oracle as O
from tests.ranks import assert_bit_equal, run_ranks, shard_of  # noqa: F401 -- shard_of: for the tests that cut a corpus the same way

SEED, ZSEED, ALPHA = 90210, 31, 0.1
BURN_IN, THIN = 1, 2                                    # the phi mean accepts iterations 2, 4, 6, ...
V = 120                                                 # the alphabet of every corpus here: a handle keeps its V for life
KS = (8, 200)                                           # lane-per-document and score-register kernels / wave-per-document and streaming
CANON = (("sweep", 4),)                                 # the uninterrupted chain every section compares with


@dataclass(frozen=True)
class Row:
    name: str
    scheme: str                    # key of native.SCHEME_FLAGS
    beta: float
    form: str                      # "theta" (ggs), "phi" (the pcgs family), "count" (no Phi)
    oracle: str                    # "c" (oracle/ggs_oracle.c) or the tests.*_restatement module of its model
    exports: tuple                 # what a second handle is given, in the order the docstring lists it
    tables: bool = False           # ggs_get_alias_tables
    lists: bool = False            # ggs_get_word_topic_lists
    mh: bool = False               # ggs_get_mh_stats
    sparse: bool = False           # ggs_get_sparse_stats
    vs: bool = False               # ggs_get_vs_stats
    theta: bool = False            # the chain keeps a theta (ggs_get_theta is part of the state compared)
    log_posterior: bool = False    # ggs_log_posterior is supported
    mean: str = "sum"              # the phi mean: "sum" of the accepted Phi, "zero" (nzvsspalias: n_sampled advances, the sum stays 0), "none"
    priors: bool = False

    @property
    def z_given_phi(self):
        return self.form != "count"

    @property
    def zeros_in_phi(self):
        return self.scheme in ("polyaurn", "polyaurn_sparse")


PHI = ("z", "phi", "iteration")
ROWS = (
    Row("ggs", "ggs", 0.05, "theta", "c", PHI, theta=True, log_posterior=True),
    Row("pcgs", "pcgs", 0.05, "phi", "c", PHI, log_posterior=True),
    Row("collapsed", "collapsed", 0.05, "count", "c", ("z", "iteration"), mean="none"),
    Row("polyaurn", "polyaurn", 0.01, "phi", "polyaurn_restatement", PHI, log_posterior=True),
    Row("spalias", "spalias", 0.05, "phi", "spalias_restatement", PHI, tables=True, log_posterior=True),
    Row("spalias_priors", "spalias", 0.05, "phi", "spalias_priors_restatement", PHI, tables=True, log_posterior=True, priors=True),
    Row("lightpclda", "lightpclda", 0.05, "phi", "lightpclda_restatement", PHI, tables=True, mh=True, log_posterior=True),
    Row("polyaurn_sparse", "polyaurn_sparse", 0.01, "phi", "polyaurn_sparse_restatement", PHI, tables=True, lists=True, sparse=True, log_posterior=True),
    Row("lightcollapsed", "lightcollapsed", 0.05, "count", "lightcollapsed_restatement", ("z", "iteration"), tables=True, lists=True, mh=True, mean="none"),
    Row("nzvsspalias", "nzvsspalias", 0.5, "phi", "nzvs_restatement", PHI, tables=True, lists=True, sparse=True, vs=True, log_posterior=True, mean="zero"),
    Row("adlda", "adlda", 0.05, "count", "adlda_restatement", ("z", "iteration"), lists=True, sparse=True, mean="none"),
)
ROW = {r.name: r for r in ROWS}
VS_PI = 0.4                                             # not the default: a handle that lost it on the way would show


def prior_cells(K):
    """spalias_priors' few zeroed cells: three topics for each of two frequent words -- no topic loses all its words, no word
    all its topics (ensureConsistentPriors)."""
    topics = [k for k in (0, 2, K - 1) for _ in range(2)]
    words = [1, 7] * 3
    return np.asarray(topics, np.int32), np.asarray(words, np.int32)


# ---- corpora ------------------------------------------------------------------------------------------------------------
def _corpus(lens, seed, words=V, zipf=True):
    rng = np.random.default_rng(seed)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p = 1.0 / np.arange(1, words + 1) if zipf else np.ones(words)
    return Corpus(doc_ptr, rng.choice(words, int(doc_ptr[-1]), p=p / p.sum()).astype(np.int32), V)


def shape_of(c):
    lens = np.diff(c.doc_ptr)
    return dict(D=c.num_docs, N=c.num_tokens, longest=int(lens.max()), distinct=int(np.unique(c.tokens).size), empty=int((lens == 0).sum()))


@functools.lru_cache(maxsize=None)
def corpus(name):
    """The corpora by name, each with the properties the tests rely on asserted here (tests/test_handle_lifecycle_model.py
    builds them all on the CPU).  Between A and every other corpus D, N, the longest document and the number of distinct words
    all differ, so a handle that goes A -> other -> A sees each of them change in both directions."""
    if name == "A":          # more documents than word types (for ggs at K <= 160: the theta draw keeps the handle's stream), three groups of 64
        c = _corpus(np.random.default_rng(1).permutation(np.arange(160) % 41), 11)
        s = shape_of(c)
        assert s["D"] == 160 > V and s["empty"] >= 3 and s["longest"] == 40 and s["distinct"] > 100
    elif name == "B":        # fewer documents than types, fewer tokens and words, one document longer than K = 200 and than A's longest
        lens = np.random.default_rng(2).permutation(np.arange(90) % 31)
        lens[17] = 300
        c = _corpus(lens, 12, words=70)
        s = shape_of(c)
        assert s["D"] == 90 < V and s["empty"] >= 2 and s["longest"] == 300 and s["distinct"] <= 70
    elif name == "LONG":     # a document the lane-per-document kernels' int16 counts cannot hold
        c = _corpus(np.array([5, 33000, 0, 12]), 13, words=70)
        s = shape_of(c)
        assert s["longest"] == 33000 > 32767 and s["empty"] == 1 and s["D"] == 4
    elif name == "PARTS":    # ggs at K = 200: D >= 2 V and D >= 8 * 64, so the streaming z step is cut into eight parts
        c = _corpus(np.random.default_rng(4).permutation(np.arange(520) % 9), 14)
        s = shape_of(c)
        assert s["D"] == 520 >= 2 * V and s["D"] >= 8 * 64 and s["empty"] > 0
    elif name == "HOT":      # ggs at K <= 160 with the table caps of HOT_ENV: 8 hot words, warm tiers behind them, cold words behind those
        c = _corpus(np.random.default_rng(5).permutation(np.arange(150) % 61), 15)
        s = shape_of(c)
        assert s["distinct"] > 8 + 3 * 16 + 32 and s["empty"] > 0
    elif name == "FEW":      # every word fits the hot table of HOT_ENV: no cold chunk, nothing to split, no warm tier
        c = _corpus(np.random.default_rng(6).permutation(np.arange(100) % 37), 16, words=8, zipf=False)
        s = shape_of(c)
        assert s["distinct"] == 8 and s["empty"] > 0
    else:
        raise KeyError(name)
    ref = shape_of(corpus("A")) if name != "A" else None
    if ref is not None and name in ("B", "LONG"):
        assert all(s[k] != ref[k] for k in ("D", "N", "longest", "distinct")), (s, ref)
    c.doc_ptr.setflags(write=False)
    c.tokens.setflags(write=False)
    return c


# small tables, as test_alternate_z_kernels_agree's "warmsparse" mode has them, and three tiers at most so that cold words remain:
# read when the handle is created
HOT_ENV = {"GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_HOT": "8", "GGS_DEBUG_WARM": "3", "GGS_DEBUG_WARM_ROWS": "16", "GGS_DEBUG_WARM_FILL": "1", "GGS_DEBUG_WARM_CPW": "0"}


def initial_z(c, K, seed=ZSEED):
    """java.util.Random(seed).nextInt(K) per token, from the oracle (ggs_init_z_java_lcg's stream without the library)"""
    return O.jrandom_ints(seed, K, c.num_tokens)


def counts_of(c, z, K):
    n = np.zeros((V, K), np.int32)
    np.add.at(n, (np.asarray(c.tokens, np.int64), np.asarray(z, np.int64)), 1)
    return n


def point_estimate(n_wk, beta):
    """ggs_get_phi of a count-form scheme: (beta + n_wk) / (betaSum + n_k), [K][V]"""
    n = n_wk.astype(np.float64)
    return np.ascontiguousarray(((beta + n) / (beta * float(n_wk.shape[0]) + n.sum(axis=0))).T)


# ---- the phi mean's rule ------------------------------------------------------------------------------------------------
def accepted(iteration, burn_in=BURN_IN, thin=THIN):
    """UPLDA:1350-1352, sample_phi_this_iteration in csrc/ggs_host_sweep.hpp"""
    return burn_in > 0 and iteration > burn_in and iteration % thin == 0


def expected_phi_mean(row, phis, n_before=0, burn_in=BURN_IN, thin=THIN):
    """(mean or None, n_sampled) of a handle that had accepted n_before Phi when its running sum last restarted (a fresh
    handle, ggs_set_corpus, ggs_set_phi: UPLDA:1897-1902 restarts the sum and keeps the count) and has since drawn
    phis = {iteration: Phi} by whole sweeps: the accepted ones added in iteration order from 0.0, divided by the count."""
    if row.mean == "none":
        return None, 0
    total, n = None, n_before
    for it in sorted(phis):
        if accepted(it, burn_in, thin):
            total = (np.zeros_like(phis[it]) if total is None else total) + phis[it]
            n += 1
    if n == 0:
        return None, 0
    if total is None:
        total = np.zeros_like(next(iter(phis.values())))
    if row.mean == "zero":
        total = np.zeros_like(total)
    return total / float(n), n


# ---- the oracle over a script of calls ----------------------------------------------------------------------------------
class Chain:
    """The oracle of a row over corpus c from z0, started at an iteration number: steps ("sweep", n), ("zgiven", n),
    ("iteration", t), ("serial", java_seed, n), ("initz", java_seed: a new seeded z, ggs_init_z_java_lcg; the C oracle only).  state(): z, n_wk, n_k and whatever else the oracle restates.
    seed, doc_base and tok_base are the handle's (ggs_config.seed, ggs_set_corpus): the key and the first elements of the streams."""

    def __init__(self, row, K, c, z0, iteration=0, seed=SEED, doc_base=0, tok_base=0):
        self.row, self.K, self.c = row, K, c
        if row.oracle == "c":
            o = self.o = O.OracleSampler(K, V, ALPHA, row.beta, seed, threads=4)
            if row.scheme == "pcgs":
                o.set_scheme("pcgs")
            o.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
            o.set_iteration(iteration)
            o.set_z(z0, redraw_phi=False)
            if row.form != "count":
                o.init_phi()
            return
        import importlib
        R = importlib.import_module("tests." + row.oracle)
        kw = {}
        if row.priors:
            kw["cells"] = prior_cells(K)
        if row.vs:
            kw["pi"] = VS_PI
        m = self.m = R.Model(K, V, ALPHA, row.beta, seed, c.doc_ptr, c.tokens, z0, tok_base=tok_base, **kw)   # no theta in these: no doc_base
        m.iteration = iteration
        if hasattr(m, "o"):
            m.o.set_iteration(iteration)
        if row.form != "count":
            m.init_phi()

    def run(self, script):
        for step in script:
            getattr(self, "_" + step[0])(*step[1:])
        return self

    def _sweep(self, n):
        if self.row.oracle != "c":
            self.m.sweep(n)
        elif self.row.form == "count":
            self.o.collapsed_parallel_sweep(n)
        else:
            self.o.sweep(n)

    def _zgiven(self, n):
        if self.row.oracle != "c" and hasattr(self.m, "sample_z_given_phi"):
            return self.m.sample_z_given_phi(n)
        if self.row.oracle != "c":                          # the polyaurn model has whole sweeps only: its z step, Phi kept
            from tests import polyaurn_restatement as PR
            m = self.m
            for _ in range(n):
                m.iteration += 1
                PR.z_step(m.doc_ptr, m.tokens, m.z, m.phi, m.alpha, m.seed, m.iteration, m.tok_base)
            return None
        for _ in range(n):
            self.o.set_iteration(self.o.iteration + 1)
            self.o.z_step()
            self.o.update_counts()

    def _iteration(self, t):
        if self.row.oracle == "c":
            return self.o.set_iteration(t)
        self.m.iteration = t
        if hasattr(self.m, "o"):
            self.m.o.set_iteration(t)

    def _initz(self, java_seed):
        assert self.row.oracle == "c"
        self.o.init_z_java_lcg(java_seed)

    def _serial(self, java_seed, n):
        assert self.row.name == "collapsed"
        self.o.collapsed_sweep(java_seed, n)

    @property
    def iteration(self):
        return self.o.iteration if self.row.oracle == "c" else self.m.iteration

    def state(self):
        row = self.row
        if row.oracle == "c":
            z = self.o.get_z()
            phi = self.o.get_phi() if row.form != "count" else None
        else:
            z = np.asarray(self.m.z, np.int32)
            phi = None if row.form == "count" else np.asarray(self.m.phi, np.float64)
        n_wk = counts_of(self.c, z, self.K)
        s = {"z": z, "n_wk": n_wk, "n_k": n_wk.sum(axis=0).astype(np.int32), "phi": phi if phi is not None else point_estimate(n_wk, row.beta),
             "iteration": self.iteration}
        if row.theta:
            s["theta"] = self.o.get_theta()
        if row.vs:
            s["vs_first_two"] = np.asarray(self.m.vs_stats_first_two(), np.int64)
        return s


@functools.lru_cache(maxsize=None)
def oracle_state(name, K, corpus_name, script=CANON, iteration=0):
    """The oracle's state after `script` on a named corpus, computed once per session and shared (read-only)."""
    c = corpus(corpus_name)
    s = Chain(ROW[name], K, c, initial_z(c, K), iteration).run(script).state()
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


# ---- handles ------------------------------------------------------------------------------------------------------------
def create(native, row, K, seed=SEED):
    """A handle of the row's scheme with its configuration (the priors, pi) and the phi mean's gating; no corpus yet."""
    h = native.GGSHandle(K, V, ALPHA, row.beta, seed, flags=native.SCHEME_FLAGS[row.scheme] | native.FLAG_SAVE_PHI_MEAN, phi_burn_in=BURN_IN,
                         phi_mean_thin=THIN)
    try:
        if row.priors:
            h.set_topic_priors(*prior_cells(K))
        if row.vs:
            h.set_variable_selection_prior(VS_PI)
    except BaseException:
        h.close()
        raise
    return h


def start(h, c, z0, doc_base=0, tok_base=0):
    """corpus, initial z, initial Phi (the count form: the magnitude launch)"""
    h.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
    h.set_z(z0, redraw_phi=False)
    h.init_phi()


def export_state(h, row):
    s = {"z": h.get_z(), "iteration": h.iteration}
    if "phi" in row.exports:
        s["phi"] = h.get_phi()
    return s


def restore(h, row, state, order=None, z_slice=slice(None)):
    """The setters in `order` (a permutation of row.exports; default: as listed).  The count form has no Phi to set: its
    ggs_init_phi (tokensPerTopic, with an exchange the merge) follows ggs_set_z."""
    for what in (order or row.exports):
        if what == "z":
            h.set_z(state["z"][z_slice], redraw_phi=False)
            if row.form == "count":
                h.init_phi()
        elif what == "phi":
            h.set_phi(state["phi"])
        else:
            h.set_iteration(state["iteration"])


def orders(row):
    return list(itertools.permutations(row.exports))


CUMULATIVE = ("mh_stats", "sparse_stats")                 # "cumulative since ggs_set_corpus": compare differences on one handle
OWN = ("n_sampled", "phi_mean")                           # a handle's own bookkeeping: pinned by expected_phi_mean


def snapshot(h, row):
    """Everything the row's handle exposes after a chain, by name.  With an exchange the counts, the count-form tables and the
    likelihoods gather: every rank calls snapshot at the same point."""
    s = {"z": h.get_z(), "phi": h.get_phi(), "iteration": h.iteration, "n_wk": h.get_type_topic_counts(), "n_k": h.get_topic_totals()}
    if row.theta:
        s["theta"] = h.get_theta()
    mean, n = h.get_phi_mean()
    s["n_sampled"] = n
    if mean is not None:
        s["phi_mean"] = mean
    if row.tables:
        s["alias_ps"], s["alias_a"], s["type_norm"] = h.alias_tables()
    if row.lists:
        s["nw"], s["lists"] = h.word_topic_lists()
    if row.mh:
        s["mh_stats"] = h.mh_stats()
    if row.sparse:
        s["sparse_stats"] = h.sparse_stats()
    if row.vs:
        s["vs_stats"] = h.vs_stats()
    s["model_log_likelihood"] = np.asarray(h.model_log_likelihood(), np.float64)
    if row.log_posterior:
        s["log_posterior"] = np.asarray(h.log_posterior(), np.float64)
    return s


def assert_same(a, b, tag, skip=()):
    """two snapshots, bit for bit in everything but the names in skip"""
    keys = (set(a) | set(b)) - set(skip)
    missing = sorted(k for k in keys if k not in a or k not in b)
    assert not missing, "%s: only one side has %s" % (tag, missing)
    for k in sorted(keys):
        assert_bit_equal(a[k], b[k], "%s: %s" % (tag, k))


def assert_is_oracle(snap, want, tag):
    """a handle's snapshot against oracle_state(): z, counts, Phi, theta, the iteration number, nzvsspalias' first two statistics"""
    for k in ("z", "n_wk", "n_k", "phi", "theta", "iteration"):
        if k in want and k in snap:
            assert_bit_equal(snap[k], want[k], "%s against the oracle: %s" % (tag, k))
    if "vs_first_two" in want and "vs_stats" in snap:
        assert_bit_equal(snap["vs_stats"][:2], want["vs_first_two"], tag + " against the oracle: undrawn and zero cells")


def zero_cells(phi):
    return int((np.asarray(phi) == 0.0).sum())


# ---- a world of ranks in one process ------------------------------------------------------------------------------------
def run_world(native, row, K, whole, world, mode, body, seed=SEED, doc_off=0, tok_off=0):
    """tests/ranks.py's run_ranks with a handle of the row's scheme (create) on every rank and the count exchange in `mode`"""
    return run_ranks(world, whole, lambda rank: create(native, row, K, seed), body, mode=mode, doc_off=doc_off, tok_off=tok_off)
