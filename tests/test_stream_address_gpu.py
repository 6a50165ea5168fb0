"""Every drawing kernel's stream address at its full width (tests/stream_address.py): a 64-bit seed with both key words in
use, an iteration number just below INT32_MAX, a tok_base at which the global token index passes 2^32 inside a document and a
doc_base at which the theta element passes 2^32 inside a row -- the corner a Params field narrowed to 32 bits, a high word
hoisted out of the lane, an int product or a 16-bit iteration would get wrong while every low-corner test stayed green.
Bit equality with the oracle throughout, no tolerance anywhere; tests/test_stream_address_model.py shows on the CPU that the
oracle is right at these corners and that the cases tell each such mistake from the truth.

  a  every scheme (tests/handle_lifecycle.py, ROWS) x K in {20, 200}: one z step given Phi (the count form: one sweep), then
     two whole sweeps, then the phi mean's gating at these iteration numbers
  b  every z kernel form of ggs, pcgs and collapsed a debug switch reaches (the environments of tests/test_knife_edge_gpu.py,
     CASES, and the collapsed forms as tests/test_collapsed_gpu.py forces them), launch_info() saying which kernel ran
  c  the theta kernel's paths (the gamma queue capped at 0 and 5 and as it is; symmetric alpha, with class-A tables, and
     asymmetric, without) and pcgs's diagnostic theta, in the rows around the crossing and everywhere else
  d  the held-out estimator at a test doc_base where global doc * particles + particle passes 2^32 inside a document
  e  the Phi side.  elem = k * V + v cannot reach 2^32 in a test of seconds (a Phi of 34 GB), so the functions the Phi kernels
     call are pinned instead -- the gamma draw, its first try and the Poisson draw over elements 2^32 - 100 ... 2^32 + 99 under
     purposes PHI and INIT_PHI: THIS IS THE LIMIT of what a small test reaches there.  The key words and the iteration of
     every Phi, Poisson and variable-selection draw are covered at handle level by a and b.
  f  two ranks whose boundary is not the crossing: rank 0 holds it, rank 1 starts past 2^32; both count-exchange modes
  g  the ends of the iteration range (include/ggs_hip.h at ggs_set_iteration): the last two sweeps, the refusals of every
     entry point that steps the iteration (ggs_group_sweep through a group of the one device there is)"""
import numpy as np
import pytest

from tests import handle_lifecycle as H
from tests import stream_address as S
from tests.handle_lifecycle import ROWS, assert_bit_equal, assert_is_oracle, assert_same
from tests.test_knife_edge_gpu import CASES
from tests.test_knife_edge_model import repeated_word_corpus, unique_word_corpus

pytestmark = pytest.mark.gpu

NAMES = [r.name for r in ROWS]
ALPHA, BETA = 0.1, 0.01

# ---- the forms of case b: (form, K) picked from CASES, the environment taken from there ------------------------------------
PICK = {"tile": 100, "sliced32": 20, "sliced64": 100, "hot_split": 20, "hot_fused": 100, "warm": 20, "stream1": 200, "stream2": 48, "pcgs_lane": 20,
        "pcgs_stream": 20, "pcgs_wave": 200}
FORMS = [c for c in CASES if PICK.get(c[0]) == c[1]]
assert sorted(c[0] for c in FORMS) == sorted(PICK)
# scheme=collapsed: lane per document below 97 topics, wave per document from there on, the two-pass kernel where forced
FORMS += [("collapsed_lane", 20, {}, "ragged", "collapsed", "lane"), ("collapsed_wave", 200, {}, "ragged", "collapsed", "wave"),
          ("collapsed_two_pass", 20, {"GGS_DEBUG_PCGS_STREAM": "1"}, "ragged", "collapsed", "lane")]
TABLE_ROWS = {"hot_split": (0, 24), "hot_fused": (0, 24), "warm": (8, 24)}     # frequency ranks of the words whose chunks must straddle the crossing


def form_corpus(form, K, kind, scheme):
    """the form's usual small corpus (tests/test_knife_edge_gpu.py make_knife_edge, tests/test_collapsed_gpu.py)"""
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    if scheme == "pcgs":
        return unique_word_corpus(300, 5, 900 + K)
    if scheme == "collapsed":
        return random_corpus(130, 300, 90, seed=K + 1, empty_every=7)
    if kind == "repeated":
        return repeated_word_corpus(300, 30, 300, 50 + K)
    return unique_word_corpus(80 if K <= 160 else 40, 26, K)


def ranked_words(c, lo, hi):
    """the words of frequency ranks lo ... hi - 1 whose rank no tie can move across lo or hi"""
    n = np.bincount(c.tokens, minlength=c.num_types)
    order = np.argsort(-n, kind="stable")
    above, below = (n[order[lo - 1]] if lo else None), n[order[hi]]
    return [int(w) for w in order[lo:hi] if n[w] > below and (above is None or n[w] < above)]


def form_corner(form, K, kind, scheme):
    """(corpus, doc, offset): where the token crossing goes.  Table forms: inside a document that holds tokens of table words
    on both sides of it, so that a chunk of the table kernel has lanes below and above 2^32."""
    c = form_corpus(form, K, kind, scheme)
    if form not in TABLE_ROWS:
        offset = 2 if scheme == "pcgs" else 5                            # pcgs's usual documents have at most 5 tokens
        return c, S.pick_doc(c, offset), offset
    words = ranked_words(c, *TABLE_ROWS[form])
    assert len(words) >= 4, (form, words)
    mine = np.isin(c.tokens, words)
    for d in range(c.num_docs // 2, c.num_docs - 1):
        b, e = int(c.doc_ptr[d]), int(c.doc_ptr[d + 1])
        for offset in range(3, (e - b - 1) // 2 + 1):
            if e - b > 2 * offset and (b + offset) % 64 and mine[b:b + offset].any() and mine[b + offset:e].any():
                return c, d, offset
    raise AssertionError("%s: no document holds table words on both sides of a crossing" % form)


def corner_cases():
    """(corpus, K, doc, offset) of every case below that calls S.bases -- tests/test_stream_address_model.py walks them without a device"""
    a = H.corpus("A")
    for K in S.KS:
        yield a, K, S.pick_doc(a), 5
    for form, K, _env, kind, scheme, _want in FORMS:
        c, doc, offset = form_corner(form, K, kind, scheme)
        yield c, K, doc, offset


def z_mismatch(zg, zo, cross, tag):
    bad = np.asarray(zg) != np.asarray(zo)
    assert not bad.any(), "%s: z differs in %d of %d tokens; before / at / after the crossing (token %d): %s" % (
        tag, bad.sum(), bad.size, cross, S.split_at_crossing(bad, cross))


# ---- a. every scheme at the corner ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("name", NAMES)
def test_every_scheme_at_the_corner(native, name, K):
    row, c = H.ROW[name], H.corpus("A")
    doc = S.pick_doc(c)
    doc_base, tok_base = S.bases(c, K, doc)
    cross, z0 = S.crossing_token(c, doc), H.initial_z(c, K)
    o = H.Chain(row, K, c, z0, S.IT0, seed=S.SEED, doc_base=doc_base, tok_base=tok_base)
    h = H.create(native, row, K, S.SEED)
    try:
        h.set_iteration(S.IT0)
        H.start(h, c, z0, doc_base, tok_base)
        if row.z_given_phi:
            h.sample_z_given_phi(1)
            o.run((("zgiven", 1),))
        else:
            h.sweep(1)
            o.run((("sweep", 1),))
        assert h.iteration == o.iteration == S.IT0 + 1
        z_mismatch(h.get_z(), o.state()["z"], cross, "%s K=%d, first step" % (name, K))
        phis = {}
        for _ in range(2):
            h.sweep(1)
            if row.mean != "none":
                phis[h.iteration] = h.get_phi()
        o.run((("sweep", 2),))
        snap, want = H.snapshot(h, row), o.state()
        assert want["iteration"] == S.IT0 + 3
        z_mismatch(snap["z"], want["z"], cross, "%s K=%d, after two sweeps" % (name, K))
        assert_is_oracle(snap, want, "%s K=%d at the corner" % (name, K))
        # the gating rule at iterations near 2^31: IT0 + 2 is odd (not accepted), IT0 + 3 even and past the burn-in (accepted)
        mean, n = H.expected_phi_mean(row, phis)
        assert n == (0 if row.mean == "none" else 1) and snap["n_sampled"] == n
        assert ("phi_mean" in snap) == (mean is not None)
        if mean is not None:
            assert_bit_equal(snap["phi_mean"], mean, name + ": phi mean")
        h.check_invariants()
    finally:
        h.close()


# ---- b. every z kernel form -----------------------------------------------------------------------------------------------
def assert_kernel(info, want):
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


@pytest.mark.parametrize("form,K,env,kind,scheme,want", FORMS, ids=["%s-K%d" % (c[0], c[1]) for c in FORMS])
def test_every_z_kernel_form_at_the_corner(native, oracle, monkeypatch, form, K, env, kind, scheme, want):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c, doc, offset = form_corner(form, K, kind, scheme)
    doc_base, tok_base = S.bases(c, K, doc, offset)
    cross = S.crossing_token(c, doc, offset)
    z0 = oracle.jrandom_ints(K, K, c.num_tokens)
    g = native.GGSHandle(K, c.num_types, ALPHA, BETA, S.SEED, flags=native.FLAG_PARANOID | native.SCHEME_FLAGS[scheme])
    o = oracle.OracleSampler(K, c.num_types, ALPHA, BETA, S.SEED, threads=4)
    try:
        if scheme == "pcgs":
            o.set_scheme("pcgs")
        for s in (g, o):
            s.set_iteration(S.IT0)
            s.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
            s.set_z(z0, redraw_phi=False)
            s.init_phi()
        if scheme == "collapsed":                                          # no Phi to condition on: two sweeps
            g.sweep(1)
            o.collapsed_parallel_sweep(1)
        else:
            g.sample_z_given_phi(1)
            o.set_iteration(o.iteration + 1)
            o.z_step()
            o.update_counts()
        info = g.launch_info()
        assert_kernel(info, want)
        tag = "%s K=%d (%s)" % (form, K, info["z_kernel"])
        z_mismatch(g.get_z(), o.get_z(), cross, tag + ", first step")
        assert (o.get_z() != z0).mean() > 0.05                             # the step moves tokens (few where every word has one token: its own count leads its column)
        g.sweep(1)
        if scheme == "collapsed":
            o.collapsed_parallel_sweep(1)
        else:
            o.sweep(1)
        assert g.iteration == o.iteration == S.IT0 + 2
        z_mismatch(g.get_z(), o.get_z(), cross, tag + ", after the sweep")
        assert_bit_equal(g.get_type_topic_counts(), o.get_type_topic_counts(), tag + ": n_wk")
        if scheme != "collapsed":
            assert_bit_equal(g.get_phi(), o.get_phi(), tag + ": phi")
        if scheme == "ggs":
            assert_bit_equal(g.get_theta(), o.get_theta(), tag + ": theta")
        g.check_invariants()
    finally:
        g.close()
        o.close()


# ---- c. the theta kernel's paths across the row crossing ------------------------------------------------------------------
def theta_rows(got, want, doc, tag):
    for d in (doc - 1, doc, doc + 1):
        assert_bit_equal(got[d], want[d], "%s: theta row %+d of the crossing's" % (tag, d - doc))
    assert_bit_equal(got, want, tag + ": theta")


@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("alpha", ["symmetric", "asymmetric"])
@pytest.mark.parametrize("queue", [None, "0", "5"])
def test_theta_paths_across_the_row_crossing(native, oracle, monkeypatch, queue, alpha, K):
    if queue is not None:
        monkeypatch.setenv("GGS_DEBUG_GAMMA_QUEUE", queue)
    c = H.corpus("A")
    doc = S.pick_doc(c)
    doc_base, tok_base = S.bases(c, K, doc)
    a = ALPHA if alpha == "symmetric" else np.linspace(0.03, 1.7, K)     # shapes on both sides of 1 where a count is 0
    g = native.GGSHandle(K, H.V, a, BETA, S.SEED, flags=native.FLAG_PARANOID)
    o = oracle.OracleSampler(K, H.V, a, BETA, S.SEED, threads=4)
    try:
        for s in (g, o):
            s.set_iteration(S.IT0)
            s.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
            s.set_z(H.initial_z(c, K), redraw_phi=False)
            s.init_phi()
        for sweep in (1, 2):                                               # the second sweep's theta may be the one drawn ahead
            g.sweep(1)
            o.sweep(1)
            theta_rows(g.get_theta(), o.get_theta(), doc, "queue %s, %s alpha, K=%d, sweep %d" % (queue, alpha, K, sweep))
        assert_bit_equal(g.get_z(), o.get_z(), "z")
    finally:
        g.close()
        o.close()


@pytest.mark.parametrize("K", S.KS)
def test_pcgs_diagnostic_theta_across_the_row_crossing(native, oracle, K):
    c = H.corpus("A")
    doc = S.pick_doc(c)
    doc_base, tok_base = S.bases(c, K, doc)
    g = native.GGSHandle(K, H.V, ALPHA, BETA, S.SEED, flags=native.FLAG_PARANOID | native.FLAG_PCGS)
    o = oracle.OracleSampler(K, H.V, ALPHA, BETA, S.SEED, threads=4)
    o.set_scheme("pcgs")
    try:
        for s in (g, o):
            s.set_iteration(S.IT0)
            s.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
            s.set_z(H.initial_z(c, K), redraw_phi=False)
            s.init_phi()
            s.sweep(1)
        o.draw_diagnostic_theta()
        g.log_posterior()
        theta_rows(g.get_theta(), o.get_theta(), doc, "pcgs diagnostic theta, K=%d" % K)
    finally:
        g.close()
        o.close()


# ---- d. held-out ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("particles", [10, 12])
def test_heldout_across_the_element_crossing(native, oracle, particles):
    """elem = global test doc * numParticles + particle: with doc_base = 2^32 // P - 3 the fourth test document's particles
    straddle 2^32 (2^32 mod 10 = 6, mod 12 = 4).  The comparison is tests/test_heldout.py's _same: per-document bit equality."""
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    from tests.test_heldout import _same
    assert 0 < S.TWO32 % particles < particles - 1
    K = 20
    full = random_corpus(140, 200, 40, seed=77, empty_every=17)
    train, _, _ = full.shard(0, 120)
    test, _, _ = full.shard(120, 140)
    assert np.diff(test.doc_ptr)[2:5].min() > 0                            # the documents around the crossing are not empty
    g = native.GGSHandle(K, train.num_types, ALPHA, BETA, S.SEED)
    o = oracle.OracleSampler(K, train.num_types, ALPHA, BETA, S.SEED, threads=4)
    try:
        for s in (g, o):
            s.set_iteration(S.IT0 - 2)
            s.set_corpus(train.doc_ptr, train.tokens)
            s.set_z(oracle.jrandom_ints(5, K, train.num_tokens), redraw_phi=False)
            s.init_phi()
            s.sweep(2)
        assert g.iteration == S.IT0
        doc_base = S.TWO32 // particles - 3
        assert (doc_base + 3) * particles < S.TWO32 < (doc_base + 4) * particles
        at = _same(g, o, test, particles, doc_base=doc_base)
        assert at != _same(g, o, test, particles, doc_base=doc_base - 100)    # the base reaches the streams
    finally:
        g.close()
        o.close()


# ---- e. the functions the Phi kernels call --------------------------------------------------------------------------------
@pytest.mark.parametrize("purpose", [S.PURPOSE_PHI, S.PURPOSE_INIT_PHI])
def test_phi_side_draws_across_the_element_crossing(native, oracle, purpose):
    from tests import polyaurn_restatement as PR
    elem0, n = S.TWO32 - 100, 200
    shape = np.where(np.arange(n) % 2 == 0, 0.01, 2.01) + (np.arange(n) % 7)          # beta + count, on both sides of 1
    want = oracle.gammas(S.SEED, S.IT0, purpose, elem0, shape)
    got, st = native.debug_draw("gamma", S.SEED, S.IT0, purpose, elem0, shape=shape)
    assert st == 0
    assert_bit_equal(got, want, "gamma draws of elements 2^32 - 100 ... 2^32 + 99")
    # the way the theta and Phi kernels draw: a straight-line first try, the general loops for what it leaves over
    first, st = native.debug_draw("gamma_first_try", S.SEED, S.IT0, purpose, elem0, shape=shape)
    assert st == 0
    assert_bit_equal(first, want, "gamma, first try + general")
    marked, _ = native.debug_draw("gamma_first_try_marked", S.SEED, S.IT0, purpose, elem0, shape=shape)
    settled = np.signbit(marked)
    assert_bit_equal(np.abs(marked), want, "gamma, marked")
    assert settled[:100].sum() > 50 and settled[100:].sum() > 50           # the first try settles most elements on either side of 2^32
    mine = [S.gamma_first_try(S.SEED, S.IT0, purpose, elem0 + i, float(shape[i])) for i in range(n)]
    both = [i for i in range(n) if mine[i] is not None]
    assert len(both) > 80
    assert_bit_equal(first[both], np.array([mine[i] for i in both]), "first tries against the direct statement")
    u, st = native.debug_draw("uniform", S.SEED, S.IT0, purpose, elem0, n)
    assert_bit_equal(u, S.first_uniforms(S.SEED, S.IT0, purpose, elem0, n), "uniforms against the direct statement")
    counts = (np.arange(n) * 37 % 250).astype(np.int32)                                # below and above the table's threshold of 100
    for beta in (0.01, 0.3):
        x = native.debug_poisson(counts, beta, 100, S.SEED, S.IT0, purpose, elem0)
        assert_bit_equal(x.astype(np.int64), PR.poisson_draw(counts, beta, 100, S.SEED, S.IT0, purpose, elem0), "Poisson draws, beta %g" % beta)


# ---- f. two ranks whose boundary is not the crossing ----------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["dense", "sparse"])
@pytest.mark.parametrize("name", ["ggs", "adlda"])
def test_two_ranks_around_the_crossing(native, name, mode):
    """The whole corpus offset so that the token crossing lies in rank 0's shard (not at its end) and rank 1 starts past 2^32;
    the theta crossing likewise in a row of rank 0.  Compared with the oracle over the whole corpus at the same offset.  With
    an exchange the z kernels count their own draws (atomicAdd) where the plan lets them."""
    row, c, K, world = H.ROW[name], H.corpus("A"), 20, 2
    half = H.shard_of(c, 0, world)[0]
    doc = S.pick_doc(c, start=half.num_docs // 2)
    assert doc < half.num_docs - 1
    doc_base, tok_base = S.bases(c, K, doc)
    cross, z0 = S.crossing_token(c, doc), H.initial_z(c, K)
    assert cross < half.num_tokens - 1 and tok_base + half.num_tokens > S.TWO32
    want = H.Chain(row, K, c, z0, S.IT0, seed=S.SEED, doc_base=doc_base, tok_base=tok_base).run((("sweep", 2),)).state()

    def body(h, rank, sub, tb):
        h.set_iteration(S.IT0)
        h.set_z(z0[tb:tb + sub.num_tokens], redraw_phi=False)
        h.init_phi()
        h.sweep(2)
        h.check_invariants()
        return H.snapshot(h, row)

    out = H.run_world(native, row, K, c, world, mode, body, seed=S.SEED, doc_off=doc_base, tok_off=tok_base)
    z_mismatch(np.concatenate([o["z"] for o in out]), want["z"], cross, "%s, %s exchange: z of the ranks" % (name, mode))
    if row.theta:
        assert_bit_equal(np.concatenate([o["theta"] for o in out]), want["theta"], name + ": theta of the ranks")
    for r, o in enumerate(out):
        for k in ("n_wk", "n_k", "phi", "iteration"):
            assert_bit_equal(o[k], want[k], "%s rank %d: %s" % (name, r, k))


# ---- g. the ends of the iteration range -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_last_iterations_and_the_refusals(native, name):
    row, c, K = H.ROW[name], H.corpus("A"), 20
    z0 = H.initial_z(c, K)
    last = S.INT32_MAX
    want = H.Chain(row, K, c, z0, last - 2, seed=S.SEED).run((("sweep", 2),)).state()
    assert want["iteration"] == last
    h = H.create(native, row, K, S.SEED)
    try:
        h.set_iteration(last - 2)
        H.start(h, c, z0)
        before = H.snapshot(h, row)
        with pytest.raises(native.GGSError) as e:                          # three sweeps in one call: refused as a whole
            h.sweep(3)
        assert e.value.code == native.ERR_STATE
        assert_same(H.snapshot(h, row), before, name + ": after a refused call of three sweeps")
        phis = {}
        for _ in range(2):
            h.sweep(1)
            if row.mean != "none":
                phis[h.iteration] = h.get_phi()
        snap = H.snapshot(h, row)
        assert_is_oracle(snap, want, name + " at INT32_MAX")
        mean, n = H.expected_phi_mean(row, phis)                           # INT32_MAX - 1 is even: accepted
        assert snap["n_sampled"] == n == (0 if row.mean == "none" else 1)
        if mean is not None:
            assert_bit_equal(snap["phi_mean"], mean, name + ": phi mean")
        calls = [lambda: h.sweep(1), h.sweep_begin]
        if row.z_given_phi:
            calls.append(lambda: h.sample_z_given_phi(1))
        if name == "collapsed":
            calls.append(lambda: h.collapsed_serial_sweep(1, 1))
        for call in calls:
            with pytest.raises(native.GGSError) as e:
                call()
            assert e.value.code == native.ERR_STATE, e.value
            assert "INT32_MAX" in str(e.value)
            assert_same(H.snapshot(h, row), snap, name + ": after a refused step")
        with pytest.raises(native.GGSError) as e:
            h.set_iteration(-1)
        assert e.value.code == native.ERR_BAD_ARG
        with pytest.raises(native.GGSError):
            h.set_iteration(-2 ** 31)
        assert h.iteration == last
        h.set_iteration(0)                                                 # the range's other end is allowed
        h.sweep(1)
        assert h.iteration == 1
        h.check_invariants()
    finally:
        h.close()


def test_group_sweep_is_refused_past_the_last_iteration(native):
    """ggs_group_sweep with the one device there is (scheme adlda, as tests/test_adlda_gpu.py drives a group): two sweeps from
    INT32_MAX - 1 are refused as a whole, one is the restatement's, and there is none behind it."""
    row, c, K = H.ROW["adlda"], H.corpus("A"), 20
    z0, last = H.initial_z(c, K), S.INT32_MAX
    want = H.Chain(row, K, c, z0, last - 1, seed=S.SEED).run((("sweep", 1),)).state()
    g = native.GGSGroup(K, H.V, H.ALPHA, row.beta, S.SEED, device_ids=[0], flags=native.FLAG_ADLDA)
    try:
        h = g.handles[0]
        h.set_corpus(c.doc_ptr, c.tokens)
        h.set_iteration(last - 1)
        g.set_z([z0], redraw_phi=True)
        with pytest.raises(native.GGSError) as e:
            g.sweep(2)
        assert e.value.code == native.ERR_STATE and "INT32_MAX" in str(e.value)
        assert h.iteration == last - 1
        assert_bit_equal(h.get_z(), z0, "z after the refused call")
        g.sweep(1)
        g.gather_counts()
        assert h.iteration == last
        assert_bit_equal(h.get_z(), want["z"], "z at INT32_MAX")
        assert_bit_equal(h.get_type_topic_counts(), want["n_wk"], "n_wk at INT32_MAX")
        with pytest.raises(native.GGSError) as e:
            g.sweep(1)
        assert e.value.code == native.ERR_STATE
        assert h.iteration == last
        assert_bit_equal(h.get_z(), want["z"], "z after the refused sweep")
    finally:
        g.close()
