"""ggs_model_log_likelihood and ggs_log_posterior (csrc/ggs_loglik.hpp) against the exact sum of the oracle's terms.

Each side of each diagnostic must satisfy  |device - exact| <= (c + 2) * 2^-53 * sum|t|  with c the longest chain of
additions on the device, computed from the launch shape (tests/diagnostics_cases.py: chains(), where the derivation is
written down) -- never fitted to what the device returns.  tests/test_diagnostics_model.py establishes the reference on
the CPU.  On every case besides: the diagnostic is run-to-run identical, the pcgs-family diagnostic theta is the oracle's
to the bit, and a sweep after the diagnostics equals the oracle's (ggs, pcgs, collapsed) or the restatement's (spalias,
polyaurn): the diagnostics leave the chain alone.

Every check prints its ratio |device - exact| / (2^-53 * sum|t|) beside the c it had to stay under (pytest -s shows them)."""
import math

import numpy as np
import pytest

from tests import diagnostics_cases as DC
from tests import polyaurn_restatement as PR
from tests import spalias_restatement as SR
from tests.ranks import assert_bit_equal, run_ranks
from tests.test_parity_gpu import compare_state

pytestmark = pytest.mark.gpu

SEED, ZSEED = 5, 6
SCHEMES = ("ggs", "pcgs", "spalias", "polyaurn")


def flags_of(native, scheme):
    return {"ggs": 0, "pcgs": native.FLAG_PCGS, "spalias": native.FLAG_SPALIAS, "polyaurn": native.FLAG_POLYAURN,
            "collapsed": native.FLAG_COLLAPSED}[scheme]


def check_side(tag, what, got, terms, c):
    e = DC.exact(terms)
    err = abs(got - e.value)
    ratio = err / (DC.U * e.abs_sum) if e.abs_sum else (0.0 if err == 0 else float("inf"))
    print("RATIO %-44s %-8s %9.3f of c + 2 = %4d   (device %.17g, exact %.17g, n = %d)" % (tag, what, ratio, c + 2, got, e.value, e.n))
    assert err <= (c + 2) * DC.U * e.abs_sum, (tag, what, got, e.value, ratio, c + 2)
    return e


def state_pair(native, oracle, scheme, corpus, K, alpha, beta, z=None):
    """The device handle in the state a driver asks the diagnostics in, and an oracle state holding the same model.
    ggs, pcgs, collapsed: the oracle runs the same chain.  spalias, polyaurn: the device's z, Phi and iteration loaded into
    an oracle pcgs state.  The last token of the longest document is moved to topic K - 1 (DC.plant_last_topic); polyaurn's
    Phi gets zeros under tokens on top of those its Poisson draw left (DC.plant_phi_zeros)."""
    g = native.GGSHandle(K, corpus.num_types, alpha, beta, SEED, flags=flags_of(native, scheme))
    g.set_corpus(corpus.doc_ptr, corpus.tokens)
    o = oracle.OracleSampler(K, corpus.num_types, alpha, beta, SEED, threads=4)
    o.set_scheme("ggs" if scheme in ("ggs", "collapsed") else "pcgs")
    o.set_corpus(corpus.doc_ptr, corpus.tokens)
    lockstep = scheme in ("ggs", "pcgs", "collapsed")
    if z is not None:                                        # z by hand: no sweep, Phi drawn from its counts
        for s in (g, o):
            s.set_z(z, redraw_phi=False)
            s.init_phi()
    else:
        for s in (g, o) if lockstep else (g,):
            s.init_z_java_lcg(ZSEED)
            s.init_phi()
            if scheme == "collapsed" and s is o:
                s.collapsed_parallel_sweep(1)
            else:
                s.sweep(1)
        planted = DC.plant_last_topic(g.get_z(), corpus.doc_ptr, K)
        g.set_z(planted, redraw_phi=False)
        o.set_z(planted, redraw_phi=False)
    if scheme == "polyaurn":
        natural = DC.phi_zeros_under_tokens(g.get_phi(), g.get_z(), corpus.tokens)
        g.set_phi(DC.plant_phi_zeros(g.get_phi(), g.get_z(), corpus.tokens, corpus.doc_ptr))
        if corpus.num_tokens:
            assert DC.phi_zeros_under_tokens(g.get_phi(), g.get_z(), corpus.tokens) > 0
            assert K < 63 or natural > 0, "the Poisson draw itself left no zero under a token"
    if not lockstep:
        o.set_phi(g.get_phi())
        o.set_iteration(g.iteration)
    assert g.iteration == o.iteration
    return g, o


def check_diagnostics(native, oracle, scheme, corpus, K, alpha, beta, tag, z=None, sweep_after=True):
    g, o = state_pair(native, oracle, scheme, corpus, K, alpha, beta, z=z)
    lens = np.diff(corpus.doc_ptr)
    c = DC.chains(corpus.num_docs, K, corpus.num_types, int(lens.max()) if lens.size else 0)
    if corpus.num_tokens and z is None:
        assert (g.get_doc_topic_counts()[:, K - 1] > 0).any()                # the K % 64 tail of the lane loop carries a term
    tag = "%s %s" % (tag, scheme)
    # ---- model log likelihood
    gd, gt = g.model_log_likelihood()
    assert g.model_log_likelihood() == (gd, gt), "not run-to-run identical"
    td, tt = o.model_log_likelihood_terms()
    check_side(tag, "ll_doc", gd, td, c["ll_doc"])
    check_side(tag, "ll_topic", gt, tt, c["ll_topic"])
    # ---- log posterior
    if scheme != "collapsed":
        if scheme != "ggs":
            o.draw_diagnostic_theta()
        gd, gt = g.log_posterior()
        assert g.log_posterior() == (gd, gt), "not run-to-run identical"
        assert_bit_equal(g.get_theta(), o.get_theta(), tag + ": theta of the diagnostic")
        td, tt = o.log_posterior_terms()
        check_side(tag, "lp_doc", gd, td, c["lp_doc"])
        check_side(tag, "lp_topic", gt, tt, c["lp_topic"])
        assert g.model_log_likelihood() == g.model_log_likelihood()          # ... and after the theta draw as before it
    # ---- the chain goes on as if nothing had been asked
    if sweep_after:
        sweep_and_compare(g, o, scheme, corpus, K, alpha, beta, tag)
    g.close()


def sweep_and_compare(g, o, scheme, corpus, K, alpha, beta, tag):
    it = g.iteration + 1
    if scheme in ("ggs", "pcgs"):
        g.sweep(1)
        o.sweep(1)
        compare_state(g, o, tag + ": sweep after the diagnostics", theta=scheme == "ggs")
    elif scheme == "collapsed":
        g.sweep(1)
        o.collapsed_parallel_sweep(1)
        assert_bit_equal(g.get_z(), o.get_z(), tag + ": z after the diagnostics")
        assert_bit_equal(g.get_type_topic_counts(), o.get_type_topic_counts(), tag + ": n_wk after the diagnostics")
    else:
        z, phi = g.get_z().astype(np.int64), g.get_phi()
        if scheme == "polyaurn":
            PR.z_step(corpus.doc_ptr, corpus.tokens.astype(np.int64), z, phi, alpha, SEED, it)
            want_phi, _, _ = PR.phi_draw(PR.counts_of(corpus.tokens, z, K, corpus.num_types), beta, PR.threshold_of(0), SEED, it, False)
        else:
            SR.z_step(corpus.doc_ptr, corpus.tokens.astype(np.int64), z, phi, g.alias_tables(), SEED, it)
            o.set_iteration(it)
            o.set_z(z.astype(np.int32), redraw_phi=False)
            o.sample_phi()
            want_phi = o.get_phi()
        g.sweep(1)
        assert g.iteration == it
        assert_bit_equal(g.get_z(), z.astype(np.int32), tag + ": z after the diagnostics")
        assert_bit_equal(g.get_phi(), want_phi, tag + ": phi after the diagnostics")


# ---- K ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,K", DC.TOPIC_CASES)
def test_topic_list(native, oracle, scheme, K):
    """K = 1, 2, around the lane stride, odd (Kp = K + 1), and up to the widest rows each scheme supports, with a per-topic
    alpha from 0.01 to 5, on 41 = 4 n + 1 documents.  From K = 4095 the four histograms of a block pass 64 KiB."""
    check_diagnostics(native, oracle, scheme, DC.wide_corpus(K), K, DC.asymmetric_alpha(K), 0.01, "K=%d" % K)


@pytest.mark.parametrize("K", [64, 65, 257])
def test_topic_list_collapsed(native, oracle, K):
    check_diagnostics(native, oracle, "collapsed", DC.wide_corpus(K), K, DC.asymmetric_alpha(K), 0.01, "K=%d" % K)


def test_beyond_four_histograms_is_refused_at_create(native):
    """From K = 10239 the four K-long histograms of a block no longer fit 160 KiB and the diagnostics answer
    GGS_ERR_UNSUPPORTED by name (ll_check_topics).  No handle gets that far: ggs_create itself refuses K = 10240, under
    scheme ggs (no z kernel's LDS plan holds so wide a row) as under spalias (4096 topics at most), with
    GGS_ERR_UNSUPPORTED, never GGS_ERR_HIP -- that refusal is asserted here in place of values."""
    assert DC.MAX_TOPICS + 2 == DC.BEYOND_FOUR_HISTOGRAMS
    for scheme in ("ggs", "spalias"):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(DC.BEYOND_FOUR_HISTOGRAMS, 60, 0.1, 0.01, SEED, flags=flags_of(native, scheme))
        assert e.value.code == native.ERR_UNSUPPORTED, (scheme, e.value)


# ---- documents -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES + ("collapsed",))
@pytest.mark.parametrize("name", list(DC.DOCUMENT_SHAPES))
def test_document_shapes(native, oracle, name, scheme):
    """D = 1, 2, 3, 5 and 4 n + 1; nothing but empty documents; empty ones mixed in; one-token documents; a 40 000-token
    document among short ones; more documents than types (with a per-topic alpha)."""
    build, K, alpha, beta = DC.DOCUMENT_SHAPES[name]
    check_diagnostics(native, oracle, scheme, build(), K, DC.resolve_alpha(alpha, K), beta, name)


# ---- the topic side --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", SCHEMES)
def test_grid_passes(native, oracle, scheme):
    """V * K = 1 053 700 cells: the 262 144 threads of the fixed grid pass four times and a fifth that ends inside a block;
    K = 257 is odd, so the Phi kernel skips the pad column of every row."""
    build, K, alpha, beta = DC.GRID_PASSES
    check_diagnostics(native, oracle, scheme, build(), K, alpha, beta, "grid passes")


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_huge_count(native, oracle, scheme):
    """One word 2 000 000 times in one topic (z set by hand, no sweep before): lgS at a large argument, 50 documents of
    40 003 tokens whose log(phi) terms a lane adds 626 at a time.  Under ggs no z step has drawn a theta: the rows are
    zeros on both sides, as for an empty document."""
    c, z = DC.huge_count_corpus()
    check_diagnostics(native, oracle, scheme, c, 4, 0.1, 0.01, "2M in one cell", z=z)


# ---- shards ----------------------------------------------------------------------------------------------------------
def _shard_rank(native, whole, K, alpha, beta, scheme, z0):
    """(make_handle, body) of a rank for tests/ranks.py's run_ranks"""
    def make_handle(rank):
        return native.GGSHandle(K, whole.num_types, alpha, beta, SEED, flags=flags_of(native, scheme))

    def body(h, rank, sub, tok_base):
        h.set_z(z0[tok_base:tok_base + sub.num_tokens], redraw_phi=True)
        h.sweep(1)
        h.check_invariants()                       # collective: gathers the corpus-wide counts
        r = dict(ll=h.model_log_likelihood(), lp=h.log_posterior())
        r["again"] = (h.model_log_likelihood(), h.log_posterior())
        r["theta"] = h.get_theta()
        h.sweep(1)
        r["z"], r["phi"] = h.get_z(), h.get_phi()
        return r
    return make_handle, body


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
@pytest.mark.parametrize("cuts", DC.SHARD_CUTS)
def test_document_shards(native, oracle, cuts, scheme):
    """One corpus cut two and three ways (uneven, one shard empty), a handle per shard with the callback exchange.  The
    document sides of both diagnostics add up to the whole corpus' exact document side within the sum of the shards' bounds;
    every shard's topic side is the whole's within its bound; under pcgs the later shards (doc_base != 0) draw rows
    doc_base... of the diagnostic theta to the bit; the sweep after equals the unsharded oracle's."""
    from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
    whole = DC.shard_corpus()
    K, alpha, beta = 33, DC.asymmetric_alpha(33), 0.01
    world = len(cuts) - 1
    z0 = java_lcg_initial_z(whole.num_tokens, K, ZSEED)
    out = run_ranks(world, whole, *_shard_rank(native, whole, K, alpha, beta, scheme, z0), all_to_all=False, cuts=cuts)
    o = oracle.OracleSampler(K, whole.num_types, alpha, beta, SEED, threads=4)
    o.set_scheme(scheme)
    o.set_corpus(whole.doc_ptr, whole.tokens)
    o.set_z(z0, redraw_phi=True)
    o.sweep(1)
    if scheme == "pcgs":
        o.draw_diagnostic_theta()
    theta = o.get_theta()
    lens = np.diff(whole.doc_ptr)
    tag = "shards %r %s" % (cuts, scheme)
    offsets = dict(zip(("ll", "lp"), DC.doc_side_terms_by_document(o.get_doc_topic_counts(), whole.doc_ptr, o.get_z(), whole.tokens, whole.num_types)))
    for name, terms in (("ll", o.model_log_likelihood_terms()), ("lp", o.log_posterior_terms())):
        doc = DC.exact(terms[0])
        off = offsets[name]
        assert off[-1] + (name == "ll") == doc.n
        # D * lgS(alphaSum), the model log likelihood's last document-side term: a shard adds D_r * lgS(alphaSum) instead, one
        # rounded product each -- world + 1 roundings of at most 2^-53 |D * lgS(alphaSum)| between the shards' sum and the whole's
        const = abs(float(terms[0][-1])) if name == "ll" else 0.0
        bound = (world + 1) * DC.U * const + DC.U * abs(doc.value)           # ... and fsum's one rounding of the shards' sum
        for r in range(world):
            lo, hi = cuts[r], cuts[r + 1]
            assert out[r]["again"][name == "lp"] == out[r][name], "not run-to-run identical"
            c = DC.chains(hi - lo, K, whole.num_types, int(lens[lo:hi].max()) if hi > lo else 0)
            check_side(tag + " rank %d" % r, name + "_topic", out[r][name][1], terms[1], c[name + "_topic"])
            # the shard's bound: its own chain lengths on the magnitudes of its own documents' terms
            mine = DC.exact(terms[0][off[lo]:off[hi]])
            bound += (c[name + "_doc"] + 2) * DC.U * (mine.abs_sum + const * (hi - lo) / whole.num_docs * (1 + 1e-9))
        got = math.fsum(out[r][name][0] for r in range(world))
        print("RATIO %-44s %-8s %9.3f of %.1f" % (tag, name + "_doc", abs(got - doc.value) / (DC.U * doc.abs_sum), bound / (DC.U * doc.abs_sum)))
        assert abs(got - doc.value) <= bound, (tag, name, got, doc.value)
    for r in range(world):
        assert_bit_equal(out[r]["theta"], theta[cuts[r]:cuts[r + 1]], tag + ": theta rows of rank %d" % r)
    o.sweep(1)
    assert_bit_equal(np.concatenate([p["z"] for p in out]), o.get_z(), tag + ": z after the diagnostics")
    for r in range(world):
        assert_bit_equal(out[r]["phi"], o.get_phi(), tag + ": phi after the diagnostics, rank %d" % r)
