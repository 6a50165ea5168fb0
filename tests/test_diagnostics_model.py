"""The reference that tests/test_diagnostics_gpu.py judges the diagnostic kernels by, established on the CPU first.

The oracle hands out the terms its Java-order loops add (orc_model_log_likelihood_terms, orc_log_posterior_terms); the
reference value of a side is math.fsum of them.  Here: the oracle's own running sums lie within the textbook bound of that
exact sum (which also proves the exported terms are the terms), the exact sums agree with independent formulas (scipy's
gammaln, plain numpy), over every shape of the GPU module, and the inputs hit the edges they are there for."""
import math

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.sampler import model_log_likelihood
from tests import diagnostics_cases as DC
from tests import polyaurn_restatement as PR

SEED, ZSEED = 5, 6


def oracle_state(oracle, scheme, corpus, K, alpha, beta, plant=True, z=None):
    """An oracle state of the kind the device holds when a diagnostic is asked for.  ggs: theta of the last z step.  pcgs:
    a fresh diagnostic theta.  polyaurn: the pcgs state with a Poisson-drawn Phi (exact zeros) in place of the Dirichlet one."""
    o = oracle.OracleSampler(K, corpus.num_types, alpha, beta, SEED, threads=4)
    o.set_scheme("ggs" if scheme == "ggs" else "pcgs")
    o.set_corpus(corpus.doc_ptr, corpus.tokens)
    if z is None:
        o.init_z_java_lcg(ZSEED)
        o.init_phi()
        o.sweep(1)
        if plant:
            o.set_z(DC.plant_last_topic(o.get_z(), corpus.doc_ptr, K), redraw_phi=False)
    else:
        o.set_z(z, redraw_phi=False)
        o.init_phi()
    if scheme == "polyaurn":
        phi, _, _ = PR.phi_draw(o.get_topic_type_counts(), beta, PR.threshold_of(0), SEED, o.iteration, False)
        o.natural_zeros = DC.phi_zeros_under_tokens(phi, o.get_z(), corpus.tokens)
        o.set_phi(DC.plant_phi_zeros(phi, o.get_z(), corpus.tokens, corpus.doc_ptr))
    if scheme != "ggs":
        o.draw_diagnostic_theta()
    return o


def running_sum_bound(e):
    """|running sum - exact| <= (n - 1) * 2^-53 * sum|t|: the textbook bound of a running sum (Higham, Accuracy and
    Stability of Numerical Algorithms, eq. 4.4, to first order)."""
    return max(e.n - 1, 0) * DC.U * e.abs_sum


def check_reference(o, corpus, alpha, beta, tag):
    """items 1 and 2 of the module's docstring on one state; returns the four Exact sides"""
    K = o.K
    sides = {}
    for name, value, terms in (("ll", o.model_log_likelihood(), o.model_log_likelihood_terms()),
                               ("lp", o.log_posterior(), o.log_posterior_terms())):
        for side, v, t in zip(("doc", "topic"), value, terms):
            e = DC.exact(t)
            sides[name + "_" + side] = e
            print("%s %s_%s: running %.17g exact %.17g, off by %.3g of a bound of %.3g (n = %d)"
                  % (tag, name, side, v, e.value, abs(v - e.value), running_sum_bound(e), e.n))
            assert abs(v - e.value) <= running_sum_bound(e), (tag, name, side, v, e.value)
            # the terms are the terms: added in order by a running double they give the oracle's result to the bit
            acc = 0.0
            for x in t.tolist():
                acc += x
            assert acc == v, (tag, name, side, acc, v)
    # the number of terms is what the loops visit
    n_dk, n_wk = o.get_doc_topic_counts(), o.get_type_topic_counts()
    D, V = corpus.num_docs, corpus.num_types
    assert sides["ll_doc"].n == int((n_dk > 0).sum()) + D + 1
    assert sides["ll_topic"].n == int((n_wk > 0).sum()) + K + 2
    z = o.get_z()
    doc_of = np.repeat(np.arange(D), np.diff(corpus.doc_ptr))
    cells = np.unique((doc_of.astype(np.int64) * K + z) * V + corpus.tokens).size
    assert sides["lp_doc"].n == cells + D * K
    assert sides["lp_topic"].n == K * V
    # independent formulas, at the tolerances tests/test_parity_gpu.py states for them
    a = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    ll = sides["ll_doc"].value + sides["ll_topic"].value
    direct = model_log_likelihood(n_dk, n_wk, o.get_topic_totals(), a, beta)
    # relative to the result, as the parity test has it; where the sides are sums of nothing but cancelling constants
    # (no token anywhere) the result is 0 and the same 1e-6 is taken of the terms' magnitude
    scale = abs(direct) if corpus.num_tokens else sides["ll_doc"].abs_sum + sides["ll_topic"].abs_sum
    assert abs(ll - direct) <= 1e-6 * scale, (tag, ll, direct)
    phi, theta = o.get_phi(), o.get_theta()
    lp = sides["lp_doc"].value + sides["lp_topic"].value
    direct = (np.log(phi[z, corpus.tokens] + 1e-12).sum() + ((n_dk.astype(np.float64) + a - 1.0) * np.log(theta + 1e-12)).sum()
              + (beta - 1.0) * np.log(phi + 1e-12).sum())
    assert abs(lp - direct) <= 1e-9 * abs(direct), (tag, lp, direct)
    return sides


def last_topic_is_hit(o, K):
    return bool((o.get_doc_topic_counts()[:, K - 1] > 0).any())


# ---- the exported terms ------------------------------------------------------------------------------------------------
def test_terms_leave_the_oracle_results_alone(oracle, cats):
    """Asking for the terms changes neither the state nor the running sums; a short buffer is not overrun."""
    import ctypes as C
    o = oracle_state(oracle, "ggs", cats, 20, 5.0, 7.0)
    before = (o.model_log_likelihood(), o.log_posterior())
    o.model_log_likelihood_terms()
    o.log_posterior_terms()
    assert (o.model_log_likelihood(), o.log_posterior()) == before
    buf = np.full(8, -1.0)
    n = oracle.lib().orc_log_posterior_terms(o._h, 1, buf.ctypes.data_as(C.POINTER(C.c_double)), 5)
    assert n == 20 * cats.num_types and (buf[5:] == -1.0).all() and (buf[:5] != -1.0).all()


def test_running_sum_bound_would_notice_a_dropped_term(oracle, cats):
    """The bound is tight enough to be a check: the exact sum without one ordinary term is outside it."""
    o = oracle_state(oracle, "ggs", cats, 20, 5.0, 7.0)
    for terms, value in zip(o.log_posterior_terms() + o.model_log_likelihood_terms(), o.log_posterior() + o.model_log_likelihood()):
        e = DC.exact(terms[:-1])
        assert abs(value - e.value) > running_sum_bound(e)


# ---- the shape list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,K", DC.TOPIC_CASES_CPU)
def test_topic_list(oracle, K, scheme):
    c = DC.wide_corpus(K)
    alpha = DC.asymmetric_alpha(K)
    assert K == 1 or (alpha.min() == 0.01 and alpha.max() == 5.0)
    o = oracle_state(oracle, scheme, c, K, alpha, 0.01)
    assert c.num_docs % 4 == 1
    assert last_topic_is_hit(o, K), "no document counts a token in topic K - 1: the K % 64 tail is not exercised"
    if scheme == "polyaurn":
        assert DC.phi_zeros_under_tokens(o.get_phi(), o.get_z(), c.tokens) >= 10, "no token of the corpus sits on an exact zero of Phi"
        assert K < 63 or o.natural_zeros > 0, "the Poisson draw itself left no zero under a token"
    check_reference(o, c, alpha, 0.01, "K=%d %s" % (K, scheme))


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "polyaurn"])
@pytest.mark.parametrize("name", list(DC.DOCUMENT_SHAPES))
def test_document_shapes(oracle, name, scheme):
    build, K, alpha, beta = DC.DOCUMENT_SHAPES[name]
    c = build()
    alpha = DC.resolve_alpha(alpha, K)
    lens = np.diff(c.doc_ptr)
    o = oracle_state(oracle, scheme, c, K, alpha, beta)
    n_dk = o.get_doc_topic_counts()
    if name.startswith("D="):
        assert c.num_docs == int(name[2:])
    elif name == "all-empty":
        assert c.num_tokens == 0 and c.num_docs > 4
    elif name == "empty-every-4":
        assert (lens == 0).sum() >= c.num_docs // 4 and c.num_docs % 4 == 1
    elif name == "one-token-documents":
        assert (lens == 1).all() and c.num_docs % 4 == 1
    elif name == "long-document":
        assert lens.max() == 40000 and lens.min() == 0
        assert n_dk.max() > 64 and (n_dk[int(np.argmax(lens))] > 0).sum() > 64      # counts and distinct topics beyond a wave
    elif name == "more-documents-than-types":
        assert c.num_docs > c.num_types and c.num_docs % 4 == 1
    if c.num_tokens:
        assert last_topic_is_hit(o, K)
    if scheme == "polyaurn" and c.num_tokens:
        assert DC.phi_zeros_under_tokens(o.get_phi(), o.get_z(), c.tokens) > 0
    check_reference(o, c, alpha, beta, "%s %s" % (name, scheme))


@pytest.mark.parametrize("scheme", ["ggs", "pcgs", "polyaurn"])
def test_grid_passes(oracle, scheme):
    build, K, alpha, beta = DC.GRID_PASSES
    c = build()
    cells, grid = c.num_types * K, DC.LL_GRID * DC.LL_BLOCK
    assert cells > 4 * grid and cells % grid and (cells % grid) % DC.LL_BLOCK      # a fifth pass that ends inside a block
    assert K % 2 == 1                                                              # Kp = K + 1: the Phi kernel skips a pad column
    o = oracle_state(oracle, scheme, c, K, alpha, beta)
    check_reference(o, c, alpha, beta, "grid passes %s" % scheme)


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_huge_count(oracle, scheme):
    c, z = DC.huge_count_corpus()
    K, alpha, beta = 4, 0.1, 0.01
    o = oracle_state(oracle, scheme, c, K, alpha, beta, z=z)
    assert o.get_type_topic_counts()[0, 2] == 2_000_000
    check_reference(o, c, alpha, beta, "2M in one cell %s" % scheme)


# ---- shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cuts", DC.SHARD_CUTS)
def test_shards_add_up(oracle, cuts):
    """Document sides of document shards (same z, same Phi, doc_base of their own) add up to the whole's, and every shard's
    topic side is the whole's.  As exact sums the shards' terms are the whole's terms but for D * lgS(alphaSum), one rounded
    product per handle: the sums differ by those roundings and the exact sums' own, at most shards + 2 of them."""
    c = DC.shard_corpus()
    assert cuts[-1] == c.num_docs and {len(x) for x in DC.SHARD_CUTS} == {3, 4} and any(lo == hi for x in DC.SHARD_CUTS for lo, hi in zip(x, x[1:]))
    K, alpha, beta = 33, DC.asymmetric_alpha(33), 0.01
    whole = oracle_state(oracle, "pcgs", c, K, alpha, beta)
    w_ll = [DC.exact(t) for t in whole.model_log_likelihood_terms()]
    w_lp = [DC.exact(t) for t in whole.log_posterior_terms()]
    ll_docs, lp_docs = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        sub, db, tb = c.shard(lo, hi)
        o = oracle.OracleSampler(K, c.num_types, alpha, beta, SEED)
        o.set_scheme("pcgs")
        o.set_corpus(sub.doc_ptr, sub.tokens, db, tb)
        o.set_z(whole.get_z()[tb:tb + sub.num_tokens], redraw_phi=False)
        o.set_counts(whole.get_type_topic_counts())
        o.set_phi(whole.get_phi())
        o.set_iteration(whole.iteration)
        o.draw_diagnostic_theta()
        assert (o.get_theta() == whole.get_theta()[lo:hi]).all()            # element (doc_base + d) * K of the stream
        s_ll = [DC.exact(t) for t in o.model_log_likelihood_terms()]
        s_lp = [DC.exact(t) for t in o.log_posterior_terms()]
        assert s_lp[1].value == w_lp[1].value and s_ll[1].value == w_ll[1].value
        ll_docs.append(s_ll[0].value)
        lp_docs.append(s_lp[0].value)
    n = len(cuts) - 1
    assert abs(math.fsum(lp_docs) - w_lp[0].value) <= (n + 2) * DC.U * w_lp[0].abs_sum
    assert abs(math.fsum(ll_docs) - w_ll[0].value) <= (n + 2) * DC.U * w_ll[0].abs_sum
