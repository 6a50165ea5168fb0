"""scheme=nzvsspalias on the CPU (no GPU): the restatement (tests/nzvs_restatement.py) against the mathematics it stands for --
fdlibm's exp against the platform's, the indicator probability against the same expression over scipy's gammaln, the numpy
model of the chain kernel's rounds against the sequential chain, the whole draw's corner cases, the z step's histogram over
a grid of uniforms against the dense conditional -- and the public surface: the flag, the header, the refusals, the registry."""
import os
import re

import numpy as np
import pytest
from scipy.special import gammaln

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import nzvs_restatement as R
from tests import spalias_restatement as SP

SEED = 777
G = 1 << 16
BETA = 0.01


# ---- exp ------------------------------------------------------------------------------------------------------------
def test_exp_is_within_one_ulp_of_the_platforms_on_100000_points():
    x = R.exp_grid()[:100000]
    with np.errstate(over="ignore", under="ignore"):
        ref = np.exp(x)
    mine = np.array([R.strict_exp(v) for v in x])
    finite = np.isfinite(ref) & (ref > 0)
    ulps = np.abs(mine[finite] - ref[finite]) / np.spacing(ref[finite])
    print("strict_exp against numpy.exp on %d points of [-745, 710]: worst %.2f ulp" % (x.size, ulps.max()))
    assert ulps.max() <= 1.0
    assert np.array_equal(mine[~finite], ref[~finite])              # overflowed to inf / underflowed to 0 alike


def test_exp_special_values_and_thresholds():
    inf = float("inf")
    assert R.strict_exp(0.0) == 1.0 and R.strict_exp(-0.0) == 1.0
    assert R.strict_exp(inf) == inf and R.strict_exp(-inf) == 0.0 and np.isnan(R.strict_exp(float("nan")))
    o, u = 7.09782712893383973096e+02, -7.45133219101941108420e+02
    assert np.isfinite(R.strict_exp(o)) and R.strict_exp(np.nextafter(o, inf)) == inf
    assert R.strict_exp(u) == 5e-324 and R.strict_exp(np.nextafter(u, -inf)) == 0.0
    assert R.strict_exp(1e-10) == 1.0 + 1e-10                       # |x| < 2^-28: 1 + x


# ---- p(s) -----------------------------------------------------------------------------------------------------------
# The largest |exponent - the same expression over gammaln| on the grid below, measured with this restatement: four lgS errors
# against gammaln (the Stirling series' truncation after the shift to z >= 2, and at n_k = 2e9 the cancellation of terms of 4e10).
EXPONENT_MEASURED = 5.735842807830238e-06


def test_indicator_exponent_against_gammaln(oracle):
    worst = 0.0
    for s in (1, 2, 10, 10 ** 3, 10 ** 6):
        for n_k in (1, 400, 2 * 10 ** 5, 2 * 10 ** 9):
            for beta in (0.01, 0.1):
                a = s * beta
                ref = float(gammaln(a + beta) + gammaln(a + n_k) - gammaln(a + beta + n_k) - gammaln(a))
                e = float(R.indicator_exponent(np.array([s]), n_k, beta)[0])
                worst = max(worst, abs(e - ref))
                p = float(R.indicator_probability(np.array([s]), n_k, beta, 0.5)[0])
                assert abs(p - np.exp(ref) / (1 + np.exp(ref))) <= 2 * EXPONENT_MEASURED   # |dp/de| <= 1/4
    print("indicator exponent against gammaln: worst absolute difference %.3g (asserted: twice %.3g)" % (worst, EXPONENT_MEASURED))
    assert worst <= 2 * EXPONENT_MEASURED


def test_indicator_probability_at_s_zero(oracle):
    for n_k in (1, 400, 2 * 10 ** 9):
        p = R.indicator_probability(np.array([0]), n_k, BETA, 0.5)[0]
        assert p == 0.0 and not np.signbit(p)                       # lgS(0) = +inf: r = 0
    p = R.indicator_probability(np.array([0]), 0, BETA, 0.5)[0]
    assert np.isnan(p) and not (0.3 > p) and not R.out_of_range(p)  # U > NaN is false (drawn); NaN passes the range check
    assert R.out_of_range(1.5) and R.out_of_range(-0.1) and not R.out_of_range(1.0) and not R.out_of_range(0.0)


# ---- the rounds -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain_rows(oracle):
    """every row with its sequential result, computed once"""
    return [(name, c, p, u, pi, R.sequential_chain(c, p, u, BETA, pi)) for name, c, p, u, pi in R.chain_cases(BETA)]


def test_rounds_equal_the_sequential_chain(chain_rows):
    most = 0
    for name, c, p, u, pi, (drawn, s_end, bad) in chain_rows:
        d, s, rounds = R.rounds_chain(c, p, u, BETA, pi)
        assert np.array_equal(d, drawn) and s == s_end, name
        assert rounds <= int((c == 0).sum()) + 1, name
        assert not bad and drawn[c != 0].all(), name
        most = max(most, rounds)
    print("%d rows: at most %d rounds" % (len(chain_rows), most))


def test_edge_rows_stand_on_the_edge(chain_rows):
    seen = 0
    for name, c, p, u, pi, (drawn, s_end, bad) in chain_rows:
        m = re.match(r"U (on|one ulp above) p\(s\) at cell (\d+)", name)
        if not m:
            continue
        cell = int(m.group(2))
        s = int(R.states_before(c, p, u, BETA, pi)[cell])
        prob = R.Probabilities(int(c.sum()), BETA, pi)(s)
        assert 0.0 < prob < 1.0
        assert u[cell] == (prob if m.group(1) == "on" else np.nextafter(prob, 2.0))
        assert drawn[cell] == (m.group(1) == "on"), name            # U == p is drawn, one ulp above is not
        seen += 1
    assert seen == 10


def test_the_chain_returns_to_zero_in_the_middle(chain_rows):
    name, c, p, u, pi, (drawn, s_end, bad) = [r for r in chain_rows if r[0] == "s returns to 0 V=65"][0]
    before = R.states_before(c, p, u, BETA, pi)
    assert before[0] == 5 and (before[5:] == 0).all() and before[64] == 0
    assert not drawn[64] and s_end == 1                             # p = 0 there: U > 0 is undrawn


def test_without_the_confirming_round_a_row_comes_out_wrong(chain_rows):
    wrong = [name for name, c, p, u, pi, (drawn, s_end, bad) in chain_rows
             if not (lambda r: np.array_equal(r[0], drawn) and r[1] == s_end)(R.rounds_chain(c, p, u, BETA, pi, confirm=False))]
    print("without the confirming round: wrong on %s" % wrong)
    assert wrong


# ---- the whole draw -------------------------------------------------------------------------------------------------
def test_a_row_with_sum_zero_becomes_zeros(oracle):
    K, V = 2, 40
    counts = np.zeros((K, V), np.int32)                             # n_k == 0: p = pi wherever s > 0
    prev = np.full((K, V), 0.5)
    prev[:, 0] = 0.0                                                # s0 = 1
    phi, drawn, s_end = R.vs_phi(counts, prev, BETA, 0.01, SEED, 3, U=np.full((K, V), 0.9))
    assert not drawn.any() and (s_end == V).all()
    assert (phi == 0.0).all() and not np.signbit(phi).any()
    nw, lists = R.drawn_lists(drawn)
    assert (nw == 0).all()


def test_an_underflowed_gamma_stays_listed_and_counts_as_a_zero(oracle):
    """Gamma(0.01) underflows to exactly 0.0 about once in 2000 draws.  All cells without tokens, all kept (U = 0): the cells that
    hold 0.0 are drawn cells -- in their words' lists -- and the next draw's s0 counts them."""
    K, V = 3, 4000
    counts = np.zeros((K, V), np.int32)
    counts[:, 0] = 9
    phi, drawn, s_end = R.vs_phi(counts, np.full((K, V), 0.5), BETA, 0.5, SEED, 1, U=np.zeros((K, V)))
    assert drawn.all()
    zeros = phi == 0.0
    print("%d of %d Gamma(%g) draws underflowed to 0.0" % (zeros.sum(), K * V, BETA))
    assert zeros.any()
    nw, lists = R.drawn_lists(drawn)
    assert (nw == K).all()                                          # the list is the drawn set, not phi != 0.0
    for k in range(K):
        assert R.states_before(counts[k], phi[k], np.zeros(V), BETA, 0.5)[0] == zeros[k].sum()
    assert np.allclose(phi.sum(axis=1), 1.0)


def test_s_ignores_cells_with_a_count(oracle):
    V = 50
    counts = np.arange(1, V + 1, dtype=np.int32)                    # no cell without tokens
    prev = np.zeros(V)                                              # every old cell 0.0: s0 = V
    drawn, s_end, bad = R.sequential_chain(counts, prev, np.full(V, 0.999), BETA, 0.5)
    assert drawn.all() and s_end == V                               # drawn, and s does not move (the reference)
    counts[7] = 0
    drawn, s_end, bad = R.sequential_chain(counts, prev, np.zeros(V), BETA, 0.5)
    assert drawn.all() and s_end == V - 1                           # the one cell without tokens, kept: one zero fewer


# ---- the z step against the dense conditional -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(oracle):
    """Twelve tokens of a restatement run, four of each kind: the alias-only ones from the first z step (every list is empty
    before the first Phi draw), the others from the third."""
    c = random_corpus(80, 50, 30, seed=4)
    K = 12
    alpha = 0.05 * (np.arange(K) + 1.0)
    z0 = oracle.jrandom_ints(5, K, c.num_tokens)
    m = R.Model(K, c.num_types, alpha, BETA, SEED, c.doc_ptr, c.tokens, z0)
    m.init_phi()
    out = []

    def collect(kinds):
        trace = []
        z = m.z.copy()
        R.z_step(m.doc_ptr, m.tokens, z, m.phi, m.tables, m.lists, SEED, m.iteration + 1, trace=trace)
        for kind in kinds:
            picked = [t for t in trace if t["kind"] == kind and (kind == R.ALIAS or len(t["list"]) >= 2)][:4]
            assert len(picked) == 4
            for t in picked:
                st = SP.DocState(K, [])
                st.cnt, st.list, st.pos = list(t["cnt"]), list(t["list"]), {k: i for i, k in enumerate(t["list"])}
                out.append(dict(st=st, w=t["w"], kind=kind, phi=m.phi, tables=m.tables, lists=m.lists))
    collect([R.ALIAS])
    assert m.stats.sum() == 0
    m.sweep(2)
    assert m.stats[R.ALIAS] >= c.num_tokens                         # the whole first sweep
    collect([R.WORD, R.DOC])
    return dict(K=K, alpha=alpha, cases=out)


def test_histogram_over_a_grid_of_uniforms_is_the_dense_conditional(cases):
    """U = (j + 0.5) / 2^16 and the bound (2K + 4) / 2^16, as tests/test_polyaurn_sparse_model.py derives it.  A token without a
    candidate goes against alpha * phi / typeNorm."""
    K, alpha, bound = cases["K"], cases["alpha"], (2 * cases["K"] + 4) / G
    kinds = [cs["kind"] for cs in cases["cases"]]
    assert kinds.count(R.WORD) == kinds.count(R.DOC) == kinds.count(R.ALIAS) == 4
    worst = 0.0
    for cs in cases["cases"]:
        st, w, (ps, a, tn) = cs["st"], cs["w"], cs["tables"]
        hist = np.zeros(K, np.int64)
        for j in range(G):
            det = {}
            hist[R.token_draw(st, cs["phi"][:, w], cs["lists"][w], ps[w], a[w], float(tn[w]), (j + 0.5) / G, K, det)] += 1
            assert det["kind"] == cs["kind"]
        if cs["kind"] == R.ALIAS:
            want = alpha * cs["phi"][:, w] / float(tn[w])
        else:
            want = (np.asarray(st.cnt, np.float64) + alpha) * cs["phi"][:, w]
            want = want / want.sum()
        worst = max(worst, float(np.abs(hist / G - want).max()))
    print("nzvsspalias conditional: worst deviation %.3g against the bound %.3g" % (worst, bound))
    assert worst <= bound


def test_no_candidate_draws_from_the_alias_table():
    K = 5
    ps, a = np.array([0.5, 1.0, 1.0, 1.0, 1.0]), np.array([3, 1, 2, 3, 4], np.int32)
    empty = SP.DocState(K, [])
    det = {}
    assert R.token_draw(empty, np.full(K, 0.2), np.arange(K), ps, a, 1.0, 0.05, K, det) == 0 and det == dict(kind=R.ALIAS, n=0)
    assert R.token_draw(empty, np.full(K, 0.2), np.arange(K), ps, a, 1.0, 0.15, K, det) == 3        # past ps[0]: the alias
    st = SP.DocState(K, [1, 1, 4])                                  # an empty word list: nw = 0 < nd
    assert R.token_draw(st, np.zeros(K), np.zeros(0, np.int64), ps, a, 0.0, 0.61, K, det) == 3 and det["kind"] == R.ALIAS
    with pytest.raises(SP.InvalidTopic):
        SP.alias_sample(ps, a, 1.0)                                 # i == K


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_registry_flag_and_entry_points():
    from ldagroupedgibbssampler_amd import _lib, native, sampler
    cfg = sampler.SimpleLDAConfiguration(topics=4, seed=1, variable_selection_prior=0.25)
    m = sampler.NZVSSpaliasUncollapsedParallelLDA(cfg)          # the class itself: create_model has no case for it (tests/test_spalias_model.py pins its refusal)
    assert isinstance(m, sampler.LDAPartiallyCollapsedGibbsSampler) and m.config.variable_selection_prior == 0.25
    assert sampler.SimpleLDAConfiguration().variable_selection_prior == 0.5
    assert sampler.NZVSSpaliasUncollapsedParallelLDA._scheme_flags == native.FLAG_NZVSSPALIAS == 512
    for name in ("getAliasTables", "getWordTopicLists", "getSparseStats"):
        assert callable(getattr(m, name))
    for name in ("set_variable_selection_prior", "vs_stats"):
        assert callable(getattr(native.GGSHandle, name))
    header = open(_lib.HEADER_PATH).read()
    for name in ("ggs_set_variable_selection_prior", "ggs_get_vs_stats", "ggs_debug_vs_indicators"):
        assert name in _lib.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    assert re.search(r"GGS_FLAG_NZVSSPALIAS\s*=\s*1\s*<<\s*9", header) and re.search(r"GGS_PURPOSE_VS\s*=\s*6", header)
    assert "#define GGS_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6   # a new bit, not a new ABI version
    assert native.Z_KERNEL_NAMES[10] == "nzvs_wave_kernel (wave per document)"
    assert sampler.PolyaUrnSparseLDA._scheme_flags == native.FLAG_POLYAURN_SPARSE == 128   # the others' bits stay as they are


def test_flag_combinations_are_refused():
    """argument checks, answered before ggs_create asks for a device -- so they can be seen here"""
    from ldagroupedgibbssampler_amd import native
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA, native.FLAG_POLYAURN_SPARSE,
                  native.FLAG_LIGHTCOLLAPSED):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_NZVSSPALIAS | other)
        assert e.value.code == native.ERR_BAD_ARG


def test_new_kernels_use_no_scratch():
    from ldagroupedgibbssampler_amd import _lib
    path = os.path.join(_lib.CSRC, "ggs_resource_summary.txt")
    if not os.path.exists(path):
        _lib.build()
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        f = line.split()
        rows[" ".join(f[:-6])] = [int(x) for x in f[-6:]]
    for name in ("ggs::vs_bits_kernel", "ggs::vs_chain_kernel<false>", "ggs::vs_chain_kernel<true>", "ggs::vs_mask_kernel", "ggs::word_list_mask_kernel",
                 "ggs::phi_gamma_vs_kernel", "ggs::nzvs_wave_kernel"):
        assert name in rows, "kernel %s is not in the build" % name
        assert rows[name][3] == 0, "%s spills %d bytes per lane" % (name, rows[name][3])
