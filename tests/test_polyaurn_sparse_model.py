"""scheme=polyaurn_sparse on the CPU (no GPU): the restatement (tests/polyaurn_sparse_restatement.py) against the
mathematics it stands for -- the draw's histogram over a grid of uniforms against the dense polyaurn conditional, two
mutants the check must reject, the words' lists -- and the public surface: the flag, the header, the refusals, the
registry.  The chain's distance from the enumerated posterior is printed, not asserted: the scheme is approximate as
polyaurn is (DESIGN.md 6e records the figures)."""
import re

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import lda_posterior as LP
from tests import polyaurn_restatement as P
from tests import polyaurn_sparse_restatement as R

SEED = 777
G = 1 << 16


# ---- the draw against the dense conditional -------------------------------------------------------------------------
def mutant_draw(kind, st, phi_w, nzw_w, ps_w, a_w, tn, U, K):
    """token_draw with one slip.  "no_cnt": the word's list whenever it is non-empty, its scores without the count factor;
    "tie_to_word": nw <= nd takes the word's list."""
    nd, nw = len(st.list), len(nzw_w)
    use_word = nw > 0 if kind == "no_cnt" else nw <= nd
    cand = [int(k) for k in nzw_w] if use_word else st.list
    if not cand:
        return R.uniform_topic(U, K)
    cnt = np.asarray([1.0 if (kind == "no_cnt" and use_word) else st.cnt[k] for k in cand], np.float64)
    cum = np.cumsum(cnt * phi_w[np.asarray(cand, np.int64)])
    s = float(cum[-1])
    if U < tn / (tn + s):
        return R.alias_sample(ps_w, a_w, U + (s * U) / tn)
    return cand[R.list_search(cum, U * (tn + s) - tn)]


@pytest.fixture(scope="module")
def cases(oracle):
    """The middle token of each document of at least two tokens, the first twelve with candidates: (state with the token
    removed, word, kind, n), on the Phi of a polyaurn run's second sweep."""
    c = random_corpus(80, 50, 30, seed=4)
    K = 12
    alpha = 0.05 * (np.arange(K) + 1.0)
    z0 = oracle.jrandom_ints(5, K, c.num_tokens)
    m = P.Model(K, c.num_types, alpha, 0.01, SEED, c.doc_ptr, c.tokens, z0)
    m.init_phi()
    m.sweep(2)
    tables = R.alias_tables(m.phi, alpha)
    nw, lists = R.word_lists(m.phi)
    out = []
    for d in range(c.num_docs):
        b, e = int(c.doc_ptr[d]), int(c.doc_ptr[d + 1])
        if e - b < 2 or len(out) == 12:
            continue
        pos = (b + e) // 2
        w = int(c.tokens[pos])
        st = R.DocState(K, m.z[b:e])
        st.remove(int(m.z[pos]))
        det = {}
        R.token_draw(st, m.phi[:, w], lists[w], tables[0][w], tables[1][w], float(tables[2][w]), 0.5, K, det)
        if det["kind"] != R.UNIFORM:
            out.append((st, w, det["kind"], det["n"]))
    return dict(K=K, alpha=alpha, phi=m.phi, tables=tables, lists=lists, cases=out)


def frequencies(draw, fx, st, w):
    K, (ps, a, tn) = fx["K"], fx["tables"]
    hist = np.zeros(K, np.int64)
    for j in range(G):
        hist[draw(st, fx["phi"][:, w], fx["lists"][w], ps[w], a[w], float(tn[w]), (j + 0.5) / G, K)] += 1
    return hist / G


def dense_conditional(fx, st, w):
    want = (np.asarray(st.cnt, np.float64) + fx["alpha"]) * fx["phi"][:, w]
    return want / want.sum()


def test_histogram_over_a_grid_of_uniforms_is_the_dense_conditional(cases):
    """U = (j + 0.5) / 2^16: the draw is piecewise constant in U, a topic's preimage is at most K + 1 intervals (its alias
    cell, the halves of the cells that alias to it, its list entry) and each end costs one grid cell: (2K + 4) / 2^16."""
    K, bound = cases["K"], (2 * cases["K"] + 4) / G
    kinds = [kind for _, _, kind, _ in cases["cases"]]
    assert len(kinds) == 12 and R.WORD in kinds and R.DOC in kinds
    worst = 0.0
    for st, w, kind, n in cases["cases"]:
        dev = float(np.abs(frequencies(R.token_draw, cases, st, w) - dense_conditional(cases, st, w)).max())
        worst = max(worst, dev)
    print("polyaurn_sparse conditional: worst deviation %.3g against the bound %.3g; %d word-list and %d document-list cases"
          % (worst, bound, kinds.count(R.WORD), kinds.count(R.DOC)))
    assert worst <= bound


def test_a_walk_without_the_count_factor_is_rejected(cases):
    bound = (2 * cases["K"] + 4) / G
    worst = max(float(np.abs(frequencies(lambda *a: mutant_draw("no_cnt", *a), cases, st, w) - dense_conditional(cases, st, w)).max())
                for st, w, _, _ in cases["cases"])
    print("mutant without the count factor: worst deviation %.3g (bound %.3g)" % (worst, bound))
    assert worst > bound


def test_a_tie_goes_to_the_documents_list():
    """nw == nd: the document's list, in ITS order.  Both lists give the same distribution, so only the draw tells: with the
    document's list (2, 0) and the word's (0, 2) the walk's first entry is topic 2, and the mutant that takes nw <= nd
    lands on topic 0 there.  One entry fewer in the word's list and it is the word's turn."""
    K = 4
    st = R.DocState(K, [2, 0, 2])                                   # list (2, 0), counts 1, 0, 2, 0
    phi_w = np.array([0.25, 0.0, 0.5, 0.0])
    alpha = np.full(K, 0.1)
    ps, a, tn = R.alias_tables(phi_w[:, None], alpha)
    ps, a, tn = ps[0], a[0], float(tn[0])
    nw, lists = R.word_lists(phi_w[:, None])
    assert nw[0] == len(st.list) == 2 and list(lists[0]) == [0, 2] and st.list == [2, 0]
    s = 2 * 0.5 + 1 * 0.25
    U = (tn + 0.2) / (tn + s)                                       # ul = 0.2: inside the first entry of either list (1.0 and 0.25 wide)
    det = {}
    assert R.token_draw(st, phi_w, lists[0], ps, a, tn, U, K, det) == 2 and det["kind"] == R.DOC and not det["prior"]
    assert mutant_draw("tie_to_word", st, phi_w, lists[0], ps, a, tn, U, K) == 0
    phi_w[0] = 0.0                                                  # nw = 1 < nd = 2: the word's list, whose only entry is 2
    nw, lists = R.word_lists(phi_w[:, None])
    det = {}
    assert R.token_draw(st, phi_w, lists[0], ps, a, tn, 0.999, K, det) == 2 and det["kind"] == R.WORD and det["n"] == 1


def test_no_candidate_draws_floor_u_k():
    K = 5
    ps, a = np.ones(K), np.arange(K, dtype=np.int32)
    det = {}
    empty = R.DocState(K, [])                                       # a one-token document with its token removed
    assert R.token_draw(empty, np.full(K, 0.2), np.arange(K), ps, a, 1.0, 0.61, K, det) == 3 and det["kind"] == R.UNIFORM
    st = R.DocState(K, [1, 1, 4])                                   # an all-zero column: nw = 0 < nd
    assert R.token_draw(st, np.zeros(K), np.zeros(0, np.int64), ps, a, 0.0, 0.999999, K, det) == 4 and det == dict(kind=R.UNIFORM, n=0)
    assert R.uniform_topic(1.0 - 2.0 ** -53, K) == K - 1


# ---- the words' lists -----------------------------------------------------------------------------------------------
def test_word_lists_of_a_phi_with_zero_columns_zero_rows_and_single_entries():
    K, V = 6, 5
    phi = np.zeros((K, V))
    phi[:, 0] = [0.5, 0.0, 0.25, 0.0, 0.0, 1.0]                     # topic 3 and 1 are zero rows throughout
    phi[4, 2] = 1e-300                                              # one non-zero per column
    phi[0, 3] = 0.5
    phi[[0, 2, 4, 5], 4] = 0.1                                      # column 1 stays all zero
    nw, lists = R.word_lists(phi)
    assert list(nw) == [3, 0, 1, 1, 4]
    assert [list(l) for l in lists] == [[0, 2, 5], [], [4], [0], [0, 2, 4, 5]]
    pad = R.padded(lists, K)
    assert pad.shape == (V, K) and list(pad[0]) == [0, 2, 5, -1, -1, -1] and (pad[1] == -1).all()


# ---- the public surface ---------------------------------------------------------------------------------------------
def test_registry_flag_and_entry_points():
    from ldagroupedgibbssampler_amd import _lib, native, sampler
    cfg = sampler.SimpleLDAConfiguration(topics=4, seed=1)
    m = sampler.create_model(cfg, "polyaurn_sparse")
    assert type(m) is sampler.PolyaUrnSparseLDA and isinstance(m, sampler.LDAPartiallyCollapsedGibbsSampler)
    assert type(sampler.create_model(sampler.SimpleLDAConfiguration(topics=4, seed=1, scheme="polyaurn_sparse"))) is sampler.PolyaUrnSparseLDA
    assert sampler.PolyaUrnSparseLDA._scheme_flags == native.FLAG_POLYAURN_SPARSE == 128
    for name in ("getAliasTables", "getWordTopicLists", "getSparseStats"):
        assert callable(getattr(m, name))
    for name in ("ggs_get_word_topic_lists", "ggs_get_sparse_stats"):
        assert name in _lib.SIGNATURES
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"GGS_FLAG_POLYAURN_SPARSE\s*=\s*1\s*<<\s*7", header)
    assert re.search(r"\bint ggs_get_word_topic_lists\(", header) and re.search(r"\bint ggs_get_sparse_stats\(", header)
    assert "#define GGS_ABI_VERSION 6" in header and _lib.ABI_VERSION == 6   # a new bit, not a new ABI version
    assert native.Z_KERNEL_NAMES[8] == "polyaurn_sparse_wave_kernel (wave per document)"
    assert sampler.PolyaUrnSpaliasLDA._scheme_flags == native.FLAG_POLYAURN == 16   # polyaurn's bits stay as they are


def test_flag_combinations_are_refused():
    """GGS_FLAG_POLYAURN_SPARSE with GGS_FLAG_COLLAPSED, GGS_FLAG_POLYAURN, GGS_FLAG_SPALIAS or GGS_FLAG_LIGHTPCLDA is
    GGS_ERR_BAD_ARG, and so is a threshold outside 1..512: argument checks, answered before ggs_create asks for a device --
    so they can be seen here."""
    from ldagroupedgibbssampler_amd import native
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA,
                  native.FLAG_POLYAURN | native.FLAG_SPALIAS):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN_SPARSE | other)
        assert e.value.code == native.ERR_BAD_ARG
    for bad in (513, -1):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_POLYAURN_SPARSE, alias_poisson_threshold=bad)
        assert e.value.code == native.ERR_BAD_ARG


def test_new_kernels_use_no_scratch():
    import os
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
    for name in ("ggs::word_list_build_kernel", "ggs::polyaurn_sparse_wave_kernel"):
        assert name in rows, "kernel %s is not in the build" % name
        assert rows[name][3] == 0, "%s spills %d bytes per lane" % (name, rows[name][3])


# ---- distance from the enumerated posterior -------------------------------------------------------------------------
N_SAMPLES, THIN = 4000, 4                                           # polyaurn's recipe (tests/lda_posterior.py), kept local


def test_restatement_chain_runs_and_stays_in_range(oracle):
    """Fixture A, seed 1, n = 4000, thin 4, default Poisson threshold.  Approximate as polyaurn is (the same Phi, the same
    uniform draw for the one-token document), so nothing is asserted about the distribution; the figures are printed.
    Recorded: chi2 = 2463.4 on 147 cells, total variation 0.3901 (polyaurn: 2539 and 0.39; the exact chains 125 ... 172 and
    0.11 ... 0.12)."""
    A = LP.FIXTURE_A
    post = LP.enumerate_posterior(A.doc_ptr, A.tokens, A.K, A.V, A.alpha, A.beta)
    z0 = oracle.jrandom_ints(1, A.K, len(A.tokens))
    m = R.Model(A.K, A.V, np.asarray(A.alpha), A.beta, 1, A.doc_ptr, A.tokens, z0)
    m.init_phi()
    idx = LP.run_chain(m.sweep, lambda: m.z, A.K, N_SAMPLES, THIN, LP.BURN_IN, max_topic=A.K - 1)
    v = LP.verdict(idx, post.p)
    print("polyaurn_sparse restatement: chi2 = %.1f on %d cells, p = %.3g, TV = %.4f" % (v.chi2, v.cells, v.pvalue, v.tv))
    assert idx.min() >= 0 and idx.max() < post.p.size and v.n == N_SAMPLES
    assert int(m.stats[:3].sum()) == (LP.BURN_IN + N_SAMPLES * THIN) * len(A.tokens) and m.stats[2] > 0
