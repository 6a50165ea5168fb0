"""scheme=spalias on the CPU (no GPU): the restatement (tests/spalias_restatement.py) against the mathematics it stands
for -- the tables' implied probabilities, the draw's histogram against the pcgs conditional, the list discipline, the
edge rules marked "ours" -- the knife-edge builder (tests/spalias_knife_edge.py) against the restatement, and the public
surface: the registry, the flag, the ABI version, the resource rows of the new kernels."""
import os
import re

import numpy as np
import pytest

from tests import spalias_knife_edge as KE
from tests import spalias_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the tables ---------------------------------------------------------------------------------------------------
def _weights(K, kind, rng):
    pi = rng.gamma(0.3, 1.0, K) + 1e-12
    if kind == "half_zero":
        pi[rng.permutation(K)[:K // 2]] = 0.0
    return pi


@pytest.mark.parametrize("kind", ["dirichlet", "half_zero"])
@pytest.mark.parametrize("K", [3, 8, 100, 1024])
def test_implied_probabilities_equal_the_normalised_weights(K, kind):
    """ps[i] / K to i and (1 - ps[i]) / K to a[i] add up to pi / typeNorm within 4 K 2^-53: at most K rounded adds of terms
    below 1 in a column of bs, plus the multiply-add of ps."""
    rng = np.random.default_rng(K)
    worst = 0.0
    for _ in range(20):
        pi = _weights(K, kind, rng)
        ps, a, tn = R.alias_table(pi)
        assert ((ps >= 0) | (ps > -4 * K * 2.0 ** -53)).all() and (ps <= 1.0).all()
        q = R.implied_probabilities(ps, a)
        worst = max(worst, float(np.abs(q - pi / tn).max()))
    print("K=%d %s: largest deviation %.3g (bound %.3g)" % (K, kind, worst, 4 * K * 2.0 ** -53))
    assert worst <= 4 * K * 2.0 ** -53


# the zero-probability cases of the reference's WalkerAliasTableTest with their inputs (the zero first, in the middle, last:
# 0/15, 5/15, 10/15 in its three orders), then some more
@pytest.mark.parametrize("pi", [[0.0 / 15.0, 5.0 / 15.0, 10.0 / 15.0], [5.0 / 15.0, 0.0 / 15.0, 10.0 / 15.0], [10.0 / 15.0, 5.0 / 15.0, 0.0 / 15.0],
                                [0.0, 1.0], [1.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0], [0.2, 0.0, 0.3, 0.0, 0.5],
                                [0.0, 0.0, 0.0, 1.0], [0.1, 0.2, 0.0, 0.7, 0.0, 0.0]])
def test_zero_weights_are_never_drawn(pi):
    pi = np.array(pi)
    ps, a, tn = R.alias_table(pi)
    G = 1 << 16
    hist = np.zeros(pi.size, np.int64)
    for g in range(G):
        hist[R.alias_sample(ps, a, (g + 0.5) / G)] += 1
    assert (hist[pi == 0.0] == 0).all(), hist
    assert np.abs(hist / G - pi / pi.sum()).max() <= (2 * pi.size + 2) / G


def test_stale_entries_read_one_and_an_underflowed_column_is_the_identity():
    ps, a, tn = R.alias_table(np.array([0.25, 0.25, 0.25, 0.25]))   # nothing to pair
    assert (ps == 1.0).all() and (a == np.arange(4)).all() and tn == 1.0
    ps, a, tn = R.alias_table(np.zeros(5))
    assert tn == 0.0 and (ps == 1.0).all() and (a == np.arange(5)).all()


# ---- the draw against the pcgs conditional ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["empty", "short", "full"])
def test_histogram_over_a_grid_of_uniforms_is_the_pcgs_conditional(case):
    """K = 8, G = 2^18 midpoint uniforms: the draw is piecewise constant in U on at most 2K + nnz + 2 intervals (2K alias
    cells and halves, nnz list entries, the branch point and the ends), so the histogram is within (2K + nnz + 2) / G of
    (n + alpha) * phi / sum."""
    K, G = 8, 1 << 18
    rng = np.random.default_rng({"empty": 1, "short": 2, "full": 3}[case])
    alpha = rng.uniform(0.05, 0.5, K)
    phi_w = rng.gamma(0.5, 1.0, K)
    topics = {"empty": [], "short": [5, 1, 5, 6], "full": list(rng.permutation(K)) * 2 + [3, 3, 0]}[case]
    st = R.DocState(K, topics)
    nnz = len(st.list)
    ps, a, tn = R.alias_table(phi_w * alpha)
    hist = np.zeros(K, np.int64)
    for g in range(G):
        hist[R.token_draw(st, 0, phi_w, ps, a, tn, (g + 0.5) / G)] += 1
    want = (np.array(st.cnt, np.float64) + alpha) * phi_w
    want /= want.sum()
    dev = float(np.abs(hist / G - want).max())
    print("%s list (nnz %d): largest deviation %.3g, bound %.3g" % (case, nnz, dev, (2 * K + nnz + 2) / G))
    assert dev <= (2 * K + nnz + 2) / G


# ---- the list and the edge rules ----------------------------------------------------------------------------------
def test_list_discipline_on_a_hand_case():
    st = R.DocState(6, [4, 2, 4, 0, 5])
    assert st.list == [4, 2, 0, 5] and st.cnt == [1, 0, 1, 0, 2, 1]
    st.remove(2)                                                    # count 0: the last entry takes its slot
    assert st.list == [4, 5, 0] and st.pos == {4: 0, 5: 1, 0: 2}
    st.remove(4)                                                    # count 1 left: nothing moves
    assert st.list == [4, 5, 0]
    st.add(3)                                                       # count becomes 1: appended
    assert st.list == [4, 5, 0, 3]
    st.remove(3)                                                    # the last entry itself
    assert st.list == [4, 5, 0] and 3 not in st.pos
    st.add(2)
    st.remove(4)
    assert st.list == [2, 5, 0] and st.pos == {2: 0, 5: 1, 0: 2}


def test_one_token_document_draws_from_the_alias_table_with_x_equal_u(oracle):
    K = 5
    phi = np.random.default_rng(0).dirichlet(np.ones(7), K)         # [K][V = 7]
    tables = R.alias_tables(phi, 0.3)
    z = np.array([2], np.int64)
    R.z_step([0, 1], [4], z, phi, tables, 11, 1)
    U = float(oracle.uniforms(11, 1, R.PURPOSE_Z, 0, 1)[0])
    assert z[0] == R.alias_sample(tables[0][4], tables[1][4], U)


def test_ul_beyond_sum_takes_the_last_entry_and_an_empty_list_keeps_the_old_topic():
    K = 4
    st = R.DocState(K, [1, 3, 3])
    phi_w = np.array([0.0, 0.5, 0.0, 0.25])
    ps, a, _ = R.alias_table(np.full(K, 0.25))
    # typeNorm 0 with a list: the likelihood branch, ul = U * sum; U within an ulp of 1 is as far as ul goes
    det = {}
    assert R.token_draw(st, 1, phi_w, ps, a, 0.0, 1.0 - 2.0 ** -53, det) == 3 and not det["prior"]
    # ul above every cum entry (an ulp above sum by rounding): the last entry; ties and equal entries: the smallest index
    cum = np.array([0.5, 1.0, 1.0, 1.0])
    assert R.list_search(cum, np.nextafter(1.0, 2.0)) == 3
    assert R.list_search(cum, 1.0) == 1 and R.list_search(cum, 0.5) == 0 and R.list_search(cum, np.nextafter(0.5, 1.0)) == 1
    # typeNorm 0 and an empty list: 0 / 0 fails the comparison, the token keeps its old topic
    empty = R.DocState(K, [])
    det = {}
    assert R.token_draw(empty, 2, np.zeros(K), ps, a, 0.0, 0.3, det) == 2 and not det["prior"]
    # typeNorm 0, a list, all scores 0: ul = 0 <= cum[0]
    assert R.token_draw(st, 1, np.zeros(K), ps, a, 0.0, 0.3) == 1


def test_alias_draw_that_reaches_k_raises():
    ps, a, _ = R.alias_table(np.array([0.5, 0.5]))
    with pytest.raises(R.InvalidTopic):
        R.alias_sample(ps, a, 1.0)


# ---- the knife-edge builder ---------------------------------------------------------------------------------------
def test_knife_edge_builder_reaches_every_category_and_the_restatement_draws_it(oracle):
    ke = KE.KnifeEdge()
    counts, expect, pairs = ke.survey()
    print(sorted(counts.items()), "branch pairs", pairs)
    for kind in KE.POSITIONS:
        for cat in ("tie", "below", "above"):
            assert counts.get((kind, cat), 0) >= KE.MIN_PER_CATEGORY, (kind, cat, counts)
    assert pairs >= KE.MIN_PER_CATEGORY
    by_j = {}
    for j, tok, want, kind, cat in expect:
        by_j.setdefault(j, []).append((tok, want, kind, cat))
    checked = 0
    for j in sorted(by_j):
        z = ke.restatement_z(j)
        if z is None:
            continue
        prefix = np.ones(z.size, bool)
        prefix[[row.target for row in ke.rows]] = False
        assert (z[prefix] == ke.z0[prefix]).all(), "a prefix token moved: the rows are not in the state they were built for"
        for tok, want, kind, cat in by_j[j]:
            assert z[tok] == want, (j, tok, kind, cat)
            checked += 1
    assert checked > 1000


# ---- the public surface -------------------------------------------------------------------------------------------
def test_registry_flag_and_abi_version():
    from ldagroupedgibbssampler_amd import _lib, native, sampler
    m = sampler.create_model(sampler.SimpleLDAConfiguration(topics=4, seed=1, scheme="spalias"))
    assert type(m) is sampler.SpaliasUncollapsedParallelLDA
    assert isinstance(m, sampler.LDAPartiallyCollapsedGibbsSampler)
    assert sampler.SpaliasUncollapsedParallelLDA._scheme_flags == native.FLAG_SPALIAS == 32
    assert _lib.ABI_VERSION == 6
    for name in ("ggs_debug_alias", "ggs_get_alias_tables"):
        assert name in _lib.SIGNATURES
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"GGS_FLAG_SPALIAS\s*=\s*1\s*<<\s*5", header) and "#define GGS_ABI_VERSION 6" in header
    for name in ("ggs_debug_alias", "ggs_get_alias_tables"):
        assert re.search(r"\bint %s\(" % name, header)
    with pytest.raises(ValueError, match="spalias"):
        sampler.create_model(sampler.SimpleLDAConfiguration(topics=4, seed=1), "nzvsspalias")


def test_flag_combinations_are_refused():
    """GGS_FLAG_SPALIAS with GGS_FLAG_COLLAPSED or GGS_FLAG_POLYAURN is GGS_ERR_BAD_ARG: an argument check, answered before
    ggs_create asks for a device -- so it can be seen here."""
    from ldagroupedgibbssampler_amd import native
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_COLLAPSED | native.FLAG_POLYAURN):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_SPALIAS | other)
        assert e.value.code == native.ERR_BAD_ARG


def test_new_kernels_use_no_scratch():
    path = os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc", "ggs_resource_summary.txt")
    if not os.path.exists(path):
        from ldagroupedgibbssampler_amd import _lib
        _lib.build()
    rows = {}
    for line in open(path):
        if line.startswith("#"):
            continue
        f = line.split()
        rows[" ".join(f[:-6])] = [int(x) for x in f[-6:]]
    for name in ("ggs::alias_build_kernel", "ggs::spalias_wave_kernel"):
        assert name in rows, "kernel %s is not in the build" % name
        vgprs, agprs, sgprs, scratch = rows[name][:4]
        assert scratch == 0, "%s spills %d bytes per lane" % (name, scratch)
