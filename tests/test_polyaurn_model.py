"""scheme=polyaurn on the CPU: the restatement's Poisson tables and draws against scipy, the two z rules on hand-built
cases, the host mirror's wiring, and the resource summary of the build (no GPU needed)."""
import os

import numpy as np
import pytest
from scipy import stats

from tests import polyaurn_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20251016


def truncated_cdf(lam, L):
    p = stats.poisson.pmf(np.arange(2 * L), lam)
    return np.cumsum(p) / p.sum()


@pytest.mark.parametrize("L", [1, 7, 100, 512])
@pytest.mark.parametrize("beta", [0.01, 0.5, 7.0])
def test_table_rows_are_the_truncated_renormalised_pmf(oracle, L, beta):
    T = R.poisson_table(beta, L)
    assert T.shape == (L, 2 * L)
    assert (T[:, -1] == 1.0).all()
    assert (np.diff(T, axis=1) >= 0).all()
    for c in sorted({0, min(1, L - 1), L // 2, L - 1}):
        ref = truncated_cdf(beta + c, L)
        np.testing.assert_allclose(T[c], ref, rtol=1e-12, atol=0)


@pytest.mark.parametrize("L", [7, 100])
def test_draws_below_the_threshold_fit_the_truncated_pmf(oracle, L):
    beta, n = 0.5, 40000
    for i, c in enumerate(sorted({0, 1, 2, 7, 50, L - 1} - ({50} if L < 51 else set()))):
        if c >= L:
            continue
        X = R.poisson_draw(np.full(n, c), beta, L, SEED, 3, R.PURPOSE_PHI, i * n)
        assert X.min() >= 0 and X.max() < 2 * L
        p = stats.poisson.pmf(np.arange(2 * L), beta + c)
        p = p / p.sum()
        obs = np.bincount(X, minlength=2 * L).astype(np.float64)
        exp = p * n
        # merge the tails so that every bin expects at least 5
        order = np.argsort(-exp)
        keep = exp >= 5
        if (~keep).any():
            obs = np.append(obs[keep], obs[~keep].sum())
            exp = np.append(exp[keep], exp[~keep].sum())
        else:
            obs, exp = obs[order], exp[order]
        if exp.size < 2:
            assert obs[0] == n
            continue
        chi = stats.chisquare(obs, exp * (obs.sum() / exp.sum()))
        assert chi.pvalue > 1e-4, (c, chi)


@pytest.mark.parametrize("c", [100, 1000, 100000])
def test_normal_branch_mean_and_variance(oracle, c):
    beta, L, n = 0.01, 100, 200000
    X = R.poisson_draw(np.full(n, c), beta, L, SEED, 5, R.PURPOSE_PHI, 10 ** 9).astype(np.float64)
    lam = beta + c
    se_mean = np.sqrt(lam / n)
    se_var = np.sqrt((lam + 2 * lam * lam) / n)
    assert abs(X.mean() - lam) < 4 * se_mean, (X.mean(), lam)
    assert abs(X.var() - lam) < 4 * se_var, (X.var(), lam)


def test_normal_branch_is_the_rounded_gaussian(oracle):
    """X = max(0, floor(sqrt(l) * g + l + 0.5)) with the element's Gaussian; the clamp holds X at 0."""
    counts = np.array([100, 101, 5000, 100], np.int64)
    beta = 0.25
    g = np.array([0.0, -1.5, 2.25, -11.0])
    u = np.zeros(4)
    X = R.poisson_from_streams(counts, beta, 100, u, g)
    lam = beta + counts
    assert list(X) == [int(np.floor(np.sqrt(lam[i]) * g[i] + lam[i] + 0.5)) if i < 3 else 0 for i in range(4)]
    assert X[3] == 0


def test_search_is_the_smallest_index_above_u(oracle):
    T = R.poisson_table(0.01, 3)
    c = np.zeros(4, np.int64)
    u = np.array([0.0, np.nextafter(T[0, 0], 0), T[0, 0], T[0, 1]])
    X = R.poisson_from_streams(c, 0.01, 3, u, np.zeros(4), T)
    assert list(X) == [0, 0, 1, 2]                               # u == T[j] moves on to j + 1


def test_phi_rows_normalise_by_the_integer_total_and_zero_rows_stay_zero(oracle):
    rng = np.random.default_rng(1)
    K, V = 6, 50
    n = rng.integers(0, 4, (K, V))
    n[2] = 0                                                      # a topic without tokens
    phi, X, tot = R.phi_draw(n, 1e-9, 100, SEED, 1, False)
    assert tot[2] == 0 and (phi[2] == 0).all() and not np.isnan(phi).any()
    for k in range(K):
        if tot[k]:
            assert np.array_equal(phi[k], X[k].astype(np.float64) / float(tot[k]))
    assert (phi == 0).any()                                       # exact zeros, no Double.MIN_VALUE clamp


def hand_case(phi, alpha, docs, z0):
    doc_ptr = np.cumsum([0] + [len(d) for d in docs])
    tokens = np.concatenate([np.asarray(d, np.int64) for d in docs])
    z = np.array(z0, np.int64)
    return doc_ptr, tokens, z


def test_one_token_documents_draw_floor_u_k(oracle):
    K = 7
    phi = np.full((K, 3), 1.0 / 3)
    doc_ptr, tokens, z = hand_case(phi, 0.1, [[0], [1, 2], [2]], [3, 1, 1, 6])
    it = 4
    n = R.z_step(doc_ptr, tokens, z, phi, 0.1, SEED, it)
    U = oracle.uniforms(SEED, it, R.PURPOSE_Z, 0, 4)
    assert z[0] == int(U[0] * K) and z[3] == int(U[3] * K)
    assert n >= 2


def test_zero_column_draws_floor_u_k(oracle):
    K = 5
    phi = np.zeros((K, 2))
    phi[:, 0] = [0.1, 0.2, 0.3, 0.2, 0.2]                         # word 1 has an all-zero column
    doc_ptr, tokens, z = hand_case(phi, 0.5, [[0, 1, 0, 1]], [0, 1, 2, 3])
    it = 2
    n = R.z_step(doc_ptr, tokens, z, phi, 0.5, SEED, it)
    U = oracle.uniforms(SEED, it, R.PURPOSE_Z, 0, 4)
    assert z[1] == int(U[1] * K) and z[3] == int(U[3] * K)
    assert n == 2


def test_other_tokens_follow_the_pcgs_walk(oracle):
    """Where neither rule applies the restated step is the oracle's pcgs step (oracle/ggs_oracle.c:732-781), bit for bit."""
    from ldagroupedgibbssampler_amd.corpus import random_corpus
    c = random_corpus(60, 30, 12, seed=3)
    keep = np.diff(c.doc_ptr) != 1                                # no one-token documents
    lens = np.diff(c.doc_ptr)[keep]
    doc_ptr = np.concatenate(([0], np.cumsum(lens)))
    tokens = np.concatenate([c.tokens[c.doc_ptr[d]:c.doc_ptr[d + 1]] for d in np.flatnonzero(keep)]).astype(np.int32)
    K, alpha, beta, it = 8, 0.2, 0.1, 3
    rng = np.random.default_rng(5)
    phi = rng.random((K, c.num_types)) + 0.01                     # no zero column
    phi /= phi.sum(axis=1, keepdims=True)
    o = oracle.OracleSampler(K, c.num_types, alpha, beta, SEED, threads=1)
    o.set_scheme("pcgs")
    o.set_corpus(doc_ptr, tokens)
    o.init_z_java_lcg(11)
    z = o.get_z().astype(np.int64)
    o.set_phi(phi)
    o.set_iteration(it)
    o.z_step()
    n = R.z_step(doc_ptr, tokens, z, phi, alpha, SEED, it)
    assert n == 0
    assert np.array_equal(z, o.get_z())


def test_create_model_returns_the_polyaurn_class_and_default_threshold():
    from ldagroupedgibbssampler_amd import native, sampler
    cfg = sampler.SimpleLDAConfiguration(scheme="polyaurn", topics=5)
    assert cfg.alias_poisson_threshold == 100
    m = sampler.create_model(cfg)
    assert type(m) is sampler.PolyaUrnSpaliasLDA
    assert isinstance(m, sampler.LDAPartiallyCollapsedGibbsSampler)
    assert m._scheme_flags == native.FLAG_POLYAURN == 16
    assert type(sampler.create_model(cfg, "pcgs")) is sampler.LDAPartiallyCollapsedGibbsSampler
    with pytest.raises(NotImplementedError):
        m.getTheta()
    assert sampler.SimpleLDAConfiguration(alias_poisson_threshold=7).alias_poisson_threshold == 7


def test_config_struct_carries_the_threshold():
    from ldagroupedgibbssampler_amd import _lib, native
    assert _lib.ABI_VERSION == 6
    names = [f[0] for f in _lib.GGSConfig._fields_]
    assert names[-1] == "alias_poisson_threshold" and "reserved" not in names
    cfg, _ = native._make_config(4, 10, 0.1, 0.01, 1, 0, native.FLAG_POLYAURN, 0, 1, 37)
    assert cfg.alias_poisson_threshold == 37 and cfg.flags == 16


def resource_rows():
    path = os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc", "ggs_resource_summary.txt")
    if not os.path.exists(path):
        pytest.fail("the build writes %s: run __graft_entry__.build()" % path)
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        parts = line.split()                                      # name (may hold spaces) and six numbers
        rows[" ".join(parts[:-6])] = [int(x) for x in parts[-6:]]
    return rows


def test_polyaurn_kernels_on_default_paths_use_no_scratch():
    rows = resource_rows()
    wanted = ["ggs::phi_poisson_kernel", "ggs::phi_poisson_totals_kernel", "ggs::phi_normalise_polyaurn_kernel",
              "ggs::phi_repack_polyaurn_kernel", "ggs::polyaurn_z_kernel"]
    # the lane-per-document instances polyaurn runs by default (K <= 168), and every wave-per-document instance
    wanted += ["ggs::polyaurn_sliced_kernel<%d>" % k for k in range(8, 169, 8)]
    wanted += ["ggs::polyaurn_wave_kernel<%d>" % nb for nb in (1, 2, 4, 8, 16, 32)]
    missing = [w for w in wanted if w not in rows]
    assert not missing, missing
    spills = {w: rows[w][3] for w in wanted if rows[w][3] != 0}
    assert not spills, spills
