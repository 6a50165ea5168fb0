"""A numpy restatement of the float32 decision rule of z_sliced32_kernel (ggs_z_sliced.hpp, ColdForm32): float32
operands (phi32_of), float32 products and prefix sums, t0' = fl32(fl64(U * A)), d_j = fl32(a_j - t0'), decided as
cnt = #{d_j < 0} when 2^-60 <= A <= FLT_MAX, min(t0', |d_j|) > (2K + 8) 2^-24 A and cnt < K.  Checked against the
Java walk (GGS:96-113 in fp64) on random and adversarial rows, with float32 denormals kept and flushed: a decided
token is never drawn differently, and an invalid walk is never decided.  Prints the undecided rate."""
import numpy as np
import pytest

F32_MIN = np.float32(2.0 ** -126)


def ftz(x, on):
    return np.where(np.abs(x) < F32_MIN, np.float32(0.0) * np.sign(x), x).astype(np.float32) if on else x


def phi32_of(x):
    with np.errstate(invalid="ignore"):
        ok = (x >= 0.0) & (x <= 1.0)
    return np.where(ok, x, np.nan).astype(np.float32)


def java_draw(theta, phi, U):
    """GGS:96-113 per row: -1 / K for the walks Java does not end inside [0, K)."""
    p = theta * phi
    S = np.add.accumulate(p, axis=1)[:, -1]
    t = np.subtract.accumulate(np.concatenate([(U * S)[:, None], p], axis=1), axis=1)   # t_0 .. t_K, sequential
    pos = t > 0.0
    first_le = np.where(~pos.all(axis=1), np.argmin(pos, axis=1), t.shape[1])     # first j with t_j <= 0 (or none)
    return first_le - 1                                                          # K: the walk ran past the row


def kernel_rule(theta, phi, U, K, KMAX, flush, margin=1.0):
    n = theta.shape[0]
    th = np.zeros((n, KMAX), np.float32)
    ph = np.zeros((n, KMAX), np.float32)
    th[:, :K] = ftz(phi32_of(theta), flush)
    ph[:, :K] = ftz(phi32_of(phi), flush)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        q = ftz(th * ph, flush)
        a = np.empty_like(q)
        acc = np.zeros(n, np.float32)
        for j in range(KMAX):                                   # the prefix chain, fp32, one rounding per add
            acc = ftz(acc + q[:, j], flush)
            a[:, j] = acc
        A = a[:, -1]
        t0 = ftz((U * A.astype(np.float64)).astype(np.float32), flush)
        d = ftz(a - t0[:, None], flush)
        cnt = np.signbit(d).sum(axis=1)
        m = np.minimum(t0, np.min(np.abs(d), axis=1))
        delta = ftz(ftz(np.float32(2 * K + 8) * np.float32(2.0 ** -24) * A, flush) * np.float32(margin), flush)
        decided = (A >= np.float32(2.0 ** -60)) & (A <= np.finfo(np.float32).max) & (m > delta) & (cnt < K)
    return decided, cnt


def rows(rng, n, K, kind):
    theta = rng.dirichlet(np.full(K, 0.1), n)
    phi = rng.gamma(0.01, size=(n, K)) / 30.0                     # Gamma(0.01) columns: values down to 1e-300 and below
    phi = np.minimum(phi, 1.0)
    if kind == "ties":
        theta = np.full((n, K), 1.0 / K)
        phi = np.repeat(rng.choice([0.25, 1e-3, 2.0 ** -30], n)[:, None], K, axis=1)
    elif kind == "tiny":
        phi = np.where(rng.random((n, K)) < 0.5, 1e-300, rng.choice([1e-40, 2.0 ** -126, 3e-39, 1e-45], (n, K)))
        theta = np.where(rng.random((n, K)) < 0.3, 4.9e-324, theta)                # Double.MIN_VALUE, the clamp
    elif kind == "zero":
        phi[: n // 2] = 0.0
        theta[n // 2:] = 0.0
    elif kind == "nan":
        phi[np.arange(n), rng.integers(0, K, n)] = np.nan
        phi[: n // 4, 0] = 1.5                                    # out of [0, 1]: NaN in the shadow
    elif kind == "dominant":
        phi = np.full((n, K), 1e-30)
        phi[np.arange(n), rng.integers(0, K, n)] = 0.5
    elif kind == "mixed":
        phi = np.where(rng.random((n, K)) < 0.5, phi, rng.choice([1e-300, 1e-42, 0.0], (n, K)))
    return theta, phi


@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("K", [1, 20, 100, 104, 113, 160])
@pytest.mark.parametrize("kind", ["random", "ties", "tiny", "zero", "nan", "dominant", "mixed"])
def test_margin32_never_decides_another_topic(K, kind, flush):
    rng = np.random.default_rng(1000 * K + len(kind) + flush)
    n = 20000 if kind == "random" else 4000
    KMAX = (K + 7) // 8 * 8
    theta, phi = rows(rng, n, K, kind)
    U = rng.random(n)
    U[:8] = [0.0, 2.0 ** -53, 0.5, 1.0 - 2.0 ** -53, 0.25, 0.75, 1e-10, 1.0 - 1e-10]
    java = java_draw(theta, phi, U)
    decided, cnt = kernel_rule(theta, phi, U, K, KMAX, flush)
    bad = decided & (cnt != java)
    assert not bad.any(), (np.flatnonzero(bad)[:5], cnt[bad][:5], java[bad][:5])
    invalid = (java < 0) | (java >= K)
    assert not (decided & invalid).any()
    rate = 1.0 - decided[~invalid].mean() if (~invalid).any() else 0.0
    print("K=%d %s flush=%d: undecided %.3g of %d valid draws" % (K, kind, flush, rate, (~invalid).sum()))
    if kind == "random" and K > 1:
        assert rate < 0.02                                         # the rule decides: the replay stays the exception


@pytest.mark.parametrize("K", [20, 100, 160])
def test_margin32_exact_ties_at_the_draw(K):
    """U*A lands exactly on a partial sum: the rule must leave it to the replay."""
    rng = np.random.default_rng(K)
    n = 2000
    theta = np.full((n, K), 1.0 / 64)
    phi = np.full((n, K), 0.5)
    j = rng.integers(0, K, n)
    S = np.add.accumulate(theta * phi, axis=1)
    U = S[np.arange(n), j] / S[:, -1]
    java = java_draw(theta, phi, U)
    decided, cnt = kernel_rule(theta, phi, U, K, (K + 7) // 8 * 8, False)
    assert not (decided & (cnt != java)).any()
    assert not decided.any()


def test_margin32_scaled_margin_decides_nothing():
    """GGS_DEBUG_MARGIN large enough (delta > A) sends every token to the replay."""
    rng = np.random.default_rng(5)
    K = 100
    theta, phi = rows(rng, 2000, K, "random")
    decided, _ = kernel_rule(theta, phi, rng.random(2000), K, 104, False, margin=1e9)
    assert not decided.any()
