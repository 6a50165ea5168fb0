"""The scalar math under the gamma draws, bit for bit against the oracle: `u53` in its two-conversion form, and the boost's
`pow` as the draws call it (`boost_pow`: e_pow.c's main path as straight-line code on its own domain, the general
`strict_pow` for the lanes of a wave outside it, decided by a ballot).

The general device functions are pinned to the oracle by test_parity_gpu.py::test_strict_math_device_bit_exact; here the
inputs sit where the new code can go wrong: on the table boundaries of e_pow.c, on either side of every edge of the fast
domain, with one lane of an otherwise in-domain wave outside it (first lane, last lane, middle, ragged last wave), and
in the draws themselves with shapes that put 1/shape on both sides of each edge.  `strict_log` has no straight-line
form, so there is no case for one.
"""
import numpy as np
import pytest

from tests.ranks import assert_bit_equal

pytestmark = pytest.mark.gpu

ALPHA, BETA = 0.1, 0.01                    # the benchmark's priors: y = 10 and y = 100
BOUNDARY_MANTISSAS = (0x3988E, 0x3988F, 0xBB679, 0xBB67A)      # e_pow.c's choice of k changes between each pair


def _double(exponent, mant20, low):
    """The double 2^exponent * 1.m with the high word's low 20 bits mant20 and the low word low."""
    bits = ((np.uint64(1023 + exponent) << np.uint64(52)) | (np.uint64(mant20) << np.uint64(32)) | np.uint64(low))
    return np.array([bits], np.uint64).view(np.float64)[0]


def _steps(x, n):
    """x and its n neighbours on either side."""
    out = [x]
    lo = hi = x
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _exponents():
    rng = np.random.default_rng(11)
    m = rng.integers(1, 5000, 8).astype(np.float64)
    ys = [10.0, 1 / ALPHA, 100.0, 1 / BETA, 2.0, 1.5, 3.5]
    ys += list(1.0 / ((ALPHA / m) * m)) + list(1.0 / ((BETA / m) * m))          # 1 / shape of a count-0 cell: (prior / magnitude) * magnitude
    ys += list(1.0 / rng.uniform(2.0 ** -20, 1.0, 10))
    return np.array(ys)


def fast_path_cases():
    rng = np.random.default_rng(12)
    xs = list(rng.integers(1, 2 ** 53, 8000).astype(np.float64) * 2.0 ** -53)                  # what a uniform can be
    xs += list(rng.integers(1, 2 ** 53, 2000).astype(np.float64) * 2.0 ** -rng.integers(54, 107, 2000).astype(np.float64))  # small ones: k below 2^52 .. 1
    xs += [2.0 ** -53, 2.0 ** -52, 0.5, 1 - 2.0 ** -53]
    for e in (-1, -2, -3, -7, -10, -11, -30, -53):
        for m in BOUNDARY_MANTISSAS:
            xs += [_double(e, m, 0), _double(e, m, 0xFFFFFFFF)]
    ys = _exponents()
    x = np.tile(np.array(xs), ys.size)
    y = np.repeat(ys, len(xs))
    # |y log2 x| on either side of 0.5, the `i > 0x3fe00000` split, and of 1 and 2, where n changes
    ex, ey = [], []
    for yy in ys:
        for t in (-0.5, -1.0, -1.5, -2.0):
            near = _steps(np.exp2(t / yy), 24)
            ex += near
            ey += [yy] * len(near)
    return np.concatenate([x, ex]), np.concatenate([y, ey])


def test_boost_pow_fast_path(native, oracle):
    x, y = fast_path_cases()
    assert 200000 < x.size < 600000
    assert_bit_equal(native.debug_math("boost_pow", x, y), oracle.pow(x, y), "pow of the boost, fast domain")


def out_of_domain_cases():
    """(x, y) that the straight-line form must hand to strict_pow, and their nearest neighbours that it keeps."""
    sub = 5e-324
    near_one = 1 - 2.0 ** -53
    c = [(0.0, 10.0), (0.0, 100.0), (sub, 10.0), (2.0 ** -1023, 1.5), (2.0 ** -1022, 1.5), (1.0, 10.0), (1.5, 10.0), (3.0, 100.0), (1e300, 3.5),
         (0.3, 1.0), (0.3, 1 + 2.0 ** -52), (0.3, 1 + 2.0 ** -21), (0.3, 1 + 2.0 ** -20),
         (near_one, 2.0 ** 31), (0.3, 2.0 ** 31), (near_one, np.nextafter(2.0 ** 31, np.inf)), (0.3, np.nextafter(2.0 ** 31, np.inf)),
         (near_one, 2.0 ** 31 + 2.0 ** 11), (near_one, 2.0 ** 64), (0.3, 2.0 ** 64),
         (2.0 ** -53, 100.0), (1e-11, 100.0), (2.0 ** -53, 2.0 ** 31),                       # underflow to 0
         (2.0 ** -10.5, 100.0), (2.0 ** -10.74, 100.0), (2.0 ** -53, 20.0), (2.0 ** -53, 20.27)]  # subnormal results: scalbn
    for yy in (100.0, 1 / BETA, 20.0):                                                       # the last normal and the first subnormal result
        c += [(xx, yy) for xx in _steps(np.exp2(-1022.0 / yy), 3)]
    c += [(xx, 100.0) for xx in _steps(np.exp2(-10.24), 2)]                                  # |y log2 x| = 1024, where the fast form stops looking
    return c


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_boost_pow_leaves_its_domain_per_lane(native, oracle, n):
    """One lane outside the domain in a wave that is otherwise inside it: first lane, last lane, middle, the ragged last
    wave (n = 65: one lane; n = 257: a last workgroup of one lane); and whole arrays outside it."""
    rng = np.random.default_rng(13)
    base_x = rng.integers(2 ** 43, 2 ** 53, n).astype(np.float64) * 2.0 ** -53             # >= 2^-10: inside the domain at y = 100
    base_y = np.where(np.arange(n) % 2 == 0, 10.0, 100.0)
    assert_bit_equal(native.debug_math("boost_pow", base_x, base_y), oracle.pow(base_x, base_y), "n=%d, all lanes inside" % n)
    places = sorted({p for p in (0, 31, 63, 64, 64 + 31, 127, 256, n // 2, n - 1) if p < n})
    for cx, cy in out_of_domain_cases():
        for p in places:
            x, y = base_x.copy(), base_y.copy()
            x[p], y[p] = cx, cy
            assert_bit_equal(native.debug_math("boost_pow", x, y), oracle.pow(x, y), "n=%d, (%r, %r) at %d" % (n, cx, cy, p))
        x, y = np.full(n, cx), np.full(n, cy)
        assert_bit_equal(native.debug_math("boost_pow", x, y), oracle.pow(x, y), "n=%d, (%r, %r) everywhere" % (n, cx, cy))


def test_u53_two_conversions(native):
    rng = np.random.default_rng(14)
    edge = np.array([0, 0xFFFFFFFF, 0x3F, 0x1F, 0x40, 0x20, 0x80000000, 0xFFFFFFC0, 0xFFFFFFE0, 0x7FFFFFFF], np.uint64)
    a = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64), np.repeat(edge, edge.size)])
    b = np.concatenate([rng.integers(0, 2 ** 32, 200000, dtype=np.uint64), np.tile(edge, edge.size)])
    m = ((a >> np.uint64(6)) << np.uint64(27)) + (b >> np.uint64(5))                       # ((next(26) << 27) + next(27)): below 2^53
    want = m.astype(np.float64) * 2.0 ** -53                                               # both steps exact
    assert_bit_equal(native.debug_math("u53", a.astype(np.float64), b.astype(np.float64)), want, "u53")
    assert want.max() == 1 - 2.0 ** -53 and want.min() == 0.0


# 1/shape on both sides of each edge of the fast domain: rounds to 1; inside 1 + 2^-20; well inside; at 2^31 (inside) and at
# 2^32 (the |y| > 2^31 branch); far beyond 2^64.  5.0 and 1.0 do not boost: their lanes stay out of the boost's ballot.
DRAW_SHAPES = (1 - 2.0 ** -53, 0.999999, 0.5, ALPHA, BETA, 2.0 ** -31, 2.0 ** -32, 1e-300, 5.0, 1.0)


@pytest.mark.parametrize("kind", ["gamma_first_try", "gamma"])
def test_draws_across_the_domain_edges(native, oracle, kind):
    seed, it = 0x0123456789ABCDEF, 3
    blocks = np.repeat(np.array(DRAW_SHAPES), 64)                                            # one wave per shape
    mixed = np.tile(np.array(DRAW_SHAPES), 64)                                               # all of them lane by lane
    for tag, shape in (("a wave per shape", blocks), ("lane by lane", mixed)):
        dev, st = native.debug_draw(kind, seed, it, native.PURPOSE_PHI, 2 ** 33 + 7, shape=shape)
        assert st == 0
        assert_bit_equal(dev, oracle.gammas(seed, it, oracle.PURPOSE_PHI, 2 ** 33 + 7, shape), "%s, %s" % (kind, tag))
