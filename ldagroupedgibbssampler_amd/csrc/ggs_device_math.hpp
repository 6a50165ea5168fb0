// ggs_device_math.hpp -- device-side numerics of the Grouped Gibbs Sampler.
//
// Everything here must round exactly as the JVM rounds the reference's double
// arithmetic, so this translation unit is compiled with -ffp-contract=off and
// never with fast-math; products and sums below are single IEEE operations.
//
//   philox4x32_10      Salmon et al. SC'11 (Random123 constants)
//   DrawStream         java.util.Random's nextDouble()/nextGaussian() semantics
//                      (JDK 8: 26+27 bit doubles, polar Gaussian with caching)
//                      fed from the Philox blocks of one (purpose, iteration, elem)
//   strict_log/pow/exp fdlibm 5.3 e_log.c / e_pow.c / e_exp.c == java.lang.StrictMath
//   boost_pow          the same pow where the gamma draws call it: e_pow.c's main path straight-line, strict_pow elsewhere
//   rgamma             cc/mallet/util/ParallelRandoms.java:60-70,148-159
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ggs_hip.h"
#include "ggs_layout.hpp"

namespace ggs {

struct U4 { uint32_t x, y, z, w; };

__device__ __forceinline__ U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                            uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one v_mad_u64_u32 per product (measured: 100 ns of a SIMD per wave and block, against 133 with v_mul_hi_u32 + v_mul_lo_u32)
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return U4{c0, c1, c2, c3};
}

// ((next(26) << 27) + next(27)) * 2^-53 with next(n) = top n bits of a 32-bit word
// Two 32-bit conversions instead of one 64-bit one (6 VALU instructions against 12), and exact: a >> 6 < 2^26 and
// b >> 5 < 2^27 convert exactly, both scalings are by powers of two, and the sum is an integer below 2^53 times 2^-53,
// so the fma -- explicit: this file is compiled with -ffp-contract=off -- rounds nothing.
__device__ __forceinline__ double u53(uint32_t a, uint32_t b) {
  return __builtin_fma((double)(b >> 5), 0x1.0p-53, (double)(a >> 6) * 0x1.0p-26);
}
// the z step's uniform of global token gtok: the first double of block 0 of (gtok, GGS_PURPOSE_Z, iteration, seed)
__device__ __forceinline__ double z_uniform(uint64_t gtok, uint32_t iteration, uint64_t seed) {
  const U4 o = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), (uint32_t)GGS_PURPOSE_Z << 24, iteration, (uint32_t)seed, (uint32_t)(seed >> 32));
  return u53(o.x, o.y);
}

__device__ __forceinline__ int32_t hi32(double x) { return (int32_t)(__double_as_longlong(x) >> 32); }
__device__ __forceinline__ uint32_t lo32(double x) { return (uint32_t)__double_as_longlong(x); }
__device__ __forceinline__ double set_hi(double x, int32_t hi) {
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)lo32(x)));
}
__device__ __forceinline__ double clr_lo(double x) {
  return __longlong_as_double((long long)((uint64_t)__double_as_longlong(x) & 0xffffffff00000000ull));
}
__device__ __forceinline__ double mk(int32_t hi, uint32_t lo) {
  return __longlong_as_double((long long)(((uint64_t)(uint32_t)hi << 32) | lo));
}

// ---- StrictMath.log ---------------------------------------------------------
// the body; strict_log below is its one out-of-line copy, ggs_similarity.hpp's kl steps take it inline (no call in a tile body)
__device__ __forceinline__ double strict_log_body(double x) {
  constexpr double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10,
                   two54 = 1.80143985094819840000e+16,
                   Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                   Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                   Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                   Lg7 = 1.479819860511658591e-01;
  int32_t hx = hi32(x);
  const uint32_t lx = lo32(x);
  int32_t k = 0;
  if (hx < 0x00100000) {
    if (((hx & 0x7fffffff) | lx) == 0) return -__builtin_huge_val();
    if (hx < 0) return __builtin_nan("");
    k -= 54; x *= two54; hx = hi32(x);
  }
  if (hx >= 0x7ff00000) return x + x;
  k += (hx >> 20) - 1023;
  hx &= 0x000fffff;
  int32_t i = (hx + 0x95f64) & 0x100000;
  x = set_hi(x, hx | (i ^ 0x3ff00000));
  k += (i >> 20);
  const double f = x - 1.0;
  const double dk = (double)k;
  if ((0x000fffff & (2 + hx)) < 3) {
    if (f == 0.0) { if (k == 0) return 0.0; return dk * ln2_hi + dk * ln2_lo; }
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    if (k == 0) return f - R;
    return dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f);
  const double z = s * s;
  i = hx - 0x6147a;
  const double w = z * z;
  const int32_t j = 0x6b851 - hx;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6));
  const double t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  i |= j;
  const double R = t2 + t1;
  if (i > 0) {
    const double hfsq = 0.5 * f * f;
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  if (k == 0) return f - s * (f - R);
  return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}
__device__ __noinline__ double strict_log(double x) { return strict_log_body(x); }

// ---- StrictMath.exp (fdlibm 5.3 e_exp.c) ------------------------------------
__device__ __noinline__ double strict_exp(double x) {
  constexpr double huge = 1.0e+300, twom1000 = 9.33263618503218878990e-302,
                   o_threshold = 7.09782712893383973096e+02, u_threshold = -7.45133219101941108420e+02,
                   ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10,
                   invln2 = 1.44269504088896338700e+00,
                   P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
                   P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06,
                   P5 = 4.13813679705723846039e-08;
  double hi = 0.0, lo = 0.0;
  int32_t k = 0;
  uint32_t hx = (uint32_t)hi32(x);
  const int32_t xsb = (int32_t)((hx >> 31) & 1u);
  hx &= 0x7fffffffu;
  if (hx >= 0x40862E42u) {                                // |x| >= 709.78...
    if (hx >= 0x7ff00000u) {
      if (((hx & 0xfffffu) | lo32(x)) != 0) return x + x; // NaN
      return xsb == 0 ? x : 0.0;                          // exp(+-inf) = {inf, 0}
    }
    if (x > o_threshold) return huge * huge;
    if (x < u_threshold) return twom1000 * twom1000;
  }
  if (hx > 0x3fd62e42u) {                                 // |x| > 0.5 ln2
    if (hx < 0x3FF0A2B2u) {                               // and |x| < 1.5 ln2
      hi = x - (xsb ? -ln2HI : ln2HI); lo = xsb ? -ln2LO : ln2LO; k = 1 - xsb - xsb;
    } else {
      k = (int32_t)(invln2 * x + (xsb ? -0.5 : 0.5));
      const double t = (double)k;
      hi = x - t * ln2HI;
      lo = t * ln2LO;
    }
    x = hi - lo;
  } else if (hx < 0x3e300000u) {                          // |x| < 2^-28
    if (huge + x > 1.0) return 1.0 + x;
  }
  const double t = x * x;
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  if (k >= -1021) return set_hi(y, hi32(y) + (int32_t)((uint32_t)k << 20));
  return set_hi(y, hi32(y) + (int32_t)((uint32_t)(k + 1000) << 20)) * twom1000;
}

// fdlibm scalbn for finite x (only reached for subnormal pow results)
__device__ __forceinline__ double strict_scalbn(double x, int n) {
  constexpr double two54 = 1.80143985094819840000e+16, twom54 = 5.55111512312578270212e-17,
                   huge = 1.0e+300, tiny = 1.0e-300;
  int32_t hx = hi32(x);
  int32_t k = (hx & 0x7ff00000) >> 20;
  if (k == 0) {
    if ((lo32(x) | (uint32_t)(hx & 0x7fffffff)) == 0) return x;
    x *= two54; hx = hi32(x);
    k = ((hx & 0x7ff00000) >> 20) - 54;
    if (n < -50000) return tiny * x;
  }
  if (k == 0x7ff) return x + x;
  k = k + n;
  if (k > 0x7fe) return huge * __builtin_copysign(huge, x);
  if (k > 0) return set_hi(x, (hx & (int32_t)0x800fffff) | (k << 20));
  if (k <= -54) {
    if (n > 50000) return huge * __builtin_copysign(huge, x);
    return tiny * __builtin_copysign(tiny, x);
  }
  k += 54;
  x = set_hi(x, (hx & (int32_t)0x800fffff) | (k << 20));
  return x * twom54;
}

// ---- StrictMath.pow for x >= +0 finite, y finite (the domain of
// ParallelRandoms.java:66, Math.pow(u, 1.0/alpha)) ----------------------------
__device__ __noinline__ double strict_pow(double x, double y) {
  constexpr double two53 = 9007199254740992.0, huge = 1.0e300, tiny = 1.0e-300,
      L1 = 5.99999999999994648725e-01, L2 = 4.28571428578550184252e-01,
      L3 = 3.33333329818377432918e-01, L4 = 2.72728123808534006489e-01,
      L5 = 2.30660745775561754067e-01, L6 = 2.06975017800338417784e-01,
      P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
      P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06,
      P5 = 4.13813679705723846039e-08,
      lg2 = 6.93147180559945286227e-01, lg2_h = 6.93147182464599609375e-01,
      lg2_l = -1.90465429995776804525e-09, ovt = 8.0085662595372944372e-0017,
      cp = 9.61796693925975554329e-01, cp_h = 9.61796700954437255859e-01,
      cp_l = -7.02846165095275826516e-09, ivln2 = 1.44269504088896338700e+00,
      ivln2_h = 1.44269502162933349609e+00, ivln2_l = 1.92596299112661746887e-08;
  const int32_t hx = hi32(x), hy = hi32(y);
  const uint32_t lx = lo32(x), ly = lo32(y);
  int32_t ix = hx & 0x7fffffff;
  const int32_t iy = hy & 0x7fffffff;
  if ((iy | ly) == 0) return 1.0;
  if (hx < 0 || ix >= 0x7ff00000 || iy >= 0x7ff00000) return __builtin_nan("");
  if ((ix | lx) == 0) return (hy < 0) ? __builtin_huge_val() : 0.0;
  if (ix == 0x3ff00000 && lx == 0) return 1.0;
  if (hy == 0x3ff00000 && ly == 0) return x;
  double ax = x, t1, t2;
  if (iy > 0x41e00000) {
    if (iy > 0x43f00000) {
      if (ix <= 0x3fefffff) return (hy < 0) ? huge * huge : tiny * tiny;
      if (ix >= 0x3ff00000) return (hy > 0) ? huge * huge : tiny * tiny;
    }
    if (ix < 0x3fefffff) return (hy < 0) ? huge * huge : tiny * tiny;
    if (ix > 0x3ff00000) return (hy > 0) ? huge * huge : tiny * tiny;
    const double t = ax - 1.0;
    const double w = (t * t) * (0.5 - t * (0.3333333333333333333333 - t * 0.25));
    const double u = ivln2_h * t;
    const double v = t * ivln2_l - w * ivln2;
    t1 = clr_lo(u + v);
    t2 = v - (t1 - u);
  } else {
    int32_t n = 0, k;
    if (ix < 0x00100000) { ax *= two53; n -= 53; ix = hi32(ax); }
    n += (ix >> 20) - 0x3ff;
    const int32_t j = ix & 0x000fffff;
    ix = j | 0x3ff00000;
    if (j <= 0x3988E) k = 0;
    else if (j < 0xBB67A) k = 1;
    else { k = 0; n += 1; ix -= 0x00100000; }
    ax = set_hi(ax, ix);
    const double bpk = k ? 1.5 : 1.0;
    const double dp_hk = k ? 5.84962487220764160156e-01 : 0.0;
    const double dp_lk = k ? 1.35003920212974897128e-08 : 0.0;
    double u = ax - bpk;
    double v = 1.0 / (ax + bpk);
    const double ss = u * v;
    const double s_h = clr_lo(ss);
    double t_h = mk(((ix >> 1) | 0x20000000) + 0x00080000 + (k << 18), 0u);
    double t_l = ax - (t_h - bpk);
    const double s_l = v * ((u - s_h * t_h) - s_h * t_l);
    double s2 = ss * ss;
    double r = s2 * s2 * (L1 + s2 * (L2 + s2 * (L3 + s2 * (L4 + s2 * (L5 + s2 * L6)))));
    r += s_l * (s_h + ss);
    s2 = s_h * s_h;
    t_h = clr_lo(3.0 + s2 + r);
    t_l = r - ((t_h - 3.0) - s2);
    u = s_h * t_h;
    v = s_l * t_h + t_l * ss;
    const double p_h = clr_lo(u + v);
    const double p_l = v - (p_h - u);
    const double z_h = cp_h * p_h;
    const double z_l = cp_l * p_h + p_l * cp + dp_lk;
    const double t = (double)n;
    t1 = clr_lo(((z_h + z_l) + dp_hk) + t);
    t2 = z_l - (((t1 - t) - dp_hk) - z_h);
  }
  const double y1 = clr_lo(y);
  double p_l = (y - y1) * t1 + y * t2;
  double p_h = y1 * t1;
  double z = p_l + p_h;
  int32_t j = hi32(z);
  int32_t i = (int32_t)lo32(z);
  if (j >= 0x40900000) {
    if (((j - 0x40900000) | i) != 0) return huge * huge;
    if (p_l + ovt > z - p_h) return huge * huge;
  } else if ((j & 0x7fffffff) >= 0x4090cc00) {
    if (((j - (int32_t)0xc090cc00) | i) != 0) return tiny * tiny;
    if (p_l <= z - p_h) return tiny * tiny;
  }
  i = j & 0x7fffffff;
  int32_t k = (i >> 20) - 0x3ff;
  int32_t n = 0;
  if (i > 0x3fe00000) {
    n = j + (0x00100000 >> (k + 1));
    k = ((n & 0x7fffffff) >> 20) - 0x3ff;
    const double t = mk(n & ~(0x000fffff >> k), 0u);
    n = ((n & 0x000fffff) | 0x00100000) >> (20 - k);
    if (j < 0) n = -n;
    p_h -= t;
  }
  double t = clr_lo(p_l + p_h);
  const double u = t * lg2_h;
  const double v = (p_l - (t - p_h)) * lg2 + t * lg2_l;
  z = u + v;
  const double w = v - (z - u);
  t = z * z;
  t1 = z - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  const double r = (z * t1) / (t1 - 2.0) - (w + z * w);
  z = 1.0 - (r - z);
  j = hi32(z);
  j += (int32_t)((uint32_t)n << 20);
  if ((j >> 20) <= 0) return strict_scalbn(z, n);
  return set_hi(z, j);
}

// ---- the boost's pow: e_pow.c's main path as straight-line code ----------------
// The boost of a gamma draw (ParallelRandoms.java:66) raises the element's first uniform, a multiple of 2^-53 in [0, 1),
// to 1/shape with shape < 1.  On
//   x normal with 0 < x < 1,
//   the high word of y in (0x3ff00000, 0x41e00000]   (1 + 2^-20 <= y < 2^31 + 2^11),
//   the high word of |y log2 x| as e_pow.c forms it below 0x40900000   (|y log2 x| < 1024), and a normal result
// strict_pow takes none of its early returns, neither of its rescalings (subnormal x, scalbn) and not the |y| > 2^31
// branch: what is left is the sequence of IEEE operations below, the same operations in the same order, with fdlibm's
// three-way choice of k and its `i > 0x3fe00000` block turned into selects (a lane outside that block subtracts +0.0
// from p_h, which changes no bit of it).  Where any of the four conditions fails -- x = 0, subnormal or >= 1,
// y <= 1 + 2^-20 or >= 2^31 + 2^11 or not finite, a result that underflows or is subnormal -- the function returns NaN,
// which no result inside the domain is, and the caller goes to strict_pow.  The shift counts are masked to five bits,
// which is what the hardware does and changes nothing inside the domain (there they are 0..20), and the integer sums
// that can wrap outside the domain are unsigned: outside it the arithmetic stays defined.
// __noinline__ like strict_pow: inlined at its three call sites it cost theta_kernel a wave per SIMD (67 -> 75 VGPRs).
__device__ __noinline__ double strict_pow_unit(double x, double y) {
  constexpr double
      L1 = 5.99999999999994648725e-01, L2 = 4.28571428578550184252e-01,
      L3 = 3.33333329818377432918e-01, L4 = 2.72728123808534006489e-01,
      L5 = 2.30660745775561754067e-01, L6 = 2.06975017800338417784e-01,
      P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03,
      P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06,
      P5 = 4.13813679705723846039e-08,
      lg2 = 6.93147180559945286227e-01, lg2_h = 6.93147182464599609375e-01,
      lg2_l = -1.90465429995776804525e-09,
      cp = 9.61796693925975554329e-01, cp_h = 9.61796700954437255859e-01,
      cp_l = -7.02846165095275826516e-09;
  const int32_t hx = hi32(x), hy = hi32(y);
  bool in_domain = (uint32_t)hx - 0x00100000u < 0x3ff00000u - 0x00100000u && (uint32_t)hy - 0x3ff00001u <= 0x41e00000u - 0x3ff00001u;
  // log2(x) = t1 + t2
  const int32_t jx = hx & 0x000fffff;
  const bool k = jx > 0x3988E && jx < 0xBB67A, up = jx >= 0xBB67A;
  const int32_t ix = jx | (up ? 0x3fe00000 : 0x3ff00000);
  const double t = (double)((hx >> 20) - 0x3ff + (up ? 1 : 0));
  const double ax = set_hi(x, ix);
  const double bpk = k ? 1.5 : 1.0;
  const double dp_hk = k ? 5.84962487220764160156e-01 : 0.0;
  const double dp_lk = k ? 1.35003920212974897128e-08 : 0.0;
  double u = ax - bpk;
  double v = 1.0 / (ax + bpk);
  const double ss = u * v;
  const double s_h = clr_lo(ss);
  double t_h = mk(((ix >> 1) | 0x20000000) + 0x00080000 + (k ? 0x00040000 : 0), 0u);
  double t_l = ax - (t_h - bpk);
  const double s_l = v * ((u - s_h * t_h) - s_h * t_l);
  double s2 = ss * ss;
  double r = s2 * s2 * (L1 + s2 * (L2 + s2 * (L3 + s2 * (L4 + s2 * (L5 + s2 * L6)))));
  r += s_l * (s_h + ss);
  s2 = s_h * s_h;
  t_h = clr_lo(3.0 + s2 + r);
  t_l = r - ((t_h - 3.0) - s2);
  u = s_h * t_h;
  v = s_l * t_h + t_l * ss;
  double p_h = clr_lo(u + v);
  double p_l = v - (p_h - u);
  const double z_h = cp_h * p_h;
  const double z_l = cp_l * p_h + p_l * cp + dp_lk;
  const double t1 = clr_lo(((z_h + z_l) + dp_hk) + t);
  const double t2 = z_l - (((t1 - t) - dp_hk) - z_h);
  // y * log2(x) = p_h + p_l, split into the integer n and the rest
  const double y1 = clr_lo(y);
  p_l = (y - y1) * t1 + y * t2;
  p_h = y1 * t1;
  double z = p_l + p_h;
  int32_t j = hi32(z);
  const int32_t i = j & 0x7fffffff;
  in_domain = in_domain && i < 0x40900000;
  const bool split = i > 0x3fe00000;
  int32_t n = (int32_t)((uint32_t)j + (0x00100000u >> (((i >> 20) - 0x3ff + 1) & 31)));
  const int32_t kn = ((n & 0x7fffffff) >> 20) - 0x3ff;
  const int32_t th = n & ~(0x000fffff >> (kn & 31));
  n = ((n & 0x000fffff) | 0x00100000) >> ((20 - kn) & 31);
  if (j < 0) n = -n;
  n = split ? n : 0;
  p_h -= mk(split ? th : 0, 0u);
  // 2^(p_h + p_l)
  const double tt = clr_lo(p_l + p_h);
  u = tt * lg2_h;
  v = (p_l - (tt - p_h)) * lg2 + tt * lg2_l;
  z = u + v;
  const double w = v - (z - u);
  const double zz = z * z;
  const double e1 = z - zz * (P1 + zz * (P2 + zz * (P3 + zz * (P4 + zz * P5))));
  r = (z * e1) / (e1 - 2.0) - (w + z * w);
  z = 1.0 - (r - z);
  j = (int32_t)((uint32_t)hi32(z) + ((uint32_t)n << 20));
  in_domain = in_domain && (j >> 20) > 0;
  return in_domain ? set_hi(z, j) : __builtin_nan("");
}
// pow as the gamma draws call it: the straight-line form, and strict_pow for the lanes it does not cover.  The test is
// one scalar branch per wave, so a wave whose lanes are all inside the domain (every wave of the theta draw at
// alpha = 0.1; 95 % of the Phi draw's at beta = 0.01, where u < 2^-10.22 leaves the normal range) runs no call.
__device__ __forceinline__ double boost_pow(double u, double inv_alpha) {
  double r = strict_pow_unit(u, inv_alpha);
  const bool outside = r != r;
  if (__ballot(outside) != 0) {
    if (outside) r = strict_pow(u, inv_alpha);
  }
  return r;
}

// ---- per-draw stream ----------------------------------------------------------
struct DrawStream {
  uint32_t k0, k1, c0, c1, c2base, c3;
  uint32_t pos;
  int32_t cached;     // block whose doubles are in d0/d1, -1 = none
  double d0, d1;
  double next_gauss;
  bool have_gauss;
  bool exhausted;

  __device__ __forceinline__ DrawStream(uint64_t seed, uint32_t iter, uint32_t purpose, uint64_t elem)
      : k0((uint32_t)seed), k1((uint32_t)(seed >> 32)), c0((uint32_t)elem), c1((uint32_t)(elem >> 32)),
        c2base(purpose << 24), c3(iter), pos(0), cached(-1), d0(0), d1(0), next_gauss(0),
        have_gauss(false), exhausted(false) {}

  __device__ __forceinline__ double next_double() {
    const uint32_t blk = pos >> 1;
    if (blk >= (uint32_t)GGS_MAX_BLOCKS) { exhausted = true; return 0.5; }
    if ((int32_t)blk != cached) {
      const U4 o = philox4x32_10(c0, c1, c2base | blk, c3, k0, k1);
      d0 = u53(o.x, o.y);
      d1 = u53(o.z, o.w);
      cached = (int32_t)blk;
    }
    const double d = (pos & 1u) ? d1 : d0;
    ++pos;
    return d;
  }
  // java.util.Random.nextGaussian
  __device__ __forceinline__ double next_gaussian() {
    if (have_gauss) { have_gauss = false; return next_gauss; }
    double v1, v2, s;
    do {
      v1 = 2 * next_double() - 1;
      v2 = 2 * next_double() - 1;
      s = v1 * v1 + v2 * v2;
      if (exhausted) return 0.0;
    } while (s >= 1 || s == 0);
    const double multiplier = sqrt(-2 * strict_log(s) / s);
    next_gauss = v2 * multiplier;
    have_gauss = true;
    return v1 * multiplier;
  }
};

// What a gamma draw needs of its shape and of nothing else: the boost decision of ParallelRandoms.java:61-66 and the
// constants of the Marsaglia-Tsang loop (ParallelRandoms.java:149-150).  Cells with the same shape have bit-equal constants,
// so a draw may take them from a table that another lane filled (the theta and Phi draws: one entry per document or tile
// column for the cells with count 0) instead of spending a square root and three divisions on its own.
struct GammaConsts {
  double shape;       // as given: Gamma(shape) is what is drawn
  double d, c;        // of the boosted shape: 1 + shape where shape < 1
  double inv_alpha;   // 1.0 / shape, the boost's exponent: set where boost is
  bool boost;
};
__device__ __forceinline__ GammaConsts gamma_consts(double alpha) {
  GammaConsts k;
  k.shape = alpha;
  k.boost = alpha < 1;
  const double shape = k.boost ? 1 + alpha : alpha;
  k.d = shape - (1.0 / 3.0);
  k.c = 1.0 / sqrt(9.0 * k.d);
  k.inv_alpha = k.boost ? 1.0 / alpha : 0.0;
  return k;
}

// ParallelRandoms.java:148-159
__device__ __forceinline__ double prgamma(DrawStream &r, const double d, const double c) {
  for (;;) {
    double x, v;
    do {
      x = r.next_gaussian();
      v = 1.0 + c * x;
      if (r.exhausted) return __builtin_nan("");
    } while (v <= 0.0);
    v = v * v * v;
    const double u = r.next_double();
    if (u < (1.0 - 0.0331 * (x * x) * (x * x))) return d * v;
    if (strict_log(u) < (0.5 * x * x + d * (1.0 - v + strict_log(v)))) return d * v;
    if (r.exhausted) return __builtin_nan("");
  }
}
// ParallelRandoms.java:60-70 with beta = 1, lambda = 0
// One prgamma instance for both branches: a wave usually mixes shapes below and above 1 (sparse
// counts), and two inlined copies would run one after the other.  The boost uniform is the
// element's first draw whatever the shape (stream layout, see oracle/ggs_oracle.c rgamma): every
// lane is then at the same stream position at every call site and new Philox blocks are needed
// by all lanes together.
__device__ __forceinline__ double rgamma(DrawStream &r, const GammaConsts &k) {
  const double u = r.next_double();                  // drawn BEFORE the Marsaglia-Tsang loop, as at ParallelRandoms.java:62
  const double g = prgamma(r, k.d, k.c);
  return k.boost ? g * boost_pow(u, k.inv_alpha) : g;
}
__device__ __forceinline__ double rgamma(DrawStream &r, double alpha) { return rgamma(r, gamma_consts(alpha)); }

// The same draw when nothing is rejected twice -- straight-line code for a whole wave.  rgamma's loops cost a wave the
// MAXIMUM over its 64 lanes: the polar method rejects 21 % of its pairs (3.3 rounds until all lanes hold one), and one
// lane in seven fails the squeeze of Marsaglia-Tsang, so both log tests and a second round of the outer loop are
// executed by practically every wave.  Here every lane evaluates polar attempts 0 and 1 (stream positions 1-2 and
// 3-4: Philox blocks 0-2) and the squeeze test once, with exactly the operations rgamma would perform on that path;
// a lane for which that does not settle the draw (both pairs rejected 4.6 %, squeeze failed ~9 %, v <= 0) returns false
// and its element is drawn by rgamma from the start of its stream -- by the caller, gathered into full waves.
// `k` may live in LDS (a table entry): its fields are read where they are used.
__device__ __forceinline__ bool rgamma_first_try(uint64_t seed, uint32_t iter, uint32_t purpose, uint64_t elem, const GammaConsts &k, double &g) {
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32), c0 = (uint32_t)elem, c1 = (uint32_t)(elem >> 32), c2 = purpose << 24;
  const U4 b0 = philox4x32_10(c0, c1, c2, iter, k0, k1), b1 = philox4x32_10(c0, c1, c2 | 1u, iter, k0, k1),
           b2 = philox4x32_10(c0, c1, c2 | 2u, iter, k0, k1);
  const double u0 = u53(b0.x, b0.y);                                  // position 0: the boost uniform
  const double a1 = 2 * u53(b0.z, b0.w) - 1, a2 = 2 * u53(b1.x, b1.y) - 1, sa = a1 * a1 + a2 * a2;    // positions 1, 2
  const double w = u53(b1.z, b1.w);                                   // position 3: the acceptance uniform, or the next pair's first
  const double e1 = 2 * w - 1, e2 = 2 * u53(b2.x, b2.y) - 1, sb = e1 * e1 + e2 * e2;                  // positions 3, 4
  const bool ok_a = !(sa >= 1 || sa == 0), ok_b = !(sb >= 1 || sb == 0);
  if (!(ok_a || ok_b)) return false;
  const double v1 = ok_a ? a1 : e1, s = ok_a ? sa : sb;
  const double u = ok_a ? w : u53(b2.z, b2.w);                        // position 3 or 5
  const double multiplier = sqrt(-2 * strict_log(s) / s);
  const double x = v1 * multiplier;
  double v = 1.0 + k.c * x;
  if (!(v > 0.0)) return false;                                       // rgamma: the cached second Gaussian comes next
  v = v * v * v;
  if (!(u < (1.0 - 0.0331 * (x * x) * (x * x)))) return false;        // rgamma: the log test, perhaps another round
  const double r = k.d * v;
  g = k.boost ? r * boost_pow(u0, k.inv_alpha) : r;
  return true;
}
__device__ __forceinline__ bool rgamma_first_try(uint64_t seed, uint32_t iter, uint32_t purpose, uint64_t elem, double alpha, double &g) {
  return rgamma_first_try(seed, iter, purpose, elem, gamma_consts(alpha), g);
}

}  // namespace ggs
