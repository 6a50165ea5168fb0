// ggs_phi_poisson.hpp -- the Phi draw of scheme=polyaurn (PolyaUrnSpaliasLDA.java: createDirichletSampler :67, the
// sampler PolyaUrnDirichletFixedCoeffPoisson.nextDistributionWithSparseness :17-40 over PoissonFixedCoeffSampler :31-50
// and PolyaUrnDirichlet.nextPoissonNormalApproximation :102-107).  Each cell (k, v) draws X ~ Poisson(beta + n_kv); a
// topic's row is X / sum_v X, or all zero when that sum is 0 (:33).  No gammas, no rejection loops in the common case and
// no exact-sum walk: the normaliser is an integer, exact in any order.
//
// Per cell, with c = n_kv, lambda = beta + c (fp64), element e = k * V + v and the purpose of ggs_hip.h:
//   c <  L  X = the smallest j with u < T_c[j]; u = the element's first uniform; T_c = row c of the host-built table
//           (build_poisson_table, ggs_host_phi.hpp): the pmf of Poisson(lambda) truncated to 2L entries, renormalised, as a
//           cumulative table with T_c[2L - 1] = 1.  The reference samples the same truncated pmf with a Walker alias
//           table; inverse CDF makes X a pure function of (u, table), so the search order cannot change a bit.
//   c >= L  X = max(0, floor(sqrt(lambda) * g + lambda + 0.5)); g = the element's first Gaussian (java.util.Random's
//           polar method on the Philox stream, as everywhere here).  The reference keeps a negative value; it needs g < -10.
// Most cells have c = 0 and u below T_0[0] (exp(-beta) renormalised: 0.99 at beta = 0.01): one Philox block and one
// compare settle them; the rest search their table row (2L doubles, L2-resident) by bisection.
#pragma once
#include "ggs_kernels.hpp"

namespace ggs {

constexpr int kPoissonMaxThreshold = 512;     // alias_poisson_threshold is 1..512 (ggs_hip.h)
constexpr int kPoissonAccStride = 16;         // unsigned long long per topic in the totals: one 128-byte line each
constexpr int kPoissonThreads = 1024;         // per workgroup

// X of one cell from its first uniform (c < L) or its Gaussian stream (c >= L)
__device__ __forceinline__ double poisson_search(const double *T, const int n, const double u) {
  int lo = 0, hi = n - 1;                     // T[n - 1] = 1 > u: the answer is in [0, n - 1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (u < T[mid]) hi = mid;
    else lo = mid + 1;
  }
  return (double)lo;
}
__device__ __forceinline__ double poisson_normal(DrawStream &rs, const double lambda) {
  const double g = rs.next_gaussian();
  const double x = floor(sqrt(lambda) * g + lambda + 0.5);
  return x > 0.0 ? x : 0.0;
}
__device__ __forceinline__ double poisson_draw(uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem, int32_t c, int32_t L,
                                               double beta, const double *table, bool &exhausted) {
  DrawStream rs(seed, iteration, purpose, elem);
  if (c < L) return poisson_search(table + (size_t)c * 2 * L, 2 * L, rs.next_double());
  const double x = poisson_normal(rs, beta + (double)c);
  exhausted = rs.exhausted;
  return x;
}

struct PhiPoissonParams {
  const int32_t *cnt;          // [V][cnt_pitch], column j = topic k0 + j
  double *out;                 // [V][out_pitch]: X as fp64 integers
  const double *table;         // [L][2L]
  unsigned long long *acc;     // [Ks][kPoissonAccStride]: [0] sum_v X, [1] sum_v n (zeroed before a draw's first launch)
  uint32_t *status;
  uint64_t seed;
  uint32_t iteration, purpose;
  int32_t Ks, out_pitch, cnt_pitch, k0, V;
  int32_t row_begin, row_end;  // the rows of this launch (with an exchange the draw is cut in two halves of the vocabulary)
  int32_t rows_per_tile;
  int32_t L;
  double beta, t00;            // t00 = T_0[0]
};

// kPoissonThreads per workgroup; a tile = rows_per_tile rows x the Ks topics, walked in row-major order (coalesced reads of
// the counts and writes of X).  A workgroup takes tiles by grid stride and gathers their totals in LDS (X as 64-bit, counts
// as 32-bit integers); they go out with one atomic per topic and workgroup at the end -- integer sums, so neither order is
// visible.  Dynamic LDS: 12 * Ks bytes.  (Measured at config 2: 256-thread workgroups of one tile each, about 2.4 per CU,
// took 98 us; the draw waits on its count loads, so what it needs is waves in flight.)
__global__ __launch_bounds__(kPoissonThreads) void phi_poisson_kernel(PhiPoissonParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned long long *xs = reinterpret_cast<unsigned long long *>(smem);
  uint32_t *ns = reinterpret_cast<uint32_t *>(smem + (size_t)p.Ks * 8);
  const int Ks = p.Ks, tid = threadIdx.x;
  const int rows = p.row_end - p.row_begin;
  const int tiles = (rows + p.rows_per_tile - 1) / p.rows_per_tile;
  const int sdv = kPoissonThreads / Ks, sj = kPoissonThreads - sdv * Ks;   // the thread's step through the tile
  bool exhausted = false;
  for (int j = tid; j < Ks; j += kPoissonThreads) { xs[j] = 0; ns[j] = 0; }
  __syncthreads();
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int v0 = p.row_begin + tile * p.rows_per_tile, nrows = min(p.rows_per_tile, p.row_end - v0);
    int dv = tid / Ks, j = tid - (tid / Ks) * Ks;
    while (dv < nrows) {
      const int v = v0 + dv;
      const int32_t c = p.cnt[(size_t)v * p.cnt_pitch + j];
      const uint64_t e = (uint64_t)(p.k0 + j) * (uint64_t)p.V + (uint64_t)v;
      double x;
      if (c == 0) {
        const U4 o = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), p.purpose << 24, p.iteration, (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        const double u = u53(o.x, o.y);                // DrawStream's first next_double()
        x = u < p.t00 ? 0.0 : poisson_search(p.table, 2 * p.L, u);
      } else if (c < 0) {                              // not a count (the paranoid check names it): no table row to read
        x = 0.0;
        atomicOr(p.status, ST_NEGATIVE_COUNT);
      } else {
        bool ex = false;
        x = poisson_draw(p.seed, p.iteration, p.purpose, e, c, p.L, p.beta, p.table, ex);
        exhausted |= ex;
        atomicAdd(&ns[j], (uint32_t)c);
      }
      p.out[(size_t)v * p.out_pitch + j] = x;
      if (x != 0.0) atomicAdd(&xs[j], (unsigned long long)x);
      j += sj; dv += sdv;
      if (j >= Ks) { j -= Ks; ++dv; }
    }
  }
  __syncthreads();
  for (int jj = tid; jj < Ks; jj += kPoissonThreads) {
    if (xs[jj]) atomicAdd(&p.acc[(size_t)jj * kPoissonAccStride], xs[jj]);
    if (ns[jj]) atomicAdd(&p.acc[(size_t)jj * kPoissonAccStride + 1], (unsigned long long)ns[jj]);
  }
  if (exhausted) atomicOr(p.status, ST_RNG_EXHAUSTED);
}

// the totals as the rest of the Phi phase wants them: tot[j] = sum_v X (fp64: exact below 2^53), n_k[j] = tokensPerTopic
__global__ __launch_bounds__(256) void phi_poisson_totals_kernel(const unsigned long long *acc, int32_t Ks, double *tot, int32_t *n_k) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Ks) return;
  tot[j] = (double)acc[(size_t)j * kPoissonAccStride];
  if (n_k) n_k[j] = (int32_t)acc[(size_t)j * kPoissonAccStride + 1];
}

// ggs_debug_poisson: X of elements elem0 + i with counts[i], through the same functions as the Phi kernel
__global__ void debug_poisson_kernel(uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0, int64_t n, const int32_t *counts,
                                     int32_t L, double beta, const double *table, double t00, int32_t *out, uint32_t *status) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t c = counts[i];
  const uint64_t e = elem0 + (uint64_t)i;
  bool ex = false;
  double x;
  if (c == 0) {
    const U4 o = philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), purpose << 24, iteration, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double u = u53(o.x, o.y);
    x = u < t00 ? 0.0 : poisson_search(table, 2 * L, u);
  } else {
    x = poisson_draw(seed, iteration, purpose, e, c, L, beta, table, ex);
  }
  if (ex) atomicOr(status, ST_RNG_EXHAUSTED);
  out[i] = (int32_t)x;
}

}  // namespace ggs
