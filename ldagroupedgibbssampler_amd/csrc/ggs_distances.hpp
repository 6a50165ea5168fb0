// ggs_distances.hpp -- the document and topic distances of the diagnostics loop ("Quantity A" and "Quantity B",
// UPLDA:723-753 and :778-806; the same loops in SerialCollapsedLDA.java:221-305 and ADLDA.java:414 ff.):
//   min_doc_distances.csv    per document d:  min over dd != d of sqrt(sum_k (theta[d][k] - theta[dd][k])^2)
//   min_topic_distances.csv  min over i > j of sqrt(sum_v (phi[i][v] - phi[j][v])^2)
//
// What "the same number" means ("distances"): per pair s = 0.0, then for k in index order t = a[k] - b[k],
// s = s + t * t with the product and the sum rounded separately (never an FMA: __dmul_rn / __dadd_rn, and the unit is built
// with -ffp-contract=off), dist = sqrt(s), and the minimum starts at 1e20 and is replaced only when dist < min.  sqrt is
// correctly rounded, hence monotone: min over partners of sqrt(s) == sqrt(min over partners of s) bit for bit, so the kernels
// keep the minimum of the SUMS and take one square root per output.  A NaN sum never replaces a minimum (NaN < x is false).
// (a - b)^2 and (b - a)^2 are the same double, so the document side computes each unordered pair once.
//
// One tile body serves both sides.  A workgroup of 256 lanes (16 x 16) owns a tile of T = 16 * R rows x T partner rows; a
// lane owns R x R pairs, rows ty + 16 * i against partners tx + 16 * j, one fp64 accumulator each.  The index k runs in
// chunks of KC, staged through LDS k-major ([KC][T + 1]): per k a lane reads R row values (4 distinct addresses per
// wave: broadcasts) and R partner values (16 consecutive doubles per lane group: conflict-free) with ds_read_b64.  Every
// accumulator receives its addends strictly in index order -- that is the whole exactness argument; there is no running
// sum trickery and no replay path.  Any length works: nothing but one chunk is ever in LDS.
//   min_row_dist_kernel    rows are row-major [n][len] (theta [D][K]); R = 4 (T = 64), KC = 32.  The transposing store into
//                          LDS has stride T + 1 doubles (odd: 2-way conflicts at most).
//   min_topic_dist_kernel  rows are element-major [len][pitch] (phiT [V][Kp] as it lies); R = 1 (T = 16: K (K - 1) / 2 lanes,
//                          one pair each, fill the machine at K = 1024), KC = 192 so that a chunk's load latency is paid
//                          once per 192 serial steps (51 KiB of static LDS).
// `diag` (partners == rows): the pair (d, d) is skipped, only tiles on and above the diagonal work, and a tile above it
// feeds the minima of its rows AND of its columns.  Per-row minima are reduced across the 16 lanes that share a row, then
// merged by a vector atomicMin on the 64-bit pattern of the non-negative sum into a buffer preset to the pattern of +inf:
// non-negative doubles order as unsigned integers and every NaN pattern lies above +inf, so NaN loses by itself.
// min_dist_finish_kernel writes min(1e20, sqrt(min_sq)), and 1e20 where nothing was merged.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ggs {

constexpr int kDistBlock = 256;                          // 16 x 16 lanes
constexpr int kDistRowR = 4, kDistRowKC = 32;            // document side: tile edge 64
constexpr int kDistTopR = 1, kDistTopKC = 192;           // topic side: tile edge 16
constexpr unsigned long long kDistInfBits = 0x7ff0000000000000ull;
constexpr double kDistNoPartner = 1e+20;                 // the reference's initial minimum

constexpr int dist_tile_edge(int R) { return 16 * R; }
constexpr int dist_lds_bytes(int R, int KC) { return 2 * KC * (dist_tile_edge(R) + 1) * (int)sizeof(double); }

// `a < b` on doubles known to be non-negative or NaN, NaN never winning
__device__ __forceinline__ double dist_min(double cur, double v) { return v < cur ? v : cur; }

template <int R, int KC, bool ELEM_MAJOR>
__device__ __forceinline__ void min_dist_tile(const double *__restrict__ A, int64_t n, int64_t pitch_a, const double *__restrict__ B, int64_t m, int64_t pitch_b,
                                              int64_t len, int diag, int64_t tile0, int64_t tiles_b, unsigned long long *__restrict__ min_bits, double *lds) {
  constexpr int T = 16 * R, LD = T + 1;
  double *As = lds, *Bs = lds + KC * LD;
  const int64_t tile = tile0 + blockIdx.x;
  const int64_t ti = tile / tiles_b, tj = tile - ti * tiles_b;
  if (diag && tj < ti) return;                           // uniform per workgroup: before any barrier
  const int64_t r0 = ti * T, c0 = tj * T;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

  double acc[R][R];
#pragma unroll
  for (int i = 0; i < R; ++i)
#pragma unroll
    for (int j = 0; j < R; ++j) acc[i][j] = 0.0;

  for (int64_t k0 = 0; k0 < len; k0 += KC) {
    const int kn = (int)(len - k0 < KC ? len - k0 : KC);
    // stage the chunk k-major; rows past the end read as 0.0 and are masked at the merge
    if (ELEM_MAJOR) {
      for (int e = tid; e < kn * T; e += kDistBlock) {
        const int kk = e / T, r = e - kk * T;
        As[kk * LD + r] = r0 + r < n ? A[(k0 + kk) * pitch_a + r0 + r] : 0.0;
        Bs[kk * LD + r] = c0 + r < m ? B[(k0 + kk) * pitch_b + c0 + r] : 0.0;
      }
    } else {
      for (int e = tid; e < KC * T; e += kDistBlock) {
        const int r = e / KC, kk = e - r * KC;
        if (kk < kn) {
          As[kk * LD + r] = r0 + r < n ? A[(r0 + r) * pitch_a + k0 + kk] : 0.0;
          Bs[kk * LD + r] = c0 + r < m ? B[(c0 + r) * pitch_b + k0 + kk] : 0.0;
        }
      }
    }
    __syncthreads();
    if (kn == KC) {
#pragma unroll 8
      for (int kk = 0; kk < KC; ++kk) {
        double a[R], b[R];
#pragma unroll
        for (int i = 0; i < R; ++i) a[i] = As[kk * LD + ty + 16 * i];
#pragma unroll
        for (int j = 0; j < R; ++j) b[j] = Bs[kk * LD + tx + 16 * j];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const double t = __dsub_rn(a[i], b[j]);
            acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(t, t));
          }
      }
    } else {
      for (int kk = 0; kk < kn; ++kk) {
        double a[R], b[R];
#pragma unroll
        for (int i = 0; i < R; ++i) a[i] = As[kk * LD + ty + 16 * i];
#pragma unroll
        for (int j = 0; j < R; ++j) b[j] = Bs[kk * LD + tx + 16 * j];
#pragma unroll
        for (int i = 0; i < R; ++i)
#pragma unroll
          for (int j = 0; j < R; ++j) {
            const double t = __dsub_rn(a[i], b[j]);
            acc[i][j] = __dadd_rn(acc[i][j], __dmul_rn(t, t));
          }
      }
    }
    __syncthreads();
  }

  const double inf = __longlong_as_double((long long)kDistInfBits);
  // rows: the 16 lanes of one ty (lanes 16 q .. 16 q + 15 of a wave) hold one row's partners
#pragma unroll
  for (int i = 0; i < R; ++i) {
    const int64_t r = r0 + ty + 16 * i;
    double v = inf;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t c = c0 + tx + 16 * j;
      if (c < m && !(diag && c == r)) v = dist_min(v, acc[i][j]);
    }
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) v = dist_min(v, __shfl_xor(v, o, 64));
    if (tx == 0 && r < n && v < inf) atomicMin(min_bits + r, (unsigned long long)__double_as_longlong(v));
  }
  // columns of a tile above the diagonal: the same sums seen from the partner's side
  if (diag && tj > ti) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const int64_t c = c0 + tx + 16 * j;
      double v = inf;
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int64_t r = r0 + ty + 16 * i;
        if (r < n) v = dist_min(v, acc[i][j]);
      }
      v = dist_min(v, __shfl_xor(v, 16, 64));
      v = dist_min(v, __shfl_xor(v, 32, 64));
      if ((tid & 63) < 16 && c < m && v < inf) atomicMin(min_bits + c, (unsigned long long)__double_as_longlong(v));
    }
  }
}

// A [n][len], B [m][len], row-major; tile = tile0 + blockIdx.x over [ceil(n / 64)][tiles_b]
__global__ __launch_bounds__(kDistBlock) void min_row_dist_kernel(const double *__restrict__ A, int64_t n, const double *__restrict__ B, int64_t m, int64_t len, int diag,
                                                                  int64_t tile0, int64_t tiles_b, unsigned long long *__restrict__ min_bits) {
  __shared__ double lds[dist_lds_bytes(kDistRowR, kDistRowKC) / sizeof(double)];
  min_dist_tile<kDistRowR, kDistRowKC, false>(A, n, len, B, m, len, len, diag, tile0, tiles_b, min_bits, lds);
}

// A [len][pitch], its first n columns the rows; always against itself, the diagonal skipped
__global__ __launch_bounds__(kDistBlock) void min_topic_dist_kernel(const double *__restrict__ A, int64_t n, int64_t pitch, int64_t len, int64_t tile0, int64_t tiles_b,
                                                                    unsigned long long *__restrict__ min_bits) {
  __shared__ double lds[dist_lds_bytes(kDistTopR, kDistTopKC) / sizeof(double)];
  min_dist_tile<kDistTopR, kDistTopKC, true>(A, n, pitch, A, n, pitch, len, 1, tile0, tiles_b, min_bits, lds);
}

__global__ void min_dist_preset_kernel(unsigned long long *min_bits, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) min_bits[i] = kDistInfBits;
}

// dist = min(1e20, sqrt(min_sq)): `sqrt(s) < 1e20` is the reference's replacement test against its initial minimum
__device__ __forceinline__ double dist_of_bits(unsigned long long bits) {
  if (bits >= kDistInfBits) return kDistNoPartner;
  const double d = sqrt(__longlong_as_double((long long)bits));
  return d < kDistNoPartner ? d : kDistNoPartner;
}

// min_dist [n]; min_sq [n] or null: the minimal sums themselves, +inf where nothing was merged
__global__ void min_dist_finish_kernel(const unsigned long long *__restrict__ min_bits, int64_t n, double *__restrict__ min_dist, double *__restrict__ min_sq) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned long long b = min_bits[i];
    min_dist[i] = dist_of_bits(b);
    if (min_sq) min_sq[i] = __longlong_as_double((long long)b);
  }
}

// *out = the distance of the smallest of the n per-row minima (one workgroup; the block minima meet in one LDS cell)
__global__ __launch_bounds__(kDistBlock) void min_dist_reduce_kernel(const unsigned long long *__restrict__ min_bits, int64_t n, double *__restrict__ out) {
  __shared__ unsigned long long cell;
  if (threadIdx.x == 0) cell = kDistInfBits;
  __syncthreads();
  unsigned long long v = kDistInfBits;
  for (int64_t i = threadIdx.x; i < n; i += kDistBlock) { const unsigned long long b = min_bits[i]; v = b < v ? b : v; }
  if (v < kDistInfBits) atomicMin(&cell, v);
  __syncthreads();
  if (threadIdx.x == 0) *out = dist_of_bits(cell);
}

}  // namespace ggs
