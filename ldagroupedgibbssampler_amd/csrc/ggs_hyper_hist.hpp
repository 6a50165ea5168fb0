// ggs_hyper_hist.hpp -- the sufficient statistics of the hyperparameter step (optimizeAlpha / optimizeBeta, MSLDA:812-905) from
// device-resident state: two histograms of COUNTS, a few KB of bins where the host route moves D x K and V x K int32.
//
//   doc_topic_hist_kernel   topicDocCounts (MSLDA:815-845): hist[k][c] = documents with n_dk == c (symmetric: every topic into row 0),
//                           and docLengthCounts (UPLDA:377-432): documents of each length
//   cell_hist_kernel        countHistogram (MSLDA:867-880): hist[c] = cells (w, k) with n_wk == c
//
// Both count only what is NOT zero.  Nearly every (document, topic) pair and most (word, topic) cells are zero, and every one of them
// would be an atomic onto bin 0: the host fills bin 0 as items - sum of the other bins of the row (hist_fill_zero_bins, ggs_host_hyper.hpp),
// in the 32-bit wrap-around arithmetic of the Java int the bin is.  The low bins, which take nearly all increments, are private to a
// workgroup in LDS and flushed once, one global add per non-empty bin; only the tail beyond that table goes straight to global atomics.
// Integer adds: the result does not depend on the order, on the grid, or on the table's size.
//
// A value >= n_bins is never used as an index: it raises HIST_OVERFLOW in *flag and the host answers GGS_ERR_BAD_ARG.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ggs {

constexpr int kHistBlock = 256, kHistWaves = kHistBlock / 64;
constexpr int kHistTabInts = 4096;                     // the workgroup's table of low bins: 16 KiB
constexpr int kHistLenBins = 1024;                     // ... and of document lengths
constexpr uint32_t HIST_OVERFLOW = 1;
constexpr int kHistPerCu = 8;                          // workgroups per CU of the persistent grids at most (the document kernel: what its LDS allows)

// ---- topicDocCounts ------------------------------------------------------------------------------------------------------------
// A wave per document and trip, persistent (launch(), ggs_host_state.hpp).  The wave keeps K int32 counts in LDS, all zero between two
// documents: it adds the document's tokens into them, then walks the tokens a second time (they are in cache) and TAKES each topic's
// count with an exchange against 0 -- the first token of a topic gets n_dk and emits (k, n_dk), the others get 0 -- so a document costs
// O(its length) whatever K is, no D x K array exists, and the counts are zero again for the next document.
struct DocHistParams {
  const int64_t *doc_ptr;
  const int32_t *z;
  uint32_t *hist;            // [rows][n_bins], zeroed
  uint32_t *len_hist;        // [n_bins], zeroed; or null
  uint32_t *flag;
  int64_t num_docs, n_bins;
  int32_t K, rows;           // rows: K, or 1 (symmetric)
  int32_t tab_bins;          // bins [0, tab_bins) of every row are kept in the LDS table: rows * tab_bins <= kHistTabInts
};
inline size_t doc_hist_lds_bytes(int K) { return sizeof(int32_t) * ((size_t)kHistWaves * K + kHistTabInts + kHistLenBins); }
// the table's bins per row: all of them where they fit, none where a row would get fewer than bins 0 and 1
inline int32_t doc_hist_tab_bins(int32_t rows, int64_t n_bins) {
  const int64_t b = n_bins < kHistTabInts / rows ? n_bins : kHistTabInts / rows;
  return b < 2 ? 0 : (int32_t)b;
}

__global__ __launch_bounds__(kHistBlock) void doc_topic_hist_kernel(DocHistParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  int32_t *lds = reinterpret_cast<int32_t *>(smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int K = p.K;
  int32_t *cnt = lds + (size_t)wave * K;
  uint32_t *tab = reinterpret_cast<uint32_t *>(lds + (size_t)kHistWaves * K);
  uint32_t *len_tab = tab + kHistTabInts;
  for (int i = threadIdx.x; i < kHistWaves * K + kHistTabInts + kHistLenBins; i += kHistBlock) lds[i] = 0;
  __syncthreads();
  const int64_t n_bins = p.n_bins;
  const int tab_bins = p.tab_bins;
  for (int64_t d = (int64_t)blockIdx.x * kHistWaves + wave; d < p.num_docs; d += (int64_t)gridDim.x * kHistWaves) {
    const int64_t beg = p.doc_ptr[d], end = p.doc_ptr[d + 1];
    for (int64_t i = beg + lane; i < end; i += 64) {
      const int32_t k = p.z[i];
      if ((uint32_t)k < (uint32_t)K) atomicAdd(&cnt[k], 1);
    }
    // one wave: its LDS operations complete in the order issued; the fences keep the compiler to that order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int64_t i = beg + lane; i < end; i += 64) {
      const int32_t k = p.z[i];
      if ((uint32_t)k >= (uint32_t)K) continue;
      const int64_t c = atomicExch(&cnt[k], 0);
      if (c <= 0) continue;
      const int32_t row = p.rows == 1 ? 0 : k;
      if (c >= n_bins) atomicOr(p.flag, HIST_OVERFLOW);
      else if (c < tab_bins) atomicAdd(&tab[row * tab_bins + (int32_t)c], 1u);
      else atomicAdd(&p.hist[(int64_t)row * n_bins + c], 1u);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane == 0 && p.len_hist) {
      const int64_t len = end - beg;
      if (len >= n_bins) atomicOr(p.flag, HIST_OVERFLOW);
      else if (len < kHistLenBins) atomicAdd(&len_tab[len], 1u);
      else atomicAdd(&p.len_hist[len], 1u);
    }
  }
  __syncthreads();
  // the flush: one global add per non-empty bin of the workgroup's tables
  const int tab_n = p.rows * tab_bins;
  for (int i = threadIdx.x; i < tab_n; i += kHistBlock) {
    const uint32_t v = tab[i];
    if (v) atomicAdd(&p.hist[(int64_t)(i / tab_bins) * n_bins + (i % tab_bins)], v);
  }
  if (p.len_hist)
    for (int i = threadIdx.x; i < kHistLenBins; i += kHistBlock) {
      const uint32_t v = len_tab[i];
      if (v) atomicAdd(&p.len_hist[i], v);             // i < n_bins: only such lengths were added
    }
}

// ---- countHistogram ------------------------------------------------------------------------------------------------------------
// A pure stream over the int32 [V][K] counts in 16-byte loads, persistent and grid-strided.  The counts 1, 2 and 3 -- most of the
// non-zero cells -- are counted in registers and added to the workgroup's LDS table once per wave at the end; the other counts below
// kHistTabInts go to the table as they come, the tail to global atomics.
struct CellHistParams {
  const int32_t *n_wk;
  uint32_t *hist;            // [n_bins], zeroed
  uint32_t *flag;
  int64_t n, n_bins;         // n = V * K cells
};
constexpr int kCellHistLdsBytes = kHistTabInts * (int)sizeof(uint32_t);
constexpr int kCellHistPerLane = 4 * 4;                // cells of a lane per work item: four 16-byte loads in flight

__device__ __forceinline__ void cell_hist_one(int32_t c, uint32_t &n1, uint32_t &n2, uint32_t &n3, uint32_t *tab, const CellHistParams &p) {
  if (c <= 0) return;
  if (c == 1) ++n1;
  else if (c == 2) ++n2;
  else if (c == 3) ++n3;
  else if (c >= p.n_bins) atomicOr(p.flag, HIST_OVERFLOW);
  else if (c < kHistTabInts) atomicAdd(&tab[c], 1u);
  else atomicAdd(&p.hist[c], 1u);
}

__global__ __launch_bounds__(kHistBlock) void cell_hist_kernel(CellHistParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  uint32_t *tab = reinterpret_cast<uint32_t *>(smem);
  for (int i = threadIdx.x; i < kHistTabInts; i += kHistBlock) tab[i] = 0;
  __syncthreads();
  uint32_t n1 = 0, n2 = 0, n3 = 0;
  const int64_t quads = p.n / 4, stride = (int64_t)gridDim.x * kHistBlock;
  const int4 *src = reinterpret_cast<const int4 *>(p.n_wk);
  int64_t q = (int64_t)blockIdx.x * kHistBlock + threadIdx.x;
  for (; q + 3 * stride < quads; q += 4 * stride) {
    const int4 a = src[q], b = src[q + stride], c = src[q + 2 * stride], e = src[q + 3 * stride];
    cell_hist_one(a.x, n1, n2, n3, tab, p); cell_hist_one(a.y, n1, n2, n3, tab, p); cell_hist_one(a.z, n1, n2, n3, tab, p); cell_hist_one(a.w, n1, n2, n3, tab, p);
    cell_hist_one(b.x, n1, n2, n3, tab, p); cell_hist_one(b.y, n1, n2, n3, tab, p); cell_hist_one(b.z, n1, n2, n3, tab, p); cell_hist_one(b.w, n1, n2, n3, tab, p);
    cell_hist_one(c.x, n1, n2, n3, tab, p); cell_hist_one(c.y, n1, n2, n3, tab, p); cell_hist_one(c.z, n1, n2, n3, tab, p); cell_hist_one(c.w, n1, n2, n3, tab, p);
    cell_hist_one(e.x, n1, n2, n3, tab, p); cell_hist_one(e.y, n1, n2, n3, tab, p); cell_hist_one(e.z, n1, n2, n3, tab, p); cell_hist_one(e.w, n1, n2, n3, tab, p);
  }
  for (; q < quads; q += stride) {
    const int4 a = src[q];
    cell_hist_one(a.x, n1, n2, n3, tab, p); cell_hist_one(a.y, n1, n2, n3, tab, p); cell_hist_one(a.z, n1, n2, n3, tab, p); cell_hist_one(a.w, n1, n2, n3, tab, p);
  }
  if (blockIdx.x == 0 && (int64_t)threadIdx.x < p.n - quads * 4) cell_hist_one(p.n_wk[quads * 4 + threadIdx.x], n1, n2, n3, tab, p);   // V * K is no multiple of 4
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { n1 += __shfl_down(n1, d); n2 += __shfl_down(n2, d); n3 += __shfl_down(n3, d); }
  if ((threadIdx.x & 63) == 0) {                       // p.n_bins > 3 or not: the table has the bins, the flush checks the range
    if (n1) atomicAdd(&tab[1], n1);
    if (n2) atomicAdd(&tab[2], n2);
    if (n3) atomicAdd(&tab[3], n3);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kHistTabInts; i += kHistBlock) {
    const uint32_t v = tab[i];
    if (!v) continue;
    if (i >= p.n_bins) atomicOr(p.flag, HIST_OVERFLOW);
    else atomicAdd(&p.hist[i], v);
  }
}

}  // namespace ggs
