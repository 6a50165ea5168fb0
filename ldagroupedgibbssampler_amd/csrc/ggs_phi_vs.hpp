// ggs_phi_vs.hpp -- scheme=nzvsspalias: the indicator chain of the variable-selection Dirichlet
// (VSDirichlet.nextDistribution, types/VSDirichlet.java:34-89, under NZVSSpaliasUncollapsedParallelLDA.loopOverTopics).
//
// Per topic k the reference walks the V cells in index order.  It carries s (zeroPhi), the number of zeros of the row so
// far: s0 = #{v : prevPhi[k][v] == 0.0}.  A cell with a count is drawn and leaves s alone.  A cell without one is kept or
// dropped by a Bernoulli indicator with
//   a = s * beta,  r = exp(lgS(a + beta) + lgS(a + n_k) - lgS(a + beta + n_k) - lgS(a)) * (pi / (1 - pi)),  p = r / (1 + r)
// (calculateIndicatorProbIsOne, :102-112; lgS = log_gamma_stirling, exp = strict_exp, n_k the topic's int token count):
// U > p leaves the cell UNDRAWN (+0.0; s++ if prevPhi != 0.0), otherwise it is drawn (s-- if prevPhi == 0.0).  U is the
// first uniform of the Philox stream (GGS_PURPOSE_VS, element k * V + v).  At s == 0 with n_k > 0, lgS(0) = +inf makes
// r = 0 and p = 0; with n_k == 0 p is NaN, U > NaN is false and the cell is drawn.  p > 1 or p < 0 (the reference throws)
// raises ST_INVARIANT.
//
// That is V sequential steps per topic.  The chain is CAUSAL -- cell v's s depends on the decisions before v only -- so it
// is solved by rounds, a workgroup per topic:
//   vs_bits_kernel   two bit rows per topic, count == 0 and prevPhi == 0.0, V bits each, from the by-word matrices
//                    n_wk [V][pitch] and phiT [V][Kp]: lane = topic, so every row read is coalesced and nothing is gathered
//                    down a column;
//   vs_chain_kernel  keeps s at the START of every 32-cell word (sw[j]; s0 everywhere before the first round).  A round:
//                    every word is walked cell by cell from sw[j] (a thread per word: inside the word the walk IS the
//                    reference's), leaving its decisions and its net step; an exclusive block scan of the steps gives the
//                    new sw.  Rounds repeat until one changes no decision and no sw[j].
//                    Exact, not approximate: word 0 starts from s0 in every round, so it is right after round 1; if the
//                    words before j are right after round t, sw[j] is right after it and word j after round t + 1.  A round
//                    that changes nothing has reproduced itself from starts that are the prefix sums of its own steps:
//                    that is the sequential chain.  Each round settles at least the first unsettled cell without a count,
//                    so there are at most (cells without a count) + 1 rounds; p moves by about 1e-6 per step of s, so in
//                    practice a handful.  Nothing is decided from a bracket of p: the computed p is not proved monotone.
//                    p(s) is looked up in a table over the window of s the round's starts span (filled by the same
//                    function, so the same bits) and computed on the spot outside it.
//                    The rows live in LDS; a row that does not fit (V > kVsLdsMaxV) runs the same rounds over global
//                    scratch (GGS_DEBUG_VS_GLOBAL=1 forces that).
//   vs_mask_kernel   the undrawn cells from bit rows by topic into zero_mask's layout, a bit per topic, by word
//                    (phi_gamma_vs_kernel and word_list_mask_kernel read it).
#pragma once
#include "ggs_kernels.hpp"
#include "ggs_loglik.hpp"

namespace ggs {

__device__ __forceinline__ double vs_probability(const int32_t s, const int32_t n_k, const double beta, const double odds) {
  const double a = (double)s * beta, nk = (double)n_k;
  const double l_a = log_gamma_stirling(a), l_ab = log_gamma_stirling(a + beta), l_an = log_gamma_stirling(a + nk),
               l_abn = log_gamma_stirling(a + beta + nk);
  const double r = strict_exp(l_ab + l_an - l_abn - l_a) * odds;
  return r / (1.0 + r);
}
__device__ __forceinline__ double vs_uniform(const uint64_t elem, const uint32_t iteration, const uint64_t seed) {
  const U4 o = philox4x32_10((uint32_t)elem, (uint32_t)(elem >> 32), (uint32_t)GGS_PURPOSE_VS << 24, iteration, (uint32_t)seed, (uint32_t)(seed >> 32));
  return u53(o.x, o.y);
}

// ---- the bit rows ----------------------------------------------------------------------------------------------------
struct VsBitsParams {
  const int32_t *cnt;          // [V][cnt_pitch], column j = topic k0 + j
  const double *phiT;          // [V][Kp], all K topics: the previous Phi
  uint32_t *cz, *pz;           // [Ks][W]: bit v & 31 of word v >> 5 = count == 0, prevPhi == 0.0; bits past V are 0
  int32_t cnt_pitch, Kp, k0, Ks, V, W;
};
__global__ __launch_bounds__(64) void vs_bits_kernel(VsBitsParams p) {
  const int lane = threadIdx.x, ncg = (p.Ks + 63) / 64;
  const int64_t items = (int64_t)p.W * ncg;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int j = (int)(it / ncg), k = (int)(it - (int64_t)j * ncg) * 64 + lane;
    if (k >= p.Ks) continue;
    uint32_t wc = 0, wp = 0;
    const int rows = min(32, p.V - j * 32);
    for (int b = 0; b < rows; ++b) {
      const size_t v = (size_t)j * 32 + b;
      wc |= (uint32_t)(p.cnt[v * p.cnt_pitch + k] == 0) << b;
      wp |= (uint32_t)(p.phiT[v * p.Kp + p.k0 + k] == 0.0) << b;
    }
    p.cz[(size_t)k * p.W + j] = wc;
    p.pz[(size_t)k * p.W + j] = wp;
  }
}

// ---- the chain -------------------------------------------------------------------------------------------------------
struct VsChainParams {
  const uint32_t *cz, *pz;     // [Ks][W]
  uint32_t *und;               // [Ks][W] out: the undrawn cells
  int32_t *work;               // GLOBAL only: [Ks][2][W], the word starts and the words' steps
  const int32_t *n_k;          // [Ks]
  const double *u;             // [Ks][V] the uniforms to use in place of Philox, or null (ggs_debug_vs_indicators)
  int32_t *s_end, *rounds;     // [Ks]
  uint32_t *status;
  uint64_t seed;
  uint32_t iteration;
  int32_t Ks, k0, V, W;
  double beta, odds;           // odds = pi / (1 - pi)
};
constexpr int kVsBlock = 256, kVsTab = 1024;
constexpr int kVsLdsMaxV = 32 * ((48 * 1024) / 20);                              // five words of LDS per 32 cells, 48 KiB
inline size_t vs_chain_lds_bytes(int W) { return (size_t)W * 20; }

template <bool GLOBAL>
__global__ __launch_bounds__(kVsBlock) void vs_chain_kernel(VsChainParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  __shared__ double ptab[kVsTab];
  __shared__ int32_t part[kVsBlock];
  __shared__ int32_t changed, bad, s_min, s_max, s_total;
  const int tid = threadIdx.x, k = blockIdx.x, W = p.W;
  const uint32_t *cz, *pz;
  uint32_t *und;
  int32_t *sw, *dl;
  if constexpr (GLOBAL) {
    cz = p.cz + (size_t)k * W; pz = p.pz + (size_t)k * W; und = p.und + (size_t)k * W;
    sw = p.work + (size_t)k * 2 * W; dl = sw + W;
  } else {
    uint32_t *l = reinterpret_cast<uint32_t *>(smem);
    for (int j = tid; j < W; j += kVsBlock) { l[j] = p.cz[(size_t)k * W + j]; l[W + j] = p.pz[(size_t)k * W + j]; }
    cz = l; pz = l + W; und = l + 2 * W;
    sw = reinterpret_cast<int32_t *>(l + 3 * W); dl = sw + W;
  }
  // s0 = the zeros of the previous row
  int32_t z = 0;
  for (int j = tid; j < W; j += kVsBlock) z += __popc(p.pz[(size_t)k * W + j]);
  if (tid == 0) s_total = 0;
  __syncthreads();
  if (z) atomicAdd(&s_total, z);
  __syncthreads();
  const int32_t s0 = s_total, n_k = p.n_k[k];
  for (int j = tid; j < W; j += kVsBlock) { sw[j] = s0; und[j] = 0u; }
  if (tid == 0) { s_min = s0; s_max = s0; }
  __syncthreads();

  const uint64_t elem0 = (uint64_t)(p.k0 + k) * (uint64_t)p.V;
  const int per = (W + kVsBlock - 1) / kVsBlock, j0 = min(tid * per, W), j1 = min(j0 + per, W);
  int32_t round = 0, s_last = s0;
  for (;;) {
    // p over the window of s this round's words can reach: their starts, and 32 steps either way inside a word
    const int32_t w0 = max(0, s_min - 32), tn = min(kVsTab, s_max + 32 - w0 + 1);
    for (int i = tid; i < tn; i += kVsBlock) ptab[i] = vs_probability(w0 + i, n_k, p.beta, p.odds);
    if (tid == 0) { changed = 0; bad = 0; }
    __syncthreads();
    bool ch = false, bd = false;
    for (int j = tid; j < W; j += kVsBlock) {
      const uint32_t pzw = pz[j];
      int32_t s = sw[j], d = 0;
      uint32_t un = 0;
      for (uint32_t bits = cz[j]; bits; bits &= bits - 1) {
        const int b = __ffs((int)bits) - 1;
        const uint64_t v = (uint64_t)j * 32 + (uint64_t)b;
        const double U = p.u ? p.u[(size_t)k * p.V + v] : vs_uniform(elem0 + v, p.iteration, p.seed);
        const uint32_t ti = (uint32_t)(s - w0);
        const double pr = ti < (uint32_t)tn ? ptab[ti] : vs_probability(s, n_k, p.beta, p.odds);
        bd |= pr > 1.0 || pr < 0.0;
        const bool prev_zero = (pzw >> b) & 1u;
        if (U > pr) { un |= 1u << b; if (!prev_zero) { s += 1; d += 1; } }
        else if (prev_zero) { s -= 1; d -= 1; }
      }
      ch |= un != und[j];
      und[j] = un; dl[j] = d;
    }
    if (ch) changed = 1;
    if (bd) bad = 1;
    __syncthreads();
    // the words' new starts: s0 + the exclusive scan of their steps
    int32_t sum = 0;
    for (int j = j0; j < j1; ++j) sum += dl[j];
    part[tid] = sum;
    if (tid == 0) { s_min = INT32_MAX; s_max = INT32_MIN; }
    __syncthreads();
    if (tid == 0) {
      int32_t run = s0;
      for (int i = 0; i < kVsBlock; ++i) { const int32_t x = part[i]; part[i] = run; run += x; }
      s_total = run;
    }
    __syncthreads();
    int32_t run = part[tid], lo = INT32_MAX, hi = INT32_MIN;
    ch = false;
    for (int j = j0; j < j1; ++j) {
      ch |= sw[j] != run;
      sw[j] = run;
      lo = min(lo, run); hi = max(hi, run);
      run += dl[j];
    }
    if (ch) changed = 1;
    if (j1 > j0) { atomicMin(&s_min, lo); atomicMax(&s_max, hi); }
    __syncthreads();
    round += 1;
    s_last = s_total;
    const bool done = !changed, runaway = round > p.V + 2;                       // the proof's bound is (cells without a count) + 1
    const bool was_bad = bad != 0;
    __syncthreads();                                                             // the flags are reset at the head of the next round
    if (done || runaway) {
      if (tid == 0 && (was_bad || runaway)) atomicOr(p.status, ST_INVARIANT);
      break;
    }
  }
  if constexpr (!GLOBAL)
    for (int j = tid; j < W; j += kVsBlock) p.und[(size_t)k * W + j] = und[j];
  if (tid == 0) { p.s_end[k] = s_last; p.rounds[k] = round; }
}

// ---- bit rows by topic -> zero_mask's layout ---------------------------------------------------------------------------
// mask [V][pitch]: bit kg & 31 of mask[v * pitch + (kg >> 5)] set = cell (kg, v) is undrawn; the topics of the slice
// [k0, k0 + Ks) only, every other bit 0.
__global__ __launch_bounds__(256) void vs_mask_kernel(const uint32_t *und, int32_t W, int32_t k0, int32_t Ks, int32_t V, int32_t pitch, uint32_t *mask) {
  const int64_t n = (int64_t)V * pitch, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int v = (int)(i / pitch), m = (int)(i - (int64_t)v * pitch);
    uint32_t word = 0;
    for (int b = 0; b < 32; ++b) {
      const int k = m * 32 + b - k0;
      if (k >= 0 && k < Ks) word |= ((und[(size_t)k * W + (v >> 5)] >> (v & 31)) & 1u) << b;
    }
    mask[i] = word;
  }
}

// ggs_get_vs_stats: the cells of phiT [V][Kp] that are exactly 0.0
__global__ __launch_bounds__(256) void vs_zero_cells_kernel(const double *phiT, int32_t K, int32_t Kp, int32_t V, unsigned long long *out) {
  const int64_t n = (int64_t)V * K, stride = (int64_t)gridDim.x * 256;
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const int v = (int)(i / K), k = (int)(i - (int64_t)v * K);
    c += phiT[(size_t)v * Kp + k] == 0.0;
  }
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}

}  // namespace ggs
