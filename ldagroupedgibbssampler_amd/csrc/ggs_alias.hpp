// ggs_alias.hpp -- scheme=spalias: the per-word Walker alias tables of the conditional's "prior" part,
// pi[k] = phi[k][w] * alpha[k] (SpaliasUncollapsedParallelLDA.java:39-60; the build is reGenerateAliasTable of
// util/OptimizedGentleAliasMethod.java).  Rebuilt whenever Phi changes, read by the z step of ggs_z_spalias.hpp.
//
// Per word: typeNorm = the k-order sum of pi from 0.0; bs[k] = pi[k] / typeNorm - 1.0 / K; k goes on the `lows` stack
// if bs[k] < 0.0, else on `highs`, both in k order; then, while both stacks hold something: pop l from lows, peek h on
// highs, c = bs[l], d = bs[h], bs[h] = c + d, pop highs if bs[h] <= 0, push h on lows if bs[h] < 0, a[l] = h,
// ps[l] = 1.0 + (double)K * c.  Every entry the loop never pairs keeps a[k] = k, ps[k] = 1.0 (ours: Java leaves ps[k]
// stale there; such an entry has a[k] = k, so no draw can tell).  A column that underflowed as a whole (typeNorm == 0)
// makes every bs NaN: all k land on highs, the table is the identity, and the z step never reads it.
//
// The pairing loop is a serial chain of at most K steps per word in which every step depends on the one before (bs[h]
// carries over), and the words are independent: V chains.  A chain runs on ONE LANE, out of LDS:
//   bs   fp64 [K]   -- pi, then bs in place; the slot of a popped l is dead (l never returns to a stack) and takes ps[l]
//   al   u16  [K]   -- the alias, preset to k
//   st   u16  [K]   -- BOTH stacks: lows grow up from 0, highs down from K (they hold K entries at the start and never
//                      more: a push on lows only ever follows a pop of highs)
// 12 bytes per topic and word.  A single-wave workgroup takes `wpb` words at a time (as many as fit 48 KiB, at most 64):
// all 64 lanes fill pi (coalesced: consecutive words' phiT rows), lanes 0..wpb-1 each sum their word's column in k order,
// all lanes form bs, lanes 0..wpb-1 fill the stacks and run the chains, all lanes write ps / a out (coalesced).  At
// K = 1024 four chains run per wave and thirteen waves fit a CU; at K = 4096 one chain per wave, three waves per CU.
// The chain is LDS-latency bound: three dependent LDS operations per step (the stack entry, bs of it, the store).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ggs {

struct AliasParams {
  const double *phiT;          // [V][Kp]
  const double *alpha;         // [K]
  double *ps;                  // [V][K]
  int32_t *a;                  // [V][K]
  double *type_norm;           // [V]
  int32_t V, K, Kp, wpb;
};

constexpr int kAliasLdsBudget = 48 * 1024;
inline int alias_words_per_block(int K) { return std::max(1, std::min(64, kAliasLdsBudget / (12 * K))); }
inline size_t alias_lds_bytes(int K, int wpb) { return (size_t)wpb * K * 12 + 64 * sizeof(double); }

// One word's pairing chain over n entries, on one lane, out of LDS: b [n] holds bs and takes ps[l] in the slot of every paired
// l, aw [n] the alias (preset to the index), s [n] both stacks.  n = K for the tables over Phi (alias_build_kernel), n = the
// word's number of non-zero topics for the tables over the counts (count_alias_build_kernel, at the end of this file).
__device__ __forceinline__ void alias_pairing_chain(double *b, uint16_t *s, uint16_t *aw, const int n) {
  int nl = 0, hp = n;                                                              // lows: s[0, nl), top s[nl - 1]; highs: s[hp, n), top s[hp]
  for (int k = 0; k < n; ++k) {
    if (b[k] < 0.0) s[nl++] = (uint16_t)k;
    else s[--hp] = (uint16_t)k;
  }
  if (nl > 0 && hp < n) {
    int h = s[hp];
    double d = b[h];
    while (true) {
      const int l = s[--nl];
      const double c = b[l];
      b[l] = 1.0 + (double)n * c;                                                  // ps[l]
      aw[l] = (uint16_t)h;
      d = c + d;
      if (d <= 0.0) {                                                              // highs loses h ...
        ++hp;
        if (d < 0.0) s[nl++] = (uint16_t)h;                                        // ... and lows takes it
        b[h] = d;
        if (nl == 0 || hp == n) break;
        h = s[hp];
        d = b[h];
      } else if (nl == 0) {
        b[h] = d;
        break;
      }
    }
  }
}

__global__ __launch_bounds__(64) void alias_build_kernel(AliasParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int K = p.K, wpb = p.wpb, lane = threadIdx.x;
  double *bs = reinterpret_cast<double *>(smem);                                   // [wpb][K]
  double *tnl = bs + (size_t)wpb * K;                                              // [64]
  uint16_t *al = reinterpret_cast<uint16_t *>(tnl + 64);                           // [wpb][K]
  uint16_t *st = al + (size_t)wpb * K;                                             // [wpb][K]
  const double inv_k = 1.0 / (double)K;

  for (int w0 = blockIdx.x * wpb; w0 < p.V; w0 += gridDim.x * wpb) {
    const int nw = min(wpb, p.V - w0), cells = nw * K;
    __syncthreads();
    for (int idx = lane; idx < cells; idx += 64) {
      const int wi = idx / K, k = idx - wi * K;
      bs[idx] = p.phiT[(size_t)(w0 + wi) * p.Kp + k] * p.alpha[k];
      al[idx] = (uint16_t)k;
    }
    __syncthreads();
    if (lane < nw) {
      const double *b = bs + (size_t)lane * K;
      double tn = 0.0;
      for (int k = 0; k < K; ++k) tn += b[k];
      tnl[lane] = tn;
      p.type_norm[w0 + lane] = tn;
    }
    __syncthreads();
    for (int idx = lane; idx < cells; idx += 64) bs[idx] = bs[idx] / tnl[idx / K] - inv_k;
    __syncthreads();
    if (lane < nw) alias_pairing_chain(bs + (size_t)lane * K, st + (size_t)lane * K, al + (size_t)lane * K, K);
    __syncthreads();
    for (int idx = lane; idx < cells; idx += 64) {
      const int wi = idx / K, k = idx - wi * K, av = al[idx];
      const size_t o = (size_t)w0 * K + idx;
      p.ps[o] = av == k ? 1.0 : bs[idx];
      p.a[o] = av;
    }
  }
}

// ---- the words' lists and tables over the counts (scheme=lightcollapsed, lightpcldaw2) -------------------------------------
// TypeTopicParallelTableBuilder.java:38-51 over the ascending list L of the word's topics with n_wk > 0:
// p_i = n_w,L[i] / topicCountBetaHat[L[i]], typeMass = the i-order sum from 0.0, then reGenerateAliasTable
// (OptimizedGentleAliasMethodDynamicSize.java:55-82) with k = nnz: bs[i] = p_i / typeMass - 1.0 / nnz and the lows / highs
// pairing chain above.  A single-wave workgroup takes `wpb` words at a time, as alias_build_kernel does: the
// whole wave makes each word's list (a ballot and a prefix popcount per block of 64 topics, as word_list_build_kernel) and
// fills p into LDS, lanes 0..wpb-1 each sum their word's p in i order and run its chain out of LDS, all lanes write out.
// Only the first nnz entries of a row of ps / a / nzw are written; a word without tokens writes nw = 0 and nothing else.
struct CountAliasParams {
  const int32_t *n_wk;         // [V][K] corpus-wide sweep-start counts
  const int32_t *n_k;          // [K]
  double *ps;                  // [V][K]
  int32_t *a;                  // [V][K]
  double *type_norm;           // [V] typeMass
  uint16_t *nzw;               // [V][K]
  int32_t *nw;                 // [V]
  int32_t *tpt;                // [V] tokensPerType
  double beta_sum;
  int32_t V, K, wpb;
};

inline size_t count_alias_lds_bytes(int K, int wpb) { return alias_lds_bytes(K, wpb) + 64 * sizeof(int32_t); }

__global__ __launch_bounds__(64) void count_alias_build_kernel(CountAliasParams p) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int K = p.K, wpb = p.wpb, lane = threadIdx.x;
  double *bs = reinterpret_cast<double *>(smem);                                   // [wpb][K]
  double *tnl = bs + (size_t)wpb * K;                                              // [64]
  int32_t *nnzl = reinterpret_cast<int32_t *>(tnl + 64);                           // [64]
  uint16_t *al = reinterpret_cast<uint16_t *>(nnzl + 64);                          // [wpb][K]
  uint16_t *st = al + (size_t)wpb * K;                                             // [wpb][K]

  for (int w0 = blockIdx.x * wpb; w0 < p.V; w0 += gridDim.x * wpb) {
    const int nwd = min(wpb, p.V - w0);
    __syncthreads();
    for (int wi = 0; wi < nwd; ++wi) {                                             // the list, p and the identity alias of word w0 + wi
      const int32_t *row = p.n_wk + (size_t)(w0 + wi) * K;
      uint16_t *out = p.nzw + (size_t)(w0 + wi) * K;
      int n = 0, tot = 0;
      for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const int c = k < K ? row[k] : 0;
        const bool nz = c > 0;
        const unsigned long long m = __ballot(nz);
        const int slot = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (nz) {                                                                  // slot < number of non-zeros <= K
          out[slot] = (uint16_t)k;
          bs[(size_t)wi * K + slot] = (double)c / ((double)p.n_k[k] + p.beta_sum);
          al[(size_t)wi * K + slot] = (uint16_t)slot;
          tot += c;
        }
        n += __popcll(m);
      }
      for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
      if (lane == 0) { nnzl[wi] = n; p.nw[w0 + wi] = n; p.tpt[w0 + wi] = tot; }
    }
    __syncthreads();
    if (lane < nwd) {
      const int n = nnzl[lane];
      const double *b = bs + (size_t)lane * K;
      double tn = 0.0;
      for (int i = 0; i < n; ++i) tn += b[i];
      tnl[lane] = tn;
      p.type_norm[w0 + lane] = tn;
    }
    __syncthreads();
    for (int wi = 0; wi < nwd; ++wi) {
      const int n = nnzl[wi];
      const double tn = tnl[wi], inv_n = 1.0 / (double)n;
      for (int i = lane; i < n; i += 64) bs[(size_t)wi * K + i] = bs[(size_t)wi * K + i] / tn - inv_n;
    }
    __syncthreads();
    if (lane < nwd && nnzl[lane] > 0)                                              // the chain above with k = nnz
      alias_pairing_chain(bs + (size_t)lane * K, st + (size_t)lane * K, al + (size_t)lane * K, nnzl[lane]);
    __syncthreads();
    for (int wi = 0; wi < nwd; ++wi) {
      const int n = nnzl[wi];
      for (int i = lane; i < n; i += 64) {
        const int av = al[(size_t)wi * K + i];
        const size_t o = (size_t)(w0 + wi) * K + i;
        p.ps[o] = av == i ? 1.0 : bs[(size_t)wi * K + i];
        p.a[o] = av;
      }
    }
  }
}

}  // namespace ggs
