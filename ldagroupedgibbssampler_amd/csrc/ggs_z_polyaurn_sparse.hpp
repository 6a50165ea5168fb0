// ggs_z_polyaurn_sparse.hpp -- scheme=polyaurn_sparse: the doubly sparse z step of PolyaUrnSpaliasLDA
// (sampleTopicAssignmentsParallel, PolyaUrnSpaliasLDA.java:180-334) over polyaurn's Poisson-drawn Phi, whose exact zeros
// it is built for.  Per token the conditional (n_dk + alpha_k) * phi[k][w] is split as in ggs_z_spalias.hpp: alpha_k *
// phi[k][w] comes from the word's alias table in O(1) (ggs_alias.hpp), and n_dk * phi[k][w] is non-zero only where BOTH
// factors are -- so it is walked over whichever list is shorter (:261-271): the word's ascending list of topics with
// phi[k][w] != 0 (word_list_build_kernel below, rebuilt with the alias tables after every Phi), or the document's list
// of non-zero topics (spalias's list, in the reference's discipline).  O(min(nnz_w, nnz_d)) per token.
//
// The kernel is sparse_wave_body<true> (ggs_z_spalias.hpp: the wave per document, its LDS, the proposal by wave scans
// with its margins and their proof in terms of n, the exact replay).  This scheme's own rules, old topic removed first,
// nd = the document list's length, nw = the word's:
//   candidates c_0 .. c_{n-1} = the word's list if nw < nd, else (a tie included) the document's list;
//   n == 0 (a one-token document, an all-zero Phi column): topic = min((int)(U * K), K - 1), polyaurn's rule; tested
//   first, such a token reaches neither the proposal nor the replay (GGS_DEBUG_MARGIN = 1e30 sends every token WITH
//   candidates through the replay);
//   a word-list candidate the document does not use (cnt == 0) scores 0.0 and is walked like any other.
// The scores are non-negative (a count times a Poisson count over a positive total), as the shared proof asks.
// Loaded ahead beside what spalias loads: nw[w] with the chunk, the first 64 entries of a token's word list two tokens
// ahead and the Phi values at them one token ahead (used if that token takes the word's list).
// Counters (ggs_get_sparse_stats) are kept in registers and added once per document.
#pragma once
#include "ggs_z_spalias.hpp"

namespace ggs {

// ---- the words' lists ------------------------------------------------------------------------------------------------
// nzw [V][K] u16 (fixed stride; entries past nw[w] are not written), nw [V].  One wave per word: per block of 64 topics a
// ballot of phi != 0.0 and each lane's prefix popcount give the slots, ascending in k.
struct WordListParams {
  const double *phiT;          // [V][Kp]
  uint16_t *nzw;               // [V][K]
  int32_t *nw;                 // [V]
  int32_t V, K, Kp;
  // FROM_MASK (scheme nzvsspalias, ggs_phi_vs.hpp): the list is the cells the variable-selection draw DREW -- bit k & 31 of
  // zero_mask[w * mask_pitch + (k >> 5)] clear -- not phi != 0.0: a drawn gamma that underflowed to 0.0 stays listed
  const uint32_t *zero_mask;
  int32_t mask_pitch;
  // FROM_COUNTS (scheme adlda, ggs_z_adlda.hpp): the list is the topics with counts[w * K + k] > 0, the corpus-wide counts
  const int32_t *counts;       // [V][K]
};

constexpr int kWordListBlock = 256;

template <bool FROM_MASK, bool FROM_COUNTS = false>
__device__ __forceinline__ void word_list_build_body(const WordListParams &p) {
  const int lane = threadIdx.x & 63, waves = kWordListBlock / 64;
  for (int64_t w = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6); w < p.V; w += (int64_t)gridDim.x * waves) {
    const double *row = p.phiT + (size_t)w * p.Kp;
    uint16_t *out = p.nzw + (size_t)w * p.K;
    int n = 0;
    for (int k0 = 0; k0 < p.K; k0 += 64) {
      const int k = k0 + lane;
      bool nz;
      if constexpr (FROM_COUNTS) nz = k < p.K && p.counts[(size_t)w * p.K + k] > 0;
      else if constexpr (FROM_MASK) nz = k < p.K && !((p.zero_mask[(size_t)w * p.mask_pitch + (k >> 5)] >> (k & 31)) & 1u);
      else nz = k < p.K && row[k] != 0.0;
      const unsigned long long m = __ballot(nz);
      const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (nz) out[n + before] = (uint16_t)k;                                       // n + before < number of non-zeros <= K
      n += __popcll(m);
    }
    if (lane == 0) p.nw[w] = n;
  }
}
__global__ __launch_bounds__(kWordListBlock) void word_list_build_kernel(WordListParams p) { word_list_build_body<false>(p); }
__global__ __launch_bounds__(kWordListBlock) void word_list_mask_kernel(WordListParams p) { word_list_build_body<true>(p); }
__global__ __launch_bounds__(kWordListBlock) void word_list_counts_kernel(WordListParams p) { word_list_build_body<false, true>(p); }

// ---- the z step ------------------------------------------------------------------------------------------------------
struct PolyaurnSparseParams : SpaliasParams {
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  unsigned long long *stats;   // [4]: word-list tokens, document-list tokens, uniform draws, sum of n
};

inline size_t polyaurn_sparse_lds_bytes(int K, int cap) { return spalias_lds_bytes(K, cap); }

__global__ __launch_bounds__(64) void polyaurn_sparse_wave_kernel(PolyaurnSparseParams sp) { sparse_wave_body<true>(sp); }
// scheme nzvsspalias (NZVSSpaliasUncollapsedParallelLDA.java:157-315): the same step over the variable-selection Phi and
// the drawn cells' lists, except that a token without a candidate draws from its word's alias table (:252-254)
__global__ __launch_bounds__(64) void nzvs_wave_kernel(PolyaurnSparseParams sp) { sparse_wave_body<true, PolyaurnSparseParams, true>(sp); }

}  // namespace ggs
