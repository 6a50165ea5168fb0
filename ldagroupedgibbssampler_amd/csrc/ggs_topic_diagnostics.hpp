// ggs_topic_diagnostics.hpp -- the per-topic quality scores of topics/TopicModelDiagnosticsPlain.java (topicsToCsv, the file
// save_doc_topic_diagnostics makes tui/ParallelLDA.java:218-225 write) from the device-resident z and type-topic counts.
// The contract -- every statistic and every score with its Java order of operations -- is the table at ggs_topic_doc_statistics
// in include/ggs_hip.h and DESIGN.md 6l.  Every product, quotient and sum is rounded on its own (-ffp-contract=off); log is
// strict_log.
//
// Document statistics (collectDocumentStatistics :108-220), in pieces of documents so that the work space stays bounded:
//   td_docs_kernel     a wave per document on a persistent grid.  LDS holds a K-long int32 histogram of the document's z and, per
//                      topic, a 128-bit mask of the positions r whose top word T_k[r] the document has under topic k.  A token
//                      (w, z) finds "is w among T_z, and where" in a CSR by word of the K * n (topic, position) pairs (built
//                      by the host from idx: most words have an empty list and cost one pair of loads).  After the tokens the
//                      lanes walk the topics: the count goes to the piece's dense row c[d][k], the pairs of the mask to the
//                      upper triangle of codoc (integer atomics, exact in any order), the wave's argmax (lowest k among equal
//                      maxima) to maxtopic[d]; every entry is cleared as it is read.
//   td_columns_kernel  lane = topic, 256 documents of the piece per wave: nonzero, rank1 and at_prop in registers, one atomic
//                      per counter at the end; the addend c * log(c) of every (document, topic) into addend[d][k] (-1.0 where
//                      c == 0: the Java adds nothing there).
//   td_clogc_kernel    the one rounding chain per topic over the documents in index order: lane = topic, s = s + addend.
//   td_mirror_kernel   codoc's lower triangle from its upper one.
// Topic scores (:226-541):
//   td_nk_kernel, td_wtc_kernel   tokensPerTopic and wordTypeCounts as integer column / row sums of the counts.
//   td_sorted_kernel   a wave per topic: the non-zero cells of the column compacted in falling id, a stable LSD radix sort by
//                      falling count (8-bit digits, only as many passes as the column's largest count needs) -- IDSorter's
//                      order -- and the chains over the sorted cells: eff_num_words always (a zero cell adds +0.0), uniform_dist
//                      and corpus_dist only for a column without zero cells (one zero cell's addend is 0.0 * log(0.0) = NaN).
//   td_small_kernel    a wave per topic: tokens, document_entropy, coherence, token-doc-diff, the three ratios and the word
//                      scores; the lanes compute the logarithms of a row in parallel, every lane then walks the Java chain.
#pragma once
#include "ggs_device_math.hpp"

namespace ggs {

constexpr int kTdMaxWords = 128;      // the cap on n: GGS_TOP_WORDS_MAX, one bit each in the 128-bit mask
constexpr int kTdStats = 9;           // nonzero, rank1, at_prop[7]
constexpr int kTdLdsPerTopic = 20;    // bytes of LDS per topic in td_docs_kernel: the count and four mask words
constexpr int kTdMaxTopics = 3072;    // 60 KiB of LDS
constexpr int kTdSegDocs = 256;       // documents per wave of td_columns_kernel
constexpr int kTdScoreRows = 10;      // topic_scores rows: the CSV's columns without word-length
constexpr int kTdWordRows = 4;        // word_scores rows: coherence, uniform_dist, corpus_dist, token-doc-diff

struct TdDocParams {
  const int64_t *doc_ptr;             // [D + 1]
  const int32_t *tok, *z;             // [N]
  const int32_t *mem_ptr, *mem;       // CSR by word: [V + 1], entries topic * 128 + position
  int32_t *crow;                      // [piece][K]
  int32_t *maxtopic;                  // [piece]
  int32_t *codoc;                     // [K][n][n]
  const double *alpha;                // [K]
  double alpha_sum;
  double *addend;                     // [piece][K]
  int32_t *doc_stats;                 // [K][9]
  int64_t d0, nd;                     // the piece: documents [d0, d0 + nd)
  int32_t K, n;
};

__global__ __launch_bounds__(64) void td_docs_kernel(TdDocParams p) {
  extern __shared__ int32_t td_lds[];                       // hist [K], then mask [K][4]
  int32_t *hist = td_lds;
  uint32_t *mask = reinterpret_cast<uint32_t *>(td_lds + p.K);
  const int lane = threadIdx.x, K = p.K, n = p.n;
  for (int i = lane; i < 5 * K; i += 64) td_lds[i] = 0;
  __syncthreads();
  for (int64_t dl = blockIdx.x; dl < p.nd; dl += gridDim.x) {
    const int64_t t0 = p.doc_ptr[p.d0 + dl], t1 = p.doc_ptr[p.d0 + dl + 1];
    for (int64_t t = t0 + lane; t < t1; t += 64) {
      const int w = p.tok[t], k = p.z[t];
      atomicAdd(&hist[k], 1);
      const int e1 = p.mem_ptr[w + 1];
      for (int e = p.mem_ptr[w]; e < e1; ++e) {
        const int m = p.mem[e];
        if ((m >> 7) == k) atomicOr(&mask[4 * k + ((m & 127) >> 5)], 1u << (m & 31));
      }
    }
    __syncthreads();
    int best_c = 0, best_k = -1;
    for (int k = lane; k < K; k += 64) {
      const int c = hist[k];
      p.crow[(size_t)dl * K + k] = c;
      if (c == 0) continue;
      hist[k] = 0;
      if (c > best_c) { best_c = c; best_k = k; }          // a lane's topics rise: strict > keeps the lowest
      int32_t *cd = p.codoc + (size_t)k * n * n;
      for (int wi = 0; wi < 4; ++wi) {
        uint32_t a = mask[4 * k + wi];
        while (a) {
          const int bi = __ffs(a) - 1, i = wi * 32 + bi;
          a &= a - 1;
          atomicAdd(&cd[i * n + i], 1);
          for (int wj = wi; wj < 4; ++wj) {
            uint32_t b = mask[4 * k + wj];
            if (wj == wi) b &= ~((2u << bi) - 1u);          // the positions above i
            while (b) {
              const int j = wj * 32 + __ffs(b) - 1;
              b &= b - 1;
              atomicAdd(&cd[i * n + j], 1);
            }
          }
        }
      }
      for (int wi = 0; wi < 4; ++wi) mask[4 * k + wi] = 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const int oc = __shfl_xor(best_c, d), ok = __shfl_xor(best_k, d);
      if (ok >= 0 && (oc > best_c || (oc == best_c && ok < best_k))) { best_c = oc; best_k = ok; }
    }
    if (lane == 0) p.maxtopic[dl] = best_k;                 // -1: an empty document
    __syncthreads();
  }
}

__global__ __launch_bounds__(64) void td_columns_kernel(TdDocParams p) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= p.K) return;
  const int64_t dl0 = (int64_t)blockIdx.y * kTdSegDocs, dl1 = min(dl0 + (int64_t)kTdSegDocs, p.nd);
  const double a_k = p.alpha[k];
  int st[kTdStats];
#pragma unroll
  for (int i = 0; i < kTdStats; ++i) st[i] = 0;
  for (int64_t dl = dl0; dl < dl1; ++dl) {
    const int c = p.crow[(size_t)dl * p.K + k];
    double a = -1.0;
    if (c > 0) {
      st[0] += 1;
      const int64_t len = p.doc_ptr[p.d0 + dl + 1] - p.doc_ptr[p.d0 + dl];
      const double prop = (a_k + (double)c) / (p.alpha_sum + (double)len);
      constexpr double P[7] = {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5};
      bool go = true;
#pragma unroll
      for (int i = 0; i < 7; ++i) { go = go && !(prop < P[i]); st[2 + i] += go ? 1 : 0; }
      a = c > 1 ? (double)c * strict_log((double)c) : 0.0;  // 1 * log(1) = +0.0
    }
    if (p.maxtopic[dl] == k) st[1] += 1;
    p.addend[(size_t)dl * p.K + k] = a;
  }
#pragma unroll
  for (int i = 0; i < kTdStats; ++i)
    if (st[i]) atomicAdd(&p.doc_stats[k * kTdStats + i], st[i]);
}

__global__ __launch_bounds__(64) void td_clogc_kernel(const double *addend, int64_t nd, int32_t K, double *clogc) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  double s = clogc[k];
  constexpr int U = 8;
  int64_t dl = 0;
  for (; dl + U <= nd; dl += U) {
    double a[U];
#pragma unroll
    for (int j = 0; j < U; ++j) a[j] = addend[(size_t)(dl + j) * K + k];
#pragma unroll
    for (int j = 0; j < U; ++j)
      if (a[j] >= 0.0) s = s + a[j];
  }
  for (; dl < nd; ++dl) {
    const double a = addend[(size_t)dl * K + k];
    if (a >= 0.0) s = s + a;
  }
  clogc[k] = s;
}

__global__ __launch_bounds__(256) void td_mirror_kernel(int32_t *codoc, int32_t K, int32_t n) {
  const int64_t total = (int64_t)K * n * n;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
    const int j = (int)(t % n), i = (int)((t / n) % n);
    const int64_t k = t / ((int64_t)n * n);
    if (i > j) codoc[t] = codoc[(k * n + j) * n + i];
  }
}

// ---- the topic scores ------------------------------------------------------------------------------------------------------
struct TdScoreParams {
  const int32_t *cnt;                 // [V][pitch]
  int32_t *n_k, *wtc;                 // [K], [V]
  const int32_t *idx;                 // [K][n]
  const int32_t *codoc, *doc_stats;   // [K][n][n], [K][9]
  const double *clogc;                // [K]
  int32_t *key_a, *id_a, *key_b, *id_b;   // [group][V] each: the sort's two buffers
  int32_t *sorted_head;               // [K][n]: the first n sorted cells' ids, -1 beyond the column's non-zero cells
  double *topic_scores;               // [10][K]
  double *word_scores;                // [4][K][n]
  double beta;
  int32_t pitch, V, K, n, k0;         // k0: the first topic of this launch's group
};

__global__ __launch_bounds__(64) void td_nk_kernel(TdScoreParams p) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= p.K) return;
  int s = 0;
  for (int w = blockIdx.y; w < p.V; w += gridDim.y) s += p.cnt[(size_t)w * p.pitch + k];
  if (s) atomicAdd(&p.n_k[k], s);
}

__device__ __forceinline__ int td_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ long long td_num_tokens(const int32_t *n_k, int K, int lane) {
  long long s = 0;
  for (int k = lane; k < K; k += 64) s += n_k[k];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d);
  return s;
}

__global__ __launch_bounds__(64) void td_wtc_kernel(TdScoreParams p) {
  const int lane = threadIdx.x;
  for (int w = blockIdx.x; w < p.V; w += gridDim.x) {
    int s = 0;
    for (int k = lane; k < p.K; k += 64) s += p.cnt[(size_t)w * p.pitch + k];
    s = td_wave_sum(s);
    if (lane == 0) p.wtc[w] = s;
  }
}

__global__ __launch_bounds__(64) void td_sorted_kernel(TdScoreParams p) {
  __shared__ int32_t off[256];
  __shared__ double buf[3][64];
  const int lane = threadIdx.x, k = p.k0 + blockIdx.x, V = p.V;
  const size_t base = (size_t)blockIdx.x * V;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int32_t *key = p.key_a + base, *id = p.id_a + base, *key2 = p.key_b + base, *id2 = p.id_b + base;
  // the non-zero cells, ids falling
  int m = 0, maxc = 0;
  for (int hi = V - 1; hi >= 0; hi -= 64) {
    const int w = hi - lane;
    const int c = w >= 0 ? p.cnt[(size_t)w * p.pitch + k] : 0;
    const unsigned long long b = __ballot(c > 0);
    if (c > 0) { const int pos = m + __popcll(b & lt); key[pos] = c; id[pos] = w; }
    m += __popcll(b);
    maxc = max(maxc, c);
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) maxc = max(maxc, __shfl_xor(maxc, d));
  __syncthreads();
  // stable LSD radix sort by falling count
  const int bits = maxc > 0 ? 32 - __clz(maxc) : 0;
  for (int shift = 0; shift < bits; shift += 8) {
    for (int i = lane; i < 256; i += 64) off[i] = 0;
    __syncthreads();
    for (int i = lane; i < m; i += 64) atomicAdd(&off[(key[i] >> shift) & 255], 1);
    __syncthreads();
    {                                                       // off[d] = cells with a larger digit: lane L owns digits 255 - 4L down to 252 - 4L
      const int d0 = 255 - 4 * lane;
      const int h0 = off[d0], h1 = off[d0 - 1], h2 = off[d0 - 2], h3 = off[d0 - 3];
      const int t = h0 + h1 + h2 + h3;
      int inc = t;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc, d); if (lane >= d) inc += o; }
      const int ex = inc - t;
      off[d0] = ex; off[d0 - 1] = ex + h0; off[d0 - 2] = ex + h0 + h1; off[d0 - 3] = ex + h0 + h1 + h2;
    }
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += 64) {
      const int i = i0 + lane;
      const bool valid = i < m;
      const int kv = valid ? key[i] : 0, iv = valid ? id[i] : 0, dg = (kv >> shift) & 255;
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (dg >> b) & 1;
        const unsigned long long bal = __ballot(bit);
        peers &= bit ? bal : ~bal;
      }
      const int rank = __popcll(peers & lt);
      if (valid) { const int pos = off[dg] + rank; key2[pos] = kv; id2[pos] = iv; }
      __syncthreads();
      if (valid && rank == 0) off[dg] += __popcll(peers);
      __syncthreads();
    }
    int32_t *t = key; key = key2; key2 = t;
    t = id; id = id2; id2 = t;
    __syncthreads();
  }
  for (int r = lane; r < p.n; r += 64) p.sorted_head[(size_t)k * p.n + r] = r < m ? id[r] : -1;
  // the chains over the sorted cells
  const int nk = p.n_k[k];
  const double nkd = (double)nk;
  const double coef = (double)td_num_tokens(p.n_k, p.K, lane) / nkd;
  const bool dense = m == V;
  double s_eff = 0.0, s_u = 0.0, s_c = 0.0;
  for (int i0 = 0; i0 < m; i0 += 64) {
    const int i = i0 + lane;
    if (i < m) {
      const double cd = (double)key[i];
      const double pr = cd / nkd;
      buf[0][lane] = pr * pr;
      if (dense) {
        buf[1][lane] = pr * strict_log((cd * (double)V) / nkd);
        buf[2][lane] = pr * strict_log(coef * cd / (double)p.wtc[id[i]]);
      }
    }
    __syncthreads();
    const int cntv = min(64, m - i0);
    for (int j = 0; j < cntv; ++j) s_eff += buf[0][j];
    if (dense)
      for (int j = 0; j < cntv; ++j) { s_u += buf[1][j]; s_c += buf[2][j]; }
    __syncthreads();
  }
  if (lane == 0) {
    const double nan = __builtin_nan("");
    p.topic_scores[(size_t)3 * p.K + k] = dense ? s_u : nan;
    p.topic_scores[(size_t)4 * p.K + k] = dense ? s_c : nan;
    p.topic_scores[(size_t)5 * p.K + k] = nk == 0 ? nan : 1.0 / s_eff;   // n_k == 0: every p is 0 / 0
  }
}

__global__ __launch_bounds__(64) void td_small_kernel(TdScoreParams p) {
  __shared__ double buf[kTdMaxWords], wd[kTdMaxWords], dd[kTdMaxWords];
  const int lane = threadIdx.x, k = blockIdx.x, n = p.n, K = p.K;
  const int32_t *cd = p.codoc + (size_t)k * n * n, *st = p.doc_stats + k * kTdStats, *ix = p.idx + (size_t)k * n;
  double *ws = p.word_scores;
  const size_t wrow = (size_t)K * n, wk = (size_t)k * n;
  const int nk = p.n_k[k];
  const double nkd = (double)nk, beta = p.beta;
  const double coef = (double)td_num_tokens(p.n_k, K, lane) / nkd;
  // coherence (:474-499)
  double topic = 0.0;
  for (int row = 0; row < n; ++row) {
    for (int col = lane; col < row; col += 64) buf[col] = strict_log(((double)cd[row * n + col] + beta) / ((double)cd[col * n + col] + beta));
    __syncthreads();
    double row_score = 0.0, mn = 0.0;
    for (int col = 0; col < row; ++col) {
      const double s = buf[col];
      row_score += s;
      if (s < mn) mn = s;
    }
    topic += row_score;
    if (lane == 0 && ws) ws[wk + row] = mn;
    __syncthreads();
  }
  const double coherence = topic;
  // the word scores of uniform_dist and corpus_dist; the two distributions of token-doc-diff (:345-396)
  for (int r = lane; r < n; r += 64) {
    const int w = ix[r];
    const double c = (double)p.cnt[(size_t)w * p.pitch + k];
    const double pr = c / nkd;
    if (ws) {
      ws[wrow + wk + r] = pr * strict_log((c * (double)p.V) / nkd);
      ws[2 * wrow + wk + r] = pr * strict_log(coef * c / (double)p.wtc[w]);
    }
    wd[r] = c;
    dd[r] = (double)cd[r * n + r];
  }
  __syncthreads();
  double word_sum = 0.0, doc_sum = 0.0;
  for (int r = 0; r < n; ++r) { word_sum += wd[r]; doc_sum += dd[r]; }
  for (int r = lane; r < n; r += 64) {
    const double pp = wd[r] / word_sum, q = dd[r] / doc_sum;
    const double mean = 0.5 * (pp + q);
    double score = 0.0;
    if (pp > 0) score += 0.5 * pp * strict_log(pp / mean);
    if (q > 0) score += 0.5 * q * strict_log(q / mean);
    buf[r] = score;
    if (ws) ws[3 * wrow + wk + r] = score;
  }
  __syncthreads();
  double diff = 0.0;
  for (int r = 0; r < n; ++r) diff += buf[r];
  if (lane == 0) {
    double *ts = p.topic_scores;
    ts[k] = nkd;
    ts[(size_t)K + k] = -p.clogc[k] / nkd + strict_log(nkd);
    ts[(size_t)2 * K + k] = coherence;
    ts[(size_t)6 * K + k] = diff;
    ts[(size_t)7 * K + k] = (double)st[1] / (double)st[0];
    ts[(size_t)8 * K + k] = (double)st[2 + 6] / (double)st[2 + 1];
    ts[(size_t)9 * K + k] = (double)st[2 + 5] / (double)st[0];
  }
}

}  // namespace ggs
