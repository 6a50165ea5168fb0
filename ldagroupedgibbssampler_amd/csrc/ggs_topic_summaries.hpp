// ggs_topic_summaries.hpp -- the best n words of every topic under the five rankings of LDAUtils.java, from the
// type-topic counts n_wk [V][pitch] on the device (TopWords.txt, RelevanceWords.txt and their three siblings).
//
//   kind          Java                                               score of (word w, topic k)
//   top           getTopWords / getTopWordIndices  :874-911          (double) n_wk
//   relevance     getTopRelevanceWords             :566-590          lambda * L + (1 - lambda) * (L - log(p_w[w])),  L = log(p_wk)
//   distinctive   getTopDistinctiveWords           :592-617,654-664  0.0 + P * log(P / p_w[w])
//   salient       getTopSalientWords               :619-644,674-685  p_w[w] * distinctive
//   k1            getK1ReWeightedWords             :752-801          p_wk / (sum over k, in index order from 0.0, of p_wk)
//   p_wk = (n_wk + beta) / mass_k (calcWordProbGivenTopic :803-818),  p_w[w] = rowsum_w / total (calcWordProb :704-720),
//   P = p_wk * (mass_k / total) / p_w[w], evaluated left to right (calcTopicProbGivenWord :826-856).
// Every product, sum and quotient is rounded on its own, in the Java order (the unit is built with -ffp-contract=off);
// log is strict_log.  The ranking is IDSorter's: falling score, equal scores (-0.0 == +0.0) by FALLING word id.
//
// The normalisers are Java running sums from 0.0 over (double) n_wk + beta: mass_k over w, rowsum_w over k, and `total`, ONE
// chain over all V * K cells with w outer and k inner.  mass_k and total are column sums in the sense of ggs_exact_sum.hpp
// (total: the one column of the cells flattened, V * K long), launched by the caller in work space of their own; ts_words_kernel
// below walks the K-long chains of every word.
//
// Selection never sorts K x V scores.  ts_select_kernel: a wave owns kTsSegWords consecutive words x 64 adjacent topics, lane =
// topic (n_wk is [V][pitch]: a wave's load of one word's 64 counts is one coalesced row piece); a lane walks its words from the
// highest id down and keeps its topic's best n so far as a sorted list -- in LDS up to kTsLdsWords, beyond in the candidate
// buffer itself.  Walking ids downwards, a word enters only by a strictly greater score than the list's last, so the zero
// cells of a sparse matrix cost one comparison each once the list holds n words.  ts_merge_kernel: a wave per topic merges the
// segments' sorted lists, lane = segments lane, lane + 64, ..., n rounds of a wave-wide argmax over the lists' heads.
// A relevance score of a zero cell needs no logarithm of its own: L is then log(beta / mass_k), one per lane.
#pragma once
#include "ggs_device_math.hpp"

namespace ggs {

constexpr int kTsTop = 0, kTsRelevance = 1, kTsDistinctive = 2, kTsSalient = 3, kTsK1 = 4, kTsKinds = 5;
constexpr int kTsSegWords = 256;     // words per segment of the selection kernel
constexpr int kTsTopics = 64;        // topics per workgroup (one wave, lane = topic)
constexpr int kTsMaxWords = 128;     // the cap on n
constexpr int kTsLdsWords = 64;      // lists of up to this many words live in LDS: 64 * 64 * 12 bytes = 48 KiB

struct TsParams {
  const int32_t *cnt;                // [V][pitch]
  const double *mass;                // [K]
  const double *total;               // [1]
  double *rowsum, *k1mass, *pw, *logpw;   // [V] each, written by ts_words_kernel
  double *cand_score;                // [nseg][n][K]: the segments' sorted lists
  int32_t *cand_id;
  int32_t *idx;                      // [K][n]
  double *score;                     // [K][n]
  double *all_scores;                // [V][K], ts_scores_kernel only
  double beta, lambda, one_minus_lambda;
  int32_t pitch, V, K, kind, n, nseg;
};

// rank key of a score: unsigned order == numeric order, the two zeros equal
__device__ __forceinline__ unsigned long long ts_key(double x) {
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  if ((b << 1) == 0) b = 0;
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ bool ts_beats(unsigned long long ua, int ia, unsigned long long ub, int ib) { return ua > ub || (ua == ub && ia > ib); }

// what a lane (topic) keeps for all of its words
struct TsTopic {
  double mass, p_t, L0;              // mass_k; mass_k / total; relevance: log(beta / mass_k), the L of a zero cell
};
__device__ __forceinline__ TsTopic ts_topic(const TsParams &p, int k) {
  TsTopic t{1.0, 0.0, 0.0};
  if (p.kind == kTsTop) return t;
  t.mass = p.mass[k];
  t.p_t = t.mass / *p.total;
  if (p.kind == kTsRelevance) t.L0 = strict_log((0.0 + p.beta) / t.mass);
  return t;
}
// the score of (w, k) with count raw
__device__ __forceinline__ double ts_score(const TsParams &p, const TsTopic &t, int w, int32_t raw) {
  if (p.kind == kTsTop) return (double)raw;
  const double weight = (double)raw + p.beta;
  const double p_wk = weight / t.mass;
  if (p.kind == kTsRelevance) {
    const double L = raw == 0 ? t.L0 : strict_log(p_wk);
    const double a = p.lambda * L;
    const double b = p.one_minus_lambda * (L - p.logpw[w]);
    return a + b;
  }
  if (p.kind == kTsK1) return p_wk / p.k1mass[w];
  const double pw = p.pw[w];
  const double P = p_wk * t.p_t / pw;
  const double d = 0.0 + P * strict_log(P / pw);            // wordDistinctiveness[w][k] += ...: a -0.0 product becomes +0.0
  return p.kind == kTsDistinctive ? d : pw * d;
}

// rowsum_w, the K1 mass, p_w and log(p_w) of every word: a wave takes 64 words, stages [64 words][64 topics] tiles through LDS
// (coalesced along k) and lane = word walks its row of the tile in index order.
__global__ __launch_bounds__(64) void ts_words_kernel(TsParams p) {
  __shared__ double tile[64][65];                            // 33 KiB; the K1 chain is a second pass over the same tiles
  const int lane = threadIdx.x, w0 = blockIdx.x * 64, w = w0 + lane;
  double rs = 0.0, km = 0.0;
  for (int pass = 0; pass < (p.kind == kTsK1 ? 2 : 1); ++pass)
    for (int k0 = 0; k0 < p.K; k0 += 64) {
      const int kw = min(64, p.K - k0), k = min(k0 + lane, p.K - 1);
      const double mass = p.mass[k];
      for (int r = 0; r < 64; ++r) {
        const int32_t raw = p.cnt[(size_t)min(w0 + r, p.V - 1) * p.pitch + k];
        const double x = (double)raw + p.beta;
        tile[r][lane] = pass ? x / mass : x;
      }
      __syncthreads();
      if (pass)
        for (int c = 0; c < kw; ++c) km += tile[lane][c];
      else
        for (int c = 0; c < kw; ++c) rs += tile[lane][c];
      __syncthreads();
    }
  if (w < p.V) {
    const double pw = rs / *p.total;
    p.rowsum[w] = rs; p.k1mass[w] = km; p.pw[w] = pw; p.logpw[w] = strict_log(pw);
  }
}

// every score, for the tests
__global__ __launch_bounds__(256) void ts_scores_kernel(TsParams p) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= p.K) return;
  const TsTopic t = ts_topic(p, k);
  for (int w = blockIdx.y; w < p.V; w += gridDim.y) p.all_scores[(size_t)w * p.K + k] = ts_score(p, t, w, p.cnt[(size_t)w * p.pitch + k]);
}

// how many words segment seg hands to the merge
__device__ __forceinline__ int ts_seg_count(const TsParams &p, int seg) { return min(p.n, min(kTsSegWords, p.V - seg * kTsSegWords)); }

template <bool LDS_LIST>
__global__ __launch_bounds__(64) void ts_select_kernel(TsParams p) {
  extern __shared__ double ts_lds[];                         // LDS_LIST: scores [n][64], then ids [n][64]
  const int lane = threadIdx.x, seg = blockIdx.x, k = blockIdx.y * kTsTopics + lane, n = p.n;
  if (k >= p.K) return;                                      // a lane touches only its own column of the lists: no barrier below
  const int v0 = seg * kTsSegWords, v1 = min(v0 + kTsSegWords, p.V);
  double *gs = p.cand_score + (size_t)seg * n * p.K + k;     // entry r of this lane's list: gs[r * K], gi[r * K]
  int32_t *gi = p.cand_id + (size_t)seg * n * p.K + k;
  double *ls = LDS_LIST ? ts_lds + lane : gs;
  int32_t *li = LDS_LIST ? reinterpret_cast<int32_t *>(ts_lds + (size_t)n * 64) + lane : gi;
  const size_t stride = LDS_LIST ? 64 : (size_t)p.K;
  const TsTopic t = ts_topic(p, k);
  int m = 0, last_id = -1;                                   // words in the list; the list's last entry once it is full
  unsigned long long last_u = 0;
  constexpr int U = 8;
  for (int wt = v1 - 1; wt >= v0; wt -= U) {
    int32_t raw[U];
#pragma unroll
    for (int j = 0; j < U; ++j) raw[j] = p.cnt[(size_t)max(wt - j, v0) * p.pitch + k];
#pragma unroll 1
    for (int j = 0; j < U && wt - j >= v0; ++j) {
      const int w = wt - j;
      const double s = ts_score(p, t, w, raw[j]);
      const unsigned long long u = ts_key(s);
      if (m == n && !ts_beats(u, w, last_u, last_id)) continue;
      int pos = m < n ? m++ : n - 1;
      while (pos > 0) {
        const double ps = ls[(size_t)(pos - 1) * stride];
        const int pi = li[(size_t)(pos - 1) * stride];
        if (!ts_beats(u, w, ts_key(ps), pi)) break;
        ls[(size_t)pos * stride] = ps; li[(size_t)pos * stride] = pi;
        --pos;
      }
      ls[(size_t)pos * stride] = s; li[(size_t)pos * stride] = w;
      if (m == n) { last_u = ts_key(ls[(size_t)(n - 1) * stride]); last_id = li[(size_t)(n - 1) * stride]; }
    }
  }
  if (LDS_LIST)
    for (int r = 0; r < m; ++r) { gs[(size_t)r * p.K] = ls[(size_t)r * 64]; gi[(size_t)r * p.K] = li[(size_t)r * 64]; }
}

// one wave per topic: n rounds of an argmax over the heads of the segments' lists
__global__ __launch_bounds__(64) void ts_merge_kernel(TsParams p) {
  extern __shared__ int32_t ts_heads[];                      // [nseg]
  const int lane = threadIdx.x, k = blockIdx.x, n = p.n;
  for (int s = lane; s < p.nseg; s += 64) ts_heads[s] = 0;   // a lane reads and writes only its own segments' heads
  double best_s = 0.0;
  unsigned long long best_u = 0;
  int best_id = -1, best_seg = -1;
  auto rescan = [&]() {
    best_u = 0; best_id = -1; best_seg = -1; best_s = 0.0;
    for (int s = lane; s < p.nseg; s += 64) {
      const int hd = ts_heads[s];
      if (hd >= ts_seg_count(p, s)) continue;
      const size_t at = ((size_t)s * n + hd) * p.K + k;
      const double sc = p.cand_score[at];
      const int id = p.cand_id[at];
      const unsigned long long u = ts_key(sc);
      if (best_id < 0 || ts_beats(u, id, best_u, best_id)) { best_u = u; best_id = id; best_seg = s; best_s = sc; }
    }
  };
  rescan();
  for (int r = 0; r < n; ++r) {
    unsigned long long wu = best_u;
    int wi = best_id;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
      const unsigned long long ou = __shfl_xor(wu, d);
      const int oi = __shfl_xor(wi, d);
      if (oi >= 0 && (wi < 0 || ts_beats(ou, oi, wu, wi))) { wu = ou; wi = oi; }
    }
    if (wi >= 0 && wi == best_id) {                          // word ids are unique: exactly one lane
      p.idx[(size_t)k * n + r] = best_id;
      p.score[(size_t)k * n + r] = best_s;
      ts_heads[best_seg] += 1;
      rescan();
    }
  }
}

}  // namespace ggs
