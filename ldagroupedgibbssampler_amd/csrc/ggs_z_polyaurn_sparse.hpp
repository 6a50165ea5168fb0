// ggs_z_polyaurn_sparse.hpp -- scheme=polyaurn_sparse: the doubly sparse z step of PolyaUrnSpaliasLDA
// (sampleTopicAssignmentsParallel, PolyaUrnSpaliasLDA.java:180-334) over polyaurn's Poisson-drawn Phi, whose exact zeros
// it is built for.  Per token the conditional (n_dk + alpha_k) * phi[k][w] is split as in ggs_z_spalias.hpp: alpha_k *
// phi[k][w] comes from the word's alias table in O(1) (ggs_alias.hpp), and n_dk * phi[k][w] is non-zero only where BOTH
// factors are -- so it is walked over whichever list is shorter (:261-271): the word's ascending list of topics with
// phi[k][w] != 0 (word_list_build_kernel below, rebuilt with the alias tables after every Phi), or the document's list
// of non-zero topics (spalias's list, in the reference's discipline).  O(min(nnz_w, nnz_d)) per token.
//
// Per token, old topic removed first; nd = the document list's length, nw = the word list's:
//   candidates c_0 .. c_{n-1} = the word's list if nw < nd, else (a tie included) the document's list;
//   n == 0 (a one-token document, an all-zero Phi column): topic = min((int)(U * K), K - 1), polyaurn's rule; tested first;
//   cum[i] = (double)cnt[c_i] * phi[c_i][w] + cum[i-1], sum = cum[n-1], tn = typeNorm[w];
//   U < tn / (tn + sum):  x = U + (sum * U) / tn, ups = x * K, i = (int)ups, topic = (ups - i) > ps[w][i] ? a[w][i] : i
//                         (i == K: GGS_ERR_INVALID_TOPIC);
//   else                  ul = U * (tn + sum) - tn, topic = c_i at the smallest i with ul <= cum[i], c_{n-1} if there is none.
// A word-list candidate the document does not use (cnt == 0) scores 0.0 and is walked like any other.
//
// The kernel is spalias_wave_kernel's in shape: one WAVE per document, a persistent grid of single-wave workgroups over
// the length-sorted document list, in LDS the counts int32 [K], the document's list u16 [cap], the back-mapping u16 [K]
// and the running sums fp64 [cap]; cap = min(K, longest document) bounds n too (n <= nd whichever list is walked).
// The sequential cum chain comes out bit-identical to the reference's by spalias's method, n in the role of nnz: wave
// scans only PROPOSE, and the chain is the replay.  The scores are non-negative (a count times a Poisson count over a
// positive total), so every partial sum of the n scores, in whatever association, and every chain value are within
// n * 2^-53 * S of the real prefix (S = the real sum) and differ by at most 2 n 2^-53 S; with
// eps = (4 n + 64) * 2^-53 (more than twice every bound below):
//   - the reference's threshold tn / (tn + sum) is within (2 n + 4) 2^-53 (relative) of this kernel's thr: U < thr (1 - eps)
//     proves the alias branch, U > thr (1 + eps) the other;
//   - alias branch: the reference's ups = (U + sum U / tn) K is within K x (2 n + 4) 2^-53 of this kernel's; with
//     dm = K eps (x + 1), a fractional part more than dm away from 0, 1 and ps[w][i] proves both i and the comparison;
//   - list branch: ul and cum[i] are each within (2 n + 6) 2^-53 (tn + S) of this kernel's; with delta = eps (tn + S'),
//     the first entry with ul' - cum'[i] < -delta is the reference's entry provided the entry before it has
//     ul' - cum'[i-1] > delta (the real prefixes are monotone; zero scores leave equal neighbours, which the second test
//     then refuses: such a token is replayed).
// A token that is not decided, and everything Java would throw on, is replayed by ONE chain of fp64 adds in candidate
// order.  GGS_DEBUG_MARGIN scales eps up: 1e30 sends every token with candidates through the replay, same bits.
//
// What does not depend on earlier tokens is loaded ahead: word, old topic, position in the word-sorted order, U,
// typeNorm[w] and nw[w] 64 tokens at a time, one chunk ahead (as spalias); and the first 64 entries of a token's word list
// two tokens ahead, the Phi values at them one token ahead (used if that token takes the word's list).  The document-list
// gather cannot be: the list changes with every token.
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
};

constexpr int kWordListBlock = 256;

__global__ __launch_bounds__(kWordListBlock) void word_list_build_kernel(WordListParams p) {
  const int lane = threadIdx.x & 63, waves = kWordListBlock / 64;
  for (int64_t w = (int64_t)blockIdx.x * waves + (threadIdx.x >> 6); w < p.V; w += (int64_t)gridDim.x * waves) {
    const double *row = p.phiT + (size_t)w * p.Kp;
    uint16_t *out = p.nzw + (size_t)w * p.K;
    int n = 0;
    for (int k0 = 0; k0 < p.K; k0 += 64) {
      const int k = k0 + lane;
      const bool nz = k < p.K && row[k] != 0.0;
      const unsigned long long m = __ballot(nz);
      const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      if (nz) out[n + before] = (uint16_t)k;                                       // n + before < number of non-zeros <= K
      n += __popcll(m);
    }
    if (lane == 0) p.nw[w] = n;
  }
}

// ---- the z step ------------------------------------------------------------------------------------------------------
struct PolyaurnSparseParams {
  PcgsParams b;
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  const double *type_norm;     // [V]
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  unsigned long long *stats;   // [4]: word-list tokens, document-list tokens, uniform draws, sum of n
  int32_t cap;                 // list capacity: min(K, longest document), at least 1
  double margin_scale;         // GGS_DEBUG_MARGIN
};

inline size_t polyaurn_sparse_lds_bytes(int K, int cap) { return spalias_lds_bytes(K, cap); }

__global__ __launch_bounds__(64) void polyaurn_sparse_wave_kernel(PolyaurnSparseParams sp) {
  const PcgsParams &p = sp.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K, cap = sp.cap;
  double *cuml = reinterpret_cast<double *>(smem);                                 // [cap]
  int32_t *cnt = reinterpret_cast<int32_t *>(cuml + cap);                          // [K]
  uint16_t *pos = reinterpret_cast<uint16_t *>(cnt + K);                           // [K]
  uint16_t *list = pos + K;                                                        // [cap]

  for (int64_t di = blockIdx.x; di < p.num_docs; di += gridDim.x) {
    const int d = p.order[di];
    if (d < 0) continue;                                                           // padding of the lane-per-document kernels' list
    const int64_t beg = p.doc_ptr[d];
    const int len = (int)(p.doc_ptr[d + 1] - beg);
    if (len == 0) continue;
    __syncthreads();
    for (int k = lane; k < K; k += 64) cnt[k] = 0;
    __syncthreads();
    // the document's list in the order in which the topics first occur (as spalias_wave_kernel builds it)
    int nnz = 0;
    for (int t0 = 0; t0 < len; t0 += 64) {
      const bool live = t0 + lane < len;
      const int zt = live ? p.z[beg + t0 + lane] : -1;
      const bool fresh = live && cnt[zt] == 0;
      __builtin_amdgcn_wave_barrier();
      if (live) atomicAdd(&cnt[zt], 1);
      unsigned long long cand = __ballot(fresh);
      while (cand) {
        const int k = __builtin_amdgcn_readlane(zt, __ffsll((long long)cand) - 1);
        if (lane == 0) { list[nnz] = (uint16_t)k; pos[k] = (uint16_t)nnz; }
        nnz += 1;
        cand &= ~__ballot(zt == k);
      }
      __builtin_amdgcn_wave_barrier();
    }

    struct Chunk { int w, zold, ip, nw; double U, tn; };
    auto load_chunk = [&](int t0) {
      Chunk c{0, 0, 0, 0, 0.0, 0.0};
      const int t = t0 + lane;
      if (t < len) {
        c.w = p.tok[beg + t]; c.zold = p.z[beg + t]; c.ip = p.inv_perm[beg + t];
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        const U4 o = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), (uint32_t)GGS_PURPOSE_Z << 24, p.iteration, (uint32_t)p.seed,
                                   (uint32_t)(p.seed >> 32));
        c.U = u53(o.x, o.y);
        c.tn = sp.type_norm[c.w];
        c.nw = sp.nw[c.w];
      }
      return c;
    };
    Chunk ch = load_chunk(0), chn = len > 64 ? load_chunk(64) : ch;
    // The first 64 entries of a token's word list and phi at them, in two stages so that no load issued here depends on
    // another of the same token step (the current token's gathers queue behind them): the entries two tokens ahead
    // (nx_tp), phi at them one token ahead (pf_tp, pf_ph).  Token u's word and list length come from its chunk.
    auto word_of = [&](const int u, int &w_u, int &nw_u, const int t_now) {
      const bool same = (u >> 6) == (t_now >> 6);                                  // else the next chunk: u <= t_now + 2
      w_u = same ? __builtin_amdgcn_readlane(ch.w, u & 63) : __builtin_amdgcn_readlane(chn.w, u & 63);
      nw_u = same ? __builtin_amdgcn_readlane(ch.nw, u & 63) : __builtin_amdgcn_readlane(chn.nw, u & 63);
    };
    auto load_entries = [&](const int u, const int t_now) -> int {                 // stage 1 of token u
      if (u >= len) return 0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? (int)sp.nzw[(size_t)w_u * K + lane] : 0;
    };
    auto load_phi = [&](const int u, const int t_now, const int tp_u) -> double {  // stage 2 of token u, entries tp_u
      if (u >= len) return 0.0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? p.phiT[(size_t)w_u * p.Kp + tp_u] : 0.0;
    };
    int pf_tp = load_entries(0, 0);
    double pf_ph = load_phi(0, 0, pf_tp);
    int nx_tp = load_entries(1, 0);
    int n_word = 0, n_doc = 0, n_unif = 0;
    unsigned long long n_sum = 0;

    for (int t = 0; t < len; ++t) {
      const int tl = t & 63;
      const int w = __builtin_amdgcn_readlane(ch.w, tl), zold = __builtin_amdgcn_readlane(ch.zold, tl), ip = __builtin_amdgcn_readlane(ch.ip, tl);
      const int nww = __builtin_amdgcn_readlane(ch.nw, tl);
      const double U = read_lane(ch.U, tl), tn = read_lane(ch.tn, tl);
      const double *row = p.phiT + (size_t)w * p.Kp;
      const uint16_t *wl = sp.nzw + (size_t)w * K;
      const int my_tp = pf_tp;                                                     // this token's, loaded ahead
      const double my_ph = pf_ph;
      pf_tp = nx_tp;                                                               // token t + 1: phi at the entries loaded a step ago
      pf_ph = load_phi(t + 1, t, nx_tp);
      nx_tp = load_entries(t + 2, t);                                              // token t + 2: its entries

      // the old topic leaves; a count of 0 leaves the list, the list's last entry takes its slot
      // (one wave per workgroup: its LDS operations execute in program order; the barriers keep the COMPILER to it)
      const int c_old = __builtin_amdgcn_readfirstlane(cnt[zold]) - 1;
      int slot_old = 0, last_t = 0;
      if (c_old == 0) { slot_old = pos[zold]; last_t = list[nnz - 1]; }
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        cnt[zold] = c_old;
        if (c_old == 0) { list[slot_old] = (uint16_t)last_t; pos[last_t] = (uint16_t)slot_old; }
      }
      if (c_old == 0) nnz -= 1;
      __builtin_amdgcn_wave_barrier();

      // the shorter list; a tie goes to the document's.  n <= nnz <= cap either way
      const bool use_word = nww < nnz;
      const int n = use_word ? nww : nnz;
      // candidate e and its score, lane by lane (the word list's first block comes from the prefetch)
      auto cand_at = [&](const int e) -> int { return use_word ? (int)wl[e] : (int)list[e]; };
      auto block_scores = [&](const int base, int &tp) -> double {
        const int e = base + lane;
        const bool valid = e < n;
        if (use_word && base == 0) { tp = my_tp; return valid ? (double)cnt[tp] * my_ph : 0.0; }
        tp = cand_at(valid ? e : 0);
        return valid ? (double)cnt[tp] * row[tp] : 0.0;
      };

      int new_topic = -1;
      if (n == 0) {                                                                // no candidate: polyaurn's uniform draw
        new_topic = polyaurn_uniform_topic(U, K);
        n_unif += 1;
      } else {
        n_word += use_word ? 1 : 0;
        n_doc += use_word ? 0 : 1;
        n_sum += (unsigned long long)n;
        // PROPOSAL (header): running sums by wave scans, any association; decided only outside the margins
        double before = 0.0;
        for (int base = 0; base < n; base += 64) {
          int tp;
          const double score = block_scores(base, tp);
          const double sc = before + wave_inclusive_scan(score);
          if (base + lane < n) cuml[base + lane] = sc;
          before = read_lane(sc, 63);                                              // lanes past the list add 0.0
        }
        const double s_hat = before;
        const double eps = (double)(4 * n + 64) * 0x1p-53 * sp.margin_scale;
        const double den = tn + s_hat, thr = tn / den;                             // 0 / 0: neither comparison holds
        if (U < thr * (1.0 - eps)) {                                               // surely the alias draw
          const double x = U + (s_hat * U) / tn;
          const double ups = x * (double)K;
          const int i = (int)ups;
          const double frac = ups - (double)i, dm = (double)K * eps * (x + 1.0);
          if (i < K && frac > dm && frac < 1.0 - dm) {
            const size_t o = (size_t)w * K + i;
            const double psv = sp.ps[o];
            if (fabs(frac - psv) > dm) new_topic = frac > psv ? sp.a[o] : i;
          }
        } else if (U > thr * (1.0 + eps)) {                                        // surely the walk over the candidates
          const double ul = U * den - tn, delta = eps * den;
          __builtin_amdgcn_wave_barrier();
          for (int base = 0; base < n; base += 64) {
            const int e = base + lane;
            const unsigned long long m = __ballot(e < n && ul - cuml[e < n ? e : 0] < -delta);   // surely ul < cum[e]
            if (m) {
              const int sel = base + __ffsll((long long)m) - 1;
              if (sel == 0 || ul - cuml[sel - 1] > delta) new_topic = cand_at(sel);   // and surely past the entry before it
              break;
            }
          }
        }
        new_topic = __builtin_amdgcn_readfirstlane(new_topic);

        if (__builtin_expect(new_topic < 0, 0)) {
          // EXACT: cum[i] = cnt[c_i] * phi[c_i][w] + cum[i-1], in candidate order, one chain of fp64 adds
          __builtin_amdgcn_wave_barrier();
          double run = 0.0, mycum = 0.0;
          int mytopic = 0;
          for (int base = 0; base < n; base += 64) {
            int tp;
            const double score = block_scores(base, tp);
            const int m = min(64, n - base);
            for (int i = 0; i < m; ++i) {
              run = run + read_lane(score, i);
              mycum = lane == i ? run : mycum;
            }
            if (base == 0) mytopic = tp;
            if (n > 64 && base + lane < n) cuml[base + lane] = mycum;
          }
          const double sum = run;

          if (U < tn / (tn + sum)) {
            const double x = U + (sum * U) / tn;
            const double ups = x * (double)K;
            const int i = (int)ups;
            if (i >= K) {
              if (lane == 0) atomicOr(p.status, ST_INVALID_TOPIC);
              new_topic = K - 1;
            } else {
              const size_t o = (size_t)w * K + i;
              new_topic = (ups - (double)i) > sp.ps[o] ? sp.a[o] : i;
            }
          } else {
            const double ul = U * (tn + sum) - tn;
            if (n <= 64) {
              const unsigned long long m = __ballot(lane < n && ul <= mycum);
              new_topic = __builtin_amdgcn_readlane(mytopic, m ? __ffsll((long long)m) - 1 : n - 1);
            } else {
              __builtin_amdgcn_wave_barrier();
              int sel = n - 1;
              for (int base = 0; base < n; base += 64) {
                const int e = base + lane;
                const unsigned long long m = __ballot(e < n && ul <= cuml[e < n ? e : 0]);
                if (m) { sel = base + __ffsll((long long)m) - 1; break; }
              }
              new_topic = cand_at(sel);
            }
          }
          new_topic = __builtin_amdgcn_readfirstlane(new_topic);
        }
      }

      const int c_new = __builtin_amdgcn_readfirstlane(cnt[new_topic]);
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        cnt[new_topic] = c_new + 1;
        if (c_new == 0) { list[nnz] = (uint16_t)new_topic; pos[new_topic] = (uint16_t)nnz; }
        p.z[beg + t] = new_topic;
        p.zw[ip] = new_topic;
      }
      if (c_new == 0) nnz += 1;
      __builtin_amdgcn_wave_barrier();

      if (tl == 63) {
        ch = chn;
        if (t + 1 + 64 < len) chn = load_chunk(t + 1 + 64);
      }
    }
    if (lane == 0) {                                                               // once per document
      if (n_word) atomicAdd(&sp.stats[0], (unsigned long long)n_word);
      if (n_doc) atomicAdd(&sp.stats[1], (unsigned long long)n_doc);
      if (n_unif) atomicAdd(&sp.stats[2], (unsigned long long)n_unif);
      if (n_sum) atomicAdd(&sp.stats[3], n_sum);
    }
  }
}

}  // namespace ggs
