// ggs_z_adlda.hpp -- scheme=adlda (ParallelLDA.java:409-412, ADLDA; its worker MyWorkerRunnable.sampleTopicsForOneDoc,
// MyWorkerRunnable.java:32-409): the SparseLDA decomposition of Yao, Mimno and McCallum over the COLLAPSED model.  No theta,
// no Phi: the state is z, the type-topic counts and tokensPerTopic.  The conditional
//     (alpha_k + n_dk) (beta + n_wk) / (betaSum + n_k)
// is split into a smoothing mass alpha_k beta / den(k), nearly constant over a sweep, a document mass beta n_dk / den(k) over
// the document's non-zero topics and a word mass (alpha_k + n_dk) n_wk / den(k) over the word's non-zero topics: the exact
// conditional of scheme=collapsed's parallel schedule at O(nnz_d + nnz_w) per token, and no V x K fp64 matrix.
//
// The schedule is scheme=collapsed's parallel one: AD-LDA with one worker per document, every document
// sampled against the counts N[w][k], T[k] as they stood at the start of the sweep, minus the token being resampled; the
// merge is the (word, z) histogram of the new assignments.
//
// At the sweep head (adlda_head_kernel, and word_list_build_kernel's body over the counts):
//     den0[k] = (double)T[k] + betaSum
//     S0      = the sum over k = 0 .. K-1, in k order from 0.0, of (alpha_k * beta) / den0[k]          (smoothingOnlyMass)
//     L_w     = the ascending list of the topics with N[w][k] > 0, and its length
// Per token: word w, old topic z0, one uniform U (the first of Philox block 0 of the token's Z stream, as pcgs takes it).
// Counts are converted to double before any arithmetic; every expression associates left to right.
//   1. n_d[z0]--; a count of 0 leaves the document's list (ggs_z_spalias.hpp's discipline: first-occurrence order, the last
//      entry fills the hole).
//   2. T'(k) = T[k] - [k == z0], G'(k) = N[w][k] - [k == z0], den(k) = (double)T'(k) + betaSum.  An earlier token of the
//      same document moves neither T nor N.
//   3. S = S0 - (alpha_z0 * beta) / den0[z0] + (alpha_z0 * beta) / den(z0)                                (:102-103, 145-146)
//   4. R = the sum over the document's list, in list order from 0.0, of (beta * n_d[c]) / den(c)          (:76, 104-105)
//   5. Q = the sum over L_w, in list order from 0.0, of score_j = ((alpha_k + n_d[k]) / den(k)) * G'(k), k the j-th entry
//      (:79, 206-209).  The entry z0 with N[w][z0] == 1 scores 0.0 and stays in the list.
//   6. sample = U * (S + R + Q)                                                                            (:215)
//   7. sample < Q (:221-246): i = -1; while sample > 0: i++, sample -= score_i; the topic is L_w[i].  A walk that runs past
//      the last entry is GGS_ERR_INVALID_TOPIC, the topic clamped to the last entry.
//      Else sample -= Q; sample < R (:250-266): sample /= beta; over the document's list in order sample -= n_d[c] / den(c),
//      the topic the first c with sample <= 0.0; K - 1 if there is none (:332-336), without an error.
//      Else sample -= R (:268-285): sample /= beta; k = 0, sample -= alpha_0 / den(0); while sample > 0.0: k++,
//      sample -= alpha_k / den(k).  k == K is GGS_ERR_INVALID_TOPIC, the topic clamped to K - 1.
//   8. n_d[new]++, into the list if the count became 1, z = new.
// Deviations from the reference (none changes the conditional): the word's candidates in ascending topic order,
// not MALLET's count-descending packed order; the document's candidates in spalias's list order; S, R and the coefficients
// formed afresh for each token from sweep-start quantities, never carried along; one worker per document; no
// hyper-parameter optimisation.
//
// The kernel: one WAVE per document over the pcgs kernels' length-sorted list, single-wave persistent workgroups.  LDS per
// wave: den0 and alpha fp64 [K] (loaded once per workgroup), the document's counts int32 [K], its list u16 [cap] and
// back-map u16 [K] as in sparse_wave_body, and one block of 64 fp64 terms.  Everything a token needs that does not depend on
// the tokens before it -- word, z0, word-sorted position, U, nnz_w, den(z0) and S (three operations on sweep-start
// quantities: computed per token, exactly, never as a running difference) -- is loaded 64 tokens at a time, one chunk ahead;
// the first 64 entries of a token's L_w come two tokens ahead, the N[w][.] cells at them one token ahead (sweep-start
// counts: nothing this sweep writes).  The kernel reads L_w and the nnz_w matching cells of N[w][.], never a K-wide row of
// global memory; the S walk reads alpha and den0 out of LDS.
// The three sequential fp64 chains (the sums R and Q, the bucket's walk) cost a dependent add per candidate; as in
// ggs_z_spalias.hpp wave scans only PROPOSE and one exact pass is the replay.  With u = 2^-53, n = nnz_w + nnz_d, all
// terms non-negative (S is formed exactly per token, the same bits on both paths, and is positive) and T = S + R + Q:
//   a sum of m non-negative terms in any association, and the reference's chain, are each within m u of the real sum
//   (relative), so the scans' Rh, Qh are within 2 nnz_d u R and 2 nnz_w u Q of the chains' R, Q; Th = S + Rh + Qh within
//   (2 n + 4) u T of T; sh = U * Th within (2 n + 6) u T of sample; s1h = sh - Qh within (4 n + 8) u T of sample - Q;
//   a walk's value after entry i is within (n + 5) u T of (its start minus the real prefix) -- the R walk in units of
//   beta: it divides the start by beta once and subtracts n_d[c] / den(c), each within 3 u of (beta n_d[c]) / den(c) / beta
//   -- and the proposal's start - scan prefix within (5 n + 9) u T of the same: they differ by at most (6 n + 14) u T.
//   With delta = (8 n + 64) u Th, more than every bound above (and than the sum of any two the decisions combine):
//   - sh < Qh - delta proves sample < Q; sh > Qh + delta disproves it; then s1h < Rh - delta proves sample - Q < R.  The
//     smoothing bucket is not proposed: it goes to the replay (its walk reads LDS only).
//   - in the proven bucket the first entry e with start - prefix[e] < -delta is the reference's entry provided e == 0
//     or start - prefix[e-1] > delta: the walk is surely still positive behind e - 1 (the real prefixes are monotone,
//     so behind every earlier entry too) and surely not behind e.  Zero scores leave equal neighbours, which the second
//     test refuses; a walk that would run past the last entry finds no e: both go to the replay, as does everything
//     the reference would raise on.
// The replay runs the chains EXACTLY as written: a block of 64 terms is formed lane-parallel (the divisions), stored to
// LDS, and every lane then runs the one chain of fp64 adds (or the walk's subtractions) over the block out of LDS --
// broadcast reads, which the compiler batches, where a chain on v_readlane costs about 55 cycles per candidate.  A walk
// re-forms its bucket's terms block by block (the same operations on the same operands: the same bits) and stops in the
// block where it ends.  GGS_DEBUG_MARGIN scales delta up: the tests send every token through the replay, and both ways
// give the restatement's bits.
// Counters (ggs_get_sparse_stats): tokens drawn from Q, from R, from S, and the sum of nnz_w + nnz_d (the document's list
// after the removal) over all tokens; kept in registers and added once per document.
#pragma once
#include "ggs_z_polyaurn_sparse.hpp"

namespace ggs {

// ---- the sweep head ------------------------------------------------------------------------------------------------------
struct AdldaHeadParams {
  const int32_t *n_k;          // [K] sweep-start tokensPerTopic
  const double *alpha;         // [K]
  double *den0;                // [K]
  double *s0;                  // [1]
  double beta, beta_sum;
  int32_t K;
};

// One wave: a block of 64 terms lane-parallel, then the k-order chain over the block out of LDS.
__global__ __launch_bounds__(64) void adlda_head_kernel(AdldaHeadParams p) {
  __shared__ double buf[64];
  const int lane = threadIdx.x;
  double run = 0.0;
  for (int k0 = 0; k0 < p.K; k0 += 64) {
    const int k = k0 + lane, m = min(64, p.K - k0);
    if (k < p.K) {
      const double den = (double)p.n_k[k] + p.beta_sum;
      p.den0[k] = den;
      buf[lane] = (p.alpha[k] * p.beta) / den;
    }
    __syncthreads();
    for (int i = 0; i < m; ++i) run = run + buf[i];
    __syncthreads();
  }
  if (lane == 0) p.s0[0] = run;
}

// ---- the z step ----------------------------------------------------------------------------------------------------------
struct AdldaParams {
  PcgsParams b;                // n_wk, n_k: the sweep-start counts; alpha, beta, beta_sum
  const double *den0;          // [K]
  const double *s0;            // [1]
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  unsigned long long *stats;   // [4]: tokens from Q, from R, from S; the sum of nnz_w + nnz_d
  int32_t cap;                 // the document list's capacity: min(K, longest document), at least 1
  double margin_scale;         // GGS_DEBUG_MARGIN: scales the certainty margins (tests send every token through the exact chains)
};

// den0 [K] f64 | alpha [K] f64 | buf [64] f64 | cnt [K] i32 | pos [K] u16 | list [cap] u16
inline size_t adlda_lds_bytes(int K, int cap) { return (size_t)K * 16 + 64 * 8 + (size_t)K * 4 + (size_t)K * 2 + (size_t)((cap + 3) & ~3) * 2; }

__global__ __launch_bounds__(64) void adlda_wave_kernel(AdldaParams ap) {
  const PcgsParams &p = ap.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K;
  const double beta = p.beta, bS = p.beta_sum;
  double *den0 = reinterpret_cast<double *>(smem);                                 // [K]
  double *alpha = den0 + K;                                                        // [K]
  double *buf = alpha + K;                                                         // [64]
  int32_t *cnt = reinterpret_cast<int32_t *>(buf + 64);                            // [K]
  uint16_t *pos = reinterpret_cast<uint16_t *>(cnt + K);                           // [K]
  uint16_t *list = pos + K;                                                        // [cap]

  for (int k = lane; k < K; k += 64) { den0[k] = ap.den0[k]; alpha[k] = p.alpha[k]; }
  const double S0 = ap.s0[0];

  for (int64_t di = blockIdx.x; di < p.num_docs; di += gridDim.x) {
    const int d = p.order[di];
    if (d < 0) continue;                                                           // padding of the lane-per-document kernels' list
    const int64_t beg = p.doc_ptr[d];
    const int len = (int)(p.doc_ptr[d + 1] - beg);
    if (len == 0) continue;
    __syncthreads();
    for (int k = lane; k < K; k += 64) cnt[k] = 0;
    __syncthreads();
    // the list in the order in which the topics first occur (as sparse_wave_body)
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

    struct Chunk { int w, z0, ip, nw; double U, denz, S; };                        // denz = den(z0); S: step 3
    auto load_chunk = [&](int t0) {
      Chunk c{0, 0, 0, 0, 0.0, 1.0, 0.0};
      const int t = t0 + lane;
      if (t < len) {
        c.w = p.tok[beg + t]; c.z0 = p.z[beg + t]; c.ip = p.inv_perm[beg + t];
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        c.U = z_uniform(gtok, p.iteration, p.seed);
        c.nw = ap.nw[c.w];
        c.denz = (double)(p.n_k[c.z0] - 1) + bS;
        const double ab = alpha[c.z0] * beta;
        c.S = S0 - ab / den0[c.z0] + ab / c.denz;
      }
      return c;
    };
    Chunk ch = load_chunk(0), chn = len > 64 ? load_chunk(64) : ch;
    // the first 64 entries of token u's word list two tokens ahead (nx_tp), the counts at them one token ahead (pf_tp, pf_g)
    auto word_of = [&](const int u, int &w_u, int &nw_u, const int t_now) {
      const bool same = (u >> 6) == (t_now >> 6);                                  // else the next chunk: u <= t_now + 2
      w_u = same ? __builtin_amdgcn_readlane(ch.w, u & 63) : __builtin_amdgcn_readlane(chn.w, u & 63);
      nw_u = same ? __builtin_amdgcn_readlane(ch.nw, u & 63) : __builtin_amdgcn_readlane(chn.nw, u & 63);
    };
    auto load_entries = [&](const int u, const int t_now) -> int {
      if (u >= len) return 0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? (int)ap.nzw[(size_t)w_u * K + lane] : 0;
    };
    auto load_cells = [&](const int u, const int t_now, const int tp_u) -> int {
      if (u >= len) return 0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? p.n_wk[(size_t)w_u * K + tp_u] : 0;
    };
    int pf_tp = load_entries(0, 0);
    int pf_g = load_cells(0, 0, pf_tp);
    int nx_tp = load_entries(1, 0);
    int n_q = 0, n_r = 0, n_s = 0;
    unsigned long long n_sum = 0;

    for (int t = 0; t < len; ++t) {
      const int tl = t & 63;
      const int w = __builtin_amdgcn_readlane(ch.w, tl), z0 = __builtin_amdgcn_readlane(ch.z0, tl), ip = __builtin_amdgcn_readlane(ch.ip, tl);
      const int nww = __builtin_amdgcn_readlane(ch.nw, tl);
      const double U = read_lane(ch.U, tl), denz = read_lane(ch.denz, tl), S = read_lane(ch.S, tl);
      const uint16_t *wl = ap.nzw + (size_t)w * K;
      const int32_t *nrow = p.n_wk + (size_t)w * K;
      const int my_tp = pf_tp, my_g = pf_g;                                        // this token's, loaded ahead
      pf_tp = nx_tp;
      pf_g = load_cells(t + 1, t, nx_tp);
      nx_tp = load_entries(t + 2, t);

      // 1. the old topic leaves; a count of 0 leaves the list, the list's last entry takes its slot
      // (one wave per workgroup: its LDS operations execute in program order; the barriers keep the COMPILER to it)
      const int c_old = __builtin_amdgcn_readfirstlane(cnt[z0]) - 1;
      int slot_old = 0, last_t = 0;
      if (c_old == 0) { slot_old = pos[z0]; last_t = list[nnz - 1]; }
      __builtin_amdgcn_wave_barrier();
      if (lane == 0) {
        cnt[z0] = c_old;
        if (c_old == 0) { list[slot_old] = (uint16_t)last_t; pos[last_t] = (uint16_t)slot_old; }
      }
      if (c_old == 0) nnz -= 1;
      __builtin_amdgcn_wave_barrier();
      n_sum += (unsigned long long)(nww + nnz);

      // a block of 64 terms, lane by lane; lanes past the bucket's end hold 0.0 and are never read by a chain
      auto den_of = [&](const int k) -> double { return k == z0 ? denz : den0[k]; };
      auto q_terms = [&](const int base) -> double {                               // step 5
        const int e = base + lane;
        if (e >= nww) return 0.0;
        int k, g;
        if (base == 0) { k = my_tp; g = my_g; } else { k = (int)wl[e]; g = nrow[k]; }
        g -= k == z0 ? 1 : 0;
        return ((alpha[k] + (double)cnt[k]) / den_of(k)) * (double)g;
      };
      auto r_terms = [&](const int base, const bool walk) -> double {              // step 4, or the R walk's n_d[c] / den(c)
        const int e = base + lane;
        if (e >= nnz) return 0.0;
        const int c = (int)list[e];
        const double n = (double)cnt[c];
        return walk ? n / den_of(c) : (beta * n) / den_of(c);
      };
      auto s_terms = [&](const int base) -> double {                               // the S walk's alpha_k / den(k)
        const int k = base + lane;
        return k < K ? alpha[k] / den_of(k) : 0.0;
      };
      auto put = [&](const double v) {
        __builtin_amdgcn_wave_barrier();
        buf[lane] = v;
        __builtin_amdgcn_wave_barrier();
      };

      int new_topic = -1, bucket = 2;
      {
        // PROPOSAL (header): the sums by wave scans, any association; a bucket and an entry are taken only outside the margins
        double Rh = 0.0, Qh = 0.0;
        for (int base = 0; base < nnz; base += 64) Rh += read_lane(wave_inclusive_scan(r_terms(base, false)), 63);
        for (int base = 0; base < nww; base += 64) Qh += read_lane(wave_inclusive_scan(q_terms(base)), 63);
        const double Th = S + Rh + Qh, sh = U * Th;
        const double delta = ((double)(8 * (nww + nnz) + 64) * 0x1p-53 * ap.margin_scale) * Th;
        // the first entry e of a bucket of n entries with (start - prefix[e]) surely negative, taken if the entry before it
        // is surely positive (the real prefixes are monotone; equal neighbours -- a zero score -- refuse it)
        auto decide = [&](const double start, const int n, auto terms) -> int {
          double before = 0.0;
          for (int base = 0; base < n; base += 64) {
            const double sc = before + wave_inclusive_scan(terms(base));
            const double dd = start - sc;
            const unsigned long long m = __ballot(base + lane < n && dd < -delta);
            if (m) {
              const int l = __ffsll((long long)m) - 1;
              const double prev = l == 0 ? start - before : read_lane(dd, l - 1);
              return (base + l == 0 || prev > delta) ? base + l : -1;
            }
            before = read_lane(sc, 63);                                            // lanes past the bucket add 0.0
          }
          return -1;
        };
        if (Th < __builtin_huge_val() && delta < Th) {
          if (sh < Qh - delta) {                                                   // surely the word's bucket
            const int sel = decide(sh, nww, [&](const int base) { return q_terms(base); });
            if (sel >= 0) { new_topic = min((int)wl[sel], K - 1); bucket = 0; }
          } else if (sh > Qh + delta) {
            const double s1 = sh - Qh;
            if (s1 < Rh - delta) {                                                 // surely the document's
              const int sel = decide(s1, nnz, [&](const int base) { return r_terms(base, false); });
              if (sel >= 0) { new_topic = (int)list[sel]; bucket = 1; }
            }
          }
        }
        new_topic = __builtin_amdgcn_readfirstlane(new_topic);
      }

      if (__builtin_expect(new_topic < 0, 0)) {
      // EXACT: the three chains as written, one fp64 operation after the other
      double R = 0.0, Q = 0.0;
      for (int base = 0; base < nnz; base += 64) {
        put(r_terms(base, false));
        const int m = min(64, nnz - base);
        for (int i = 0; i < m; ++i) R = R + buf[i];
      }
      for (int base = 0; base < nww; base += 64) {
        put(q_terms(base));
        const int m = min(64, nww - base);
        for (int i = 0; i < m; ++i) Q = Q + buf[i];
      }
      double sample = U * (S + R + Q);                                             // 6.

      if (sample < Q) {                                                            // 7. the word's bucket
        bucket = 0;
        int sel = -1;
        for (int base = 0; base < nww && sel < 0; base += 64) {
          put(q_terms(base));
          const int m = min(64, nww - base);
          for (int i = 0; i < m; ++i) {
            if (!(sample > 0.0)) { sel = max(base + i - 1, 0); break; }
            sample -= buf[i];
          }
        }
        if (sel < 0) {
          if (sample > 0.0 || nww <= 0) {                                          // past the last entry
            if (lane == 0) atomicOr(p.status, ST_INVALID_TOPIC);
          }
          sel = max(nww - 1, 0);
        }
        sel = __builtin_amdgcn_readfirstlane(sel);
        new_topic = min((int)wl[sel], K - 1);
      } else {
        sample -= Q;
        if (sample < R) {                                                          // the document's bucket
          bucket = 1;
          sample /= beta;
          int sel = -1;
          for (int base = 0; base < nnz && sel < 0; base += 64) {
            put(r_terms(base, true));
            const int m = min(64, nnz - base);
            for (int i = 0; i < m; ++i) {
              sample -= buf[i];
              if (sample <= 0.0) { sel = base + i; break; }
            }
          }
          sel = __builtin_amdgcn_readfirstlane(sel);
          new_topic = sel < 0 ? K - 1 : (int)list[sel];
        } else {                                                                   // the smoothing bucket
          bucket = 2;
          sample -= R;
          sample /= beta;
          int sel = -1;
          for (int base = 0; base < K && sel < 0; base += 64) {
            put(s_terms(base));
            const int m = min(64, K - base);
            for (int i = 0; i < m; ++i) {
              sample -= buf[i];
              if (!(sample > 0.0)) { sel = base + i; break; }
            }
          }
          sel = __builtin_amdgcn_readfirstlane(sel);
          if (sel < 0) {
            if (lane == 0) atomicOr(p.status, ST_INVALID_TOPIC);
            sel = K - 1;
          }
          new_topic = sel;
        }
      }
      new_topic = __builtin_amdgcn_readfirstlane(new_topic);
      }
      n_q += bucket == 0 ? 1 : 0;
      n_r += bucket == 1 ? 1 : 0;
      n_s += bucket == 2 ? 1 : 0;

      // 8.
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
      if (n_q) atomicAdd(&ap.stats[0], (unsigned long long)n_q);
      if (n_r) atomicAdd(&ap.stats[1], (unsigned long long)n_r);
      if (n_s) atomicAdd(&ap.stats[2], (unsigned long long)n_s);
      if (n_sum) atomicAdd(&ap.stats[3], n_sum);
    }
  }
}

}  // namespace ggs
