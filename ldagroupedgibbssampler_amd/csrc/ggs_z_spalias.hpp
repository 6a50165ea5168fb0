// ggs_z_spalias.hpp -- the z loop of scheme=spalias (SpaliasUncollapsedParallelLDA.java:124-242, sampleNewTopic :277-293):
// the pcgs conditional (n_dk + alpha_k) * phi[k][w] split into alpha_k * phi[k][w], drawn in O(1) from the word's alias
// table (ggs_alias.hpp), and n_dk * phi[k][w], which is non-zero only for the topics the document uses: O(nnz_d) per
// token instead of O(K).  The kernel's body, sparse_wave_body, is also polyaurn_sparse's (ggs_z_polyaurn_sparse.hpp),
// which walks the word's list of topics with phi != 0 instead wherever that list is the shorter one.
//
// One WAVE per document (documents are independent given Phi, the tokens of a document strictly sequential), one
// single-wave workgroup per wave, a persistent grid over the length-sorted document list of the pcgs kernels.  On chip
// (LDS) per wave: the document's topic counts int32 [K], the list of its non-zero topics u16 [cap] in the reference's
// discipline (filled by walking the tokens in order, a topic appended when its count becomes 1; a topic whose count
// falls to 0 replaced by the list's last entry), the back-mapping topic -> list slot u16 [K], and the running sums
// fp64 [cap]; cap = min(K, longest document).
//
// Per token (old topic removed first) there are n candidates c_0 .. c_{n-1}.  For spalias they are the document's list
// and n = nnz, its length; for polyaurn_sparse the shorter of that list and the word's, so n <= nnz <= cap either way.
// Lane i of each block of 64 candidates gathers phiT[w][c_i] and forms cnt[c_i] * phi (count converted to double, one
// multiply; a candidate the document does not use scores 0.0).  The reference's running sum cum[i] = score_i + cum[i-1]
// is a sequential chain of fp64 adds; as ONE chain executed on values read lane by lane out of the registers
// (v_readlane) it costs about 55 cycles of a SIMD's issue per candidate (measured: 46 ms per z step at K = 1024,
// nnz_d = 100, against 15 for the dense pcgs kernel), so, as in ggs_z_pcgs_wave.hpp, wave scans only PROPOSE and the
// chain is the replay:
//   the scores are non-negative, so every partial sum of the n scores, in whatever association, and every chain value
//   of Java's are within n * 2^-53 * S of the real prefix (S = the real sum), and they differ by at most 2 n 2^-53 S;
//   with eps = (4 n + 64) * 2^-53 (more than twice every bound below):
//   - Java's threshold tn / (tn + sum) is within (2 n + 4) 2^-53 (relative) of this kernel's thr: U < thr (1 - eps)
//     proves the alias branch, U > thr (1 + eps) the other;
//   - alias branch: Java's ups = (U + sum U / tn) K is within K x (2 n + 4) 2^-53 of this kernel's; with
//     dm = K eps (x + 1), a fractional part more than dm away from 0, 1 and ps[w][i] proves both i and the comparison;
//   - list branch: Java's ul and cum[i] are each within (2 n + 6) 2^-53 (tn + S) of this kernel's; with
//     delta = eps (tn + S'), the first entry with ul' - cum'[i] < -delta is Java's entry provided the entry before it
//     has ul' - cum'[i-1] > delta (the real prefixes are monotone; zero scores leave equal neighbours, which the second
//     test then refuses: such a token is replayed).
// A token that is not decided (about n * 2^-45 of them), and everything Java would throw on, is replayed exactly, by ONE
// chain of fp64 adds in candidate order.  GGS_DEBUG_MARGIN scales eps up: the tests send every token through the replay,
// and both ways give the restatement's bits.  In the replay, with tn = typeNorm[w], sum = cum[n-1] (0.0 without
// candidates) and the token's uniform U:
//   U < tn / (tn + sum):  x = U + (sum * U) / tn, ups = x * K, i = (int)ups, topic = (ups - i) > ps[w][i] ? a[w][i] : i
//                         (i == K: GGS_ERR_INVALID_TOPIC, as a pcgs walk that runs past K);
//   else                  ul = U * (tn + sum) - tn, topic = c_i at the smallest i with ul <= cum[i] (a ballot), c_{n-1}
//                         if there is none.
// Without candidates (n == 0; polyaurn_sparse has its own rule, in its header) spalias's token goes through the same
// lines: the proposal may prove the alias branch (its list branch asks for n > 0), and in the replay tn > 0 makes the
// threshold 1.0 > U, the alias draw at x = U, while tn == 0 (0 / 0 fails the comparison) keeps the old topic -- reached
// by a one-token document of a word whose Phi column ggs_set_phi has zeroed.
// Everything a token needs that does not depend on earlier tokens -- word, old topic, position in the word-sorted
// order, U (Philox), typeNorm[w] -- is loaded 64 tokens at a time, one chunk ahead, as in the pcgs wave kernel.
#pragma once
#include "ggs_z_pcgs.hpp"

namespace ggs {

struct SpaliasParams {          // PolyaurnSparseParams (ggs_z_polyaurn_sparse.hpp) adds the words' lists and the counters
  PcgsParams b;
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  const double *type_norm;     // [V]
  int32_t cap;                 // list capacity: min(K, longest document), at least 1
  double margin_scale;         // GGS_DEBUG_MARGIN: scales the certainty margins (tests send every token through the exact chain)
};

inline size_t spalias_lds_bytes(int K, int cap) { return (size_t)cap * 8 + (size_t)K * 4 + (size_t)K * 2 + (size_t)((cap + 3) & ~3) * 2; }

// WORD_LISTS: polyaurn_sparse (Params = PolyaurnSparseParams: the words' lists exist, the counters are kept); without:
// spalias (SpaliasParams).  Every difference between the two is an `if constexpr (WORD_LISTS)` or a condition on it below.
// N0_ALIAS (nzvsspalias, with WORD_LISTS): a token without a candidate draws sample(w, U) from its word's alias table instead of
// polyaurn's floor(U * K); a draw with i == K is GGS_ERR_INVALID_TOPIC.
template <bool WORD_LISTS, class Params, bool N0_ALIAS = false>
__device__ __forceinline__ void sparse_wave_body(const Params &sp) {
  const PcgsParams &p = sp.b;
  const uint16_t *nzw = nullptr;                                                   // [V][K]: the words' lists,
  const int32_t *nw = nullptr;                                                     // [V]: their lengths
  if constexpr (WORD_LISTS) { nzw = sp.nzw; nw = sp.nw; }
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
    // the list in the order in which the topics first occur: a chunk's candidates (count 0 before the chunk) are taken in
    // lane order, one distinct topic at a time
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

    struct Chunk { int w, zold, ip, nw; double U, tn; };                           // nw: the word list's length (WORD_LISTS)
    auto load_chunk = [&](int t0) {
      Chunk c{0, 0, 0, 0, 0.0, 0.0};
      const int t = t0 + lane;
      if (t < len) {
        c.w = p.tok[beg + t]; c.zold = p.z[beg + t]; c.ip = p.inv_perm[beg + t];
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        c.U = z_uniform(gtok, p.iteration, p.seed);
        c.tn = sp.type_norm[c.w];
        if constexpr (WORD_LISTS) c.nw = nw[c.w];
      }
      return c;
    };
    Chunk ch = load_chunk(0), chn = len > 64 ? load_chunk(64) : ch;
    // WORD_LISTS: the first 64 entries of a token's word list and phi at them are loaded ahead too (the document-list
    // gather cannot be: the list changes with every token), in two stages so that no load issued here depends on another
    // of the same token step (the current token's gathers queue behind them): the entries two tokens ahead (nx_tp), phi
    // at them one token ahead (pf_tp, pf_ph).  Token u's word and list length come from its chunk.
    auto word_of = [&](const int u, int &w_u, int &nw_u, const int t_now) {
      const bool same = (u >> 6) == (t_now >> 6);                                  // else the next chunk: u <= t_now + 2
      w_u = same ? __builtin_amdgcn_readlane(ch.w, u & 63) : __builtin_amdgcn_readlane(chn.w, u & 63);
      nw_u = same ? __builtin_amdgcn_readlane(ch.nw, u & 63) : __builtin_amdgcn_readlane(chn.nw, u & 63);
    };
    auto load_entries = [&](const int u, const int t_now) -> int {                 // stage 1 of token u
      if (u >= len) return 0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? (int)nzw[(size_t)w_u * K + lane] : 0;
    };
    auto load_phi = [&](const int u, const int t_now, const int tp_u) -> double {  // stage 2 of token u, entries tp_u
      if (u >= len) return 0.0;
      int w_u, nw_u;
      word_of(u, w_u, nw_u, t_now);
      return lane < nw_u ? p.phiT[(size_t)w_u * p.Kp + tp_u] : 0.0;
    };
    int pf_tp = 0, nx_tp = 0;
    double pf_ph = 0.0;
    if constexpr (WORD_LISTS) {
      pf_tp = load_entries(0, 0);
      pf_ph = load_phi(0, 0, pf_tp);
      nx_tp = load_entries(1, 0);
    }
    int n_word = 0, n_doc = 0, n_unif = 0;                                         // ggs_get_sparse_stats (WORD_LISTS): in registers,
    unsigned long long n_sum = 0;                                                  // added once per document

    for (int t = 0; t < len; ++t) {
      const int tl = t & 63;
      const int w = __builtin_amdgcn_readlane(ch.w, tl), zold = __builtin_amdgcn_readlane(ch.zold, tl), ip = __builtin_amdgcn_readlane(ch.ip, tl);
      const double U = read_lane(ch.U, tl), tn = read_lane(ch.tn, tl);
      const double *row = p.phiT + (size_t)w * p.Kp;
      const uint16_t *wl = nullptr;                                                // the word's list
      int nww = 0, my_tp = 0;
      double my_ph = 0.0;
      if constexpr (WORD_LISTS) {
        wl = nzw + (size_t)w * K;
        nww = __builtin_amdgcn_readlane(ch.nw, tl);
        my_tp = pf_tp;                                                             // this token's, loaded ahead
        my_ph = pf_ph;
        pf_tp = nx_tp;                                                             // token t + 1: phi at the entries loaded a step ago
        pf_ph = load_phi(t + 1, t, nx_tp);
        nx_tp = load_entries(t + 2, t);                                            // token t + 2: its entries
      }

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

      // the candidates: the document's list, or (WORD_LISTS) the shorter one, a tie going to the document's
      const bool use_word = WORD_LISTS && nww < nnz;
      const int n = use_word ? nww : nnz;
      // candidate e and a block's scores, lane by lane (the word list's first block comes from the prefetch)
      auto cand_at = [&](const int e) -> int { return use_word ? (int)wl[e] : (int)list[e]; };
      auto block_scores = [&](const int base, int &tp) -> double {
        const int e = base + lane;
        const bool valid = e < n;
        if (use_word && base == 0) { tp = my_tp; return valid ? (double)cnt[tp] * my_ph : 0.0; }
        tp = cand_at(valid ? e : 0);
        return valid ? (double)cnt[tp] * row[tp] : 0.0;
      };

      int new_topic = -1;
      if (WORD_LISTS && n == 0) {                                                  // no candidate: polyaurn's uniform draw, or (N0_ALIAS) the word's alias table
        if constexpr (N0_ALIAS) {
          const double ups = U * (double)K;
          const int i = (int)ups;
          if (i >= K) {
            if (lane == 0) atomicOr(p.status, ST_INVALID_TOPIC);
            new_topic = K - 1;
          } else {
            const size_t o = (size_t)w * K + i;
            new_topic = (ups - (double)i) > sp.ps[o] ? sp.a[o] : i;
          }
        } else {
          new_topic = polyaurn_uniform_topic(U, K);
        }
        n_unif += 1;
      } else {
        if constexpr (WORD_LISTS) {
          n_word += use_word ? 1 : 0;
          n_doc += use_word ? 0 : 1;
          n_sum += (unsigned long long)n;
        }
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
        } else if (U > thr * (1.0 + eps) && (WORD_LISTS || n > 0)) {               // surely the walk over the candidates
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
            if (!WORD_LISTS && n == 0) {                                           // needs tn == 0 (header)
              new_topic = zold;
            } else if (n <= 64) {
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
    if constexpr (WORD_LISTS) {
      if (lane == 0) {                                                             // once per document
        if (n_word) atomicAdd(&sp.stats[0], (unsigned long long)n_word);
        if (n_doc) atomicAdd(&sp.stats[1], (unsigned long long)n_doc);
        if (n_unif) atomicAdd(&sp.stats[2], (unsigned long long)n_unif);
        if (n_sum) atomicAdd(&sp.stats[3], n_sum);
      }
    }
  }
}

__global__ __launch_bounds__(64) void spalias_wave_kernel(SpaliasParams sp) { sparse_wave_body<false>(sp); }

}  // namespace ggs
