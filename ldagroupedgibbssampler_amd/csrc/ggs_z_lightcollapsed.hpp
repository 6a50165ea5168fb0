// ggs_z_lightcollapsed.hpp -- scheme=lightcollapsed (CollapsedLightLDA.java; ParallelLDA.java:429-433): the LightLDA sampler of
// Yuan et al. over the COLLAPSED model.  No theta, no Phi: the state is z, the type-topic counts and tokensPerTopic.  Per
// token two Metropolis-Hastings proposals, one from the word's alias table over the counts and one from the document's own
// indicator array, each accepted on a product of a handful of quotients: O(1) per token, whatever K.
//
// The schedule is scheme=collapsed's parallel one: AD-LDA with one worker per document.  The reference gives
// every document batch a private copy of typeTopicCounts / tokensPerTopic (CollapsedLightLDA.java:795-802) and moves it with
// balanceGlobalCounts (:1130-1135); with one document per worker and the rule of the collapsed schedule -- a document is
// sampled against the counts as they stood at the start of the sweep, minus the token being resampled -- that copy shrinks
// to the sweep-start counts with the token in flight moved.  While a token of word w is processed, z0 its old topic and s its
// current one (z0, or an accepted word proposal):
//     G(k) = n_wk[start][w][k] - [k == z0] + [k == s]      stands for globalTypeTopicCounts[type][k]
//     T(k) = n_k[start][k]     - [k == z0] + [k == s]      stands for globalTokensPerTopic[k]
// Earlier tokens of the same document do not move G or T.  n[k] is the document's histogram with the token in flight (at s)
// and ni[k] = n[k] - [k == s]; both run along the document as in the reference (localTopicCounts, localTopicCounts_i).
//
// Per token, (U1, U2, U3, U4) its uniforms, b = beta, bS = betaSum = beta * V, counts converted to double first, the quotients
// multiplied left to right as calculateWordAcceptanceProbability (:1094-1128) and calculateDocumentAcceptanceProbability
// (:1050-1091) multiply them:
//   word proposal  u_w = U1 * (tokensPerType[w] + beta * K).  u_w < tokensPerType[w]: t = list_w[generateSample(u_w /
//                  tokensPerType[w])] on the word's table of nnz_w entries (ups = u * nnz, i = (int)ups, (ups - i) > ps[i] ?
//                  a[i] : i); otherwise t = (int)(((u_w - tokensPerType[w]) / (beta * K)) * K) (:946-954).  If t != z0, with
//                  s = z0 and a = alpha[z0]:
//                    pi_w = (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1)) * (bS + (T(s) - 1)) / (bS + T(t))
//                                                     * (b + G(s)) / (b + G(t))       * (bS + T(t)) / (bS + T(s))
//                  accepted if pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--, n[t]++, s = t (G and T follow by definition).
//   doc proposal   t exactly as in LightPCLDA (ggs_z_lightpc.hpp: ui = U3 * (len + alphaSum), z[doc][(int)ui] -- this sweep's
//                  topics before the position, the old ones from it on -- or the alpha branch).  If t != s, a = alpha[s]:
//                    pi_d = (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1)) * (bS + (T(s) - 1)) / (bS + T(t))
//                                                     * (a + n[s]) / (a + n[t])
//                  new = t if pi_d > 1, else if U4 < pi_d, else s.  If t == s, new = z0 (`newTopic` keeps its initial value,
//                  :928, :1008): that undoes an accepted word proposal.
//   n[s]--, z[pos] = new, n[new]++.
// It is alpha[oldTopic] everywhere, and the word proposal weighs tokensPerType against beta * K while its acceptance assumes
// (n_wk + beta) / (n_k + betaSum): the chain is approximate as written and nothing of it is repaired here.
//
// Ours: the uniforms are lightpclda's (U1, U2 from Philox block 0, U3, U4 from block 1 of the token's Z stream, taken whether or
// not the branch that uses them runs).  A word's list is in ascending topic order; topicCountBetaHat[k] = (double)n_k + betaSum,
// afresh each sweep; tokensPerType[w] = the integer sum of the word's sweep-start row.  A table draw with i == nnz, and a
// beta- or alpha-branch topic == K, are GGS_ERR_INVALID_TOPIC, the topic clamped to the last valid one.  The three counters
// (ggs_get_mh_stats) are lightpclda's three classes.
#pragma once
#include "ggs_alias.hpp"
#include "ggs_z_pcgs.hpp"

namespace ggs {

// ---- the words' lists and tables over the counts -------------------------------------------------------------------------
// TypeTopicParallelTableBuilder.java:38-51 over the ascending list L of the word's topics with n_wk > 0:
// p_i = n_w,L[i] / topicCountBetaHat[L[i]], typeMass = the i-order sum from 0.0, then reGenerateAliasTable
// (OptimizedGentleAliasMethodDynamicSize.java:55-82) with k = nnz: bs[i] = p_i / typeMass - 1.0 / nnz and the lows / highs
// pairing chain of ggs_alias.hpp.  A single-wave workgroup takes `wpb` words at a time, as alias_build_kernel does: the
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
    if (lane < nwd && nnzl[lane] > 0)                                              // the chain of ggs_alias.hpp with k = nnz
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

// ---- the z step --------------------------------------------------------------------------------------------------------
// One WAVE per document over the pcgs kernels' length-sorted list, single-wave persistent workgroups, n[K] int32 in LDS, as
// lightpc_wave_kernel (ggs_z_lightpc.hpp), whose chunk machinery this is: everything a token needs that is independent of
// the tokens before it is computed for 64 tokens at once, lane-parallel, one chunk ahead -- word, z0, word-sorted position,
// the uniforms, which branch of the word proposal and hence the table cell, the list entry or the beta-branch topic, the
// count cells n_wk and n_k at z0 and at the word proposal, alpha of both, the four quotients of pi_w that do not involve the
// document, (int)ui or the alpha-branch topic and, where the document proposal is known ahead (the alpha branch; (int)ui the
// token's own position or a later one), its count cells and the two count quotients of pi_d for both outcomes of the word
// proposal.  A chunk's new topics stay in a register and go out as one vector store when the chunk ends; at the head of the
// next chunk, after that store has completed (vmcnt(0); the read is at agent scope), the tokens whose (int)ui lies in an
// earlier chunk gather z there and form their quotients.  The serial part per token is three count reads from LDS, two
// divisions, seven multiplies and the update; a token whose (int)ui is an earlier position of the SAME chunk takes the fresh
// topic from the register, loads its two count cells and divides twice more.
struct LightCollapsedParams {
  PcgsParams b;                // n_wk, n_k: the sweep-start counts; beta, beta_sum
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  const int32_t *tpt;          // [V]
  unsigned long long *mh;      // [3]: word proposal kept, document proposal accepted, left on z0
  double alpha_sum;
};

inline size_t lightcollapsed_lds_bytes(int K) { return (size_t)K * 4; }

__global__ __launch_bounds__(64) void lightcollapsed_wave_kernel(LightCollapsedParams lp) {
  const PcgsParams &p = lp.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K;
  const double fK = (double)K, alpha_sum = lp.alpha_sum, beta = p.beta, bS = p.beta_sum, bK = beta * fK;
  int32_t *cnt = reinterpret_cast<int32_t *>(smem);                                // [K]

  // the two count quotients of pi_d, t = the document proposal with cells (gd, td), for s = z0 (A) and s = the word proposal (B)
  auto q_a = [&](const int g0, const int t0, const int gd, const int td, double &q2, double &q3) {
    q2 = (beta + (double)gd) / (beta + ((double)g0 - 1.0));
    q3 = (bS + ((double)t0 - 1.0)) / (bS + (double)td);
  };
  auto q_b = [&](const int gw, const int tw, const int gd, const int td, const bool t_is_z0, double &q2, double &q3) {
    const int gs = gw + 1, ts = tw + 1, gt = gd - (t_is_z0 ? 1 : 0), tt = td - (t_is_z0 ? 1 : 0);
    q2 = (beta + (double)gt) / (beta + ((double)gs - 1.0));
    q3 = (bS + ((double)ts - 1.0)) / (bS + (double)tt);
  };

  for (int64_t di = blockIdx.x; di < p.num_docs; di += gridDim.x) {
    const int d = p.order[di];
    if (d < 0) continue;                                                           // padding of the lane-per-document kernels' list
    const int64_t beg = p.doc_ptr[d];
    const int len = (int)(p.doc_ptr[d + 1] - beg);
    if (len == 0) continue;
    __syncthreads();
    for (int k = lane; k < K; k += 64) cnt[k] = 0;
    __syncthreads();
    for (int t0 = 0; t0 < len; t0 += 64)
      if (t0 + lane < len) atomicAdd(&cnt[p.z[beg + t0 + lane]], 1);
    __syncthreads();
    const double flen = (double)len, span = flen + alpha_sum;

    // idx: (int)ui, or -1 on the alpha branch.  dt: the document proposal where it is known ahead, qa* / qb* its quotients
    struct Chunk { int w, z0, ip, wp, idx, dt, g0, gw, t0, tw; double U2, U4, a0, aw, r2, r3, r4, r5, qa2, qa3, qb2, qb3; };
    auto doc_quotients = [&](Chunk &c) {                                           // of c.dt
      const int gd = p.n_wk[(size_t)c.w * K + c.dt], td = p.n_k[c.dt];
      q_a(c.g0, c.t0, gd, td, c.qa2, c.qa3);
      q_b(c.gw, c.tw, gd, td, c.dt == c.z0, c.qb2, c.qb3);
    };
    auto load_chunk = [&](int t0) {
      Chunk c{};
      c.idx = -1;
      const int t = t0 + lane;
      if (t < len) {
        c.w = p.tok[beg + t]; c.z0 = p.z[beg + t]; c.ip = p.inv_perm[beg + t];
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        const U4 o0 = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), (uint32_t)GGS_PURPOSE_Z << 24, p.iteration, (uint32_t)p.seed,
                                    (uint32_t)(p.seed >> 32));
        const U4 o1 = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), ((uint32_t)GGS_PURPOSE_Z << 24) | 1u, p.iteration, (uint32_t)p.seed,
                                    (uint32_t)(p.seed >> 32));
        const double U1 = u53(o0.x, o0.y), U3 = u53(o1.x, o1.y);
        c.U2 = u53(o0.z, o0.w); c.U4 = u53(o1.z, o1.w);
        const size_t wrow = (size_t)c.w * K;
        const int nnz = lp.nw[c.w];
        const double ftpt = (double)lp.tpt[c.w];
        const double u_w = U1 * (ftpt + bK);
        if (u_w < ftpt) {                                                          // the table over the word's counts
          const double ups = (u_w / ftpt) * (double)nnz;                           // generateSample(u), k = nnz
          int i = (int)ups;
          if (i >= nnz || nnz <= 0) {
            atomicOr(p.status, ST_INVALID_TOPIC);
            i = max(nnz - 1, 0);
          } else if ((ups - (double)i) > lp.ps[wrow + i]) {
            i = min(max(lp.a[wrow + i], 0), nnz - 1);
          }
          c.wp = min((int)lp.nzw[wrow + i], K - 1);
        } else {
          int k = (int)(((u_w - ftpt) / bK) * fK);
          if (k >= K) { atomicOr(p.status, ST_INVALID_TOPIC); k = K - 1; }
          c.wp = max(k, 0);
        }
        c.g0 = p.n_wk[wrow + c.z0]; c.gw = p.n_wk[wrow + c.wp]; c.t0 = p.n_k[c.z0]; c.tw = p.n_k[c.wp];
        c.a0 = p.alpha[c.z0]; c.aw = p.alpha[c.wp];
        // pi_w's quotients two to five: s = z0, t = the word proposal (unused where they are equal)
        c.r2 = (beta + (double)c.gw) / (beta + ((double)c.g0 - 1.0));
        c.r3 = (bS + ((double)c.t0 - 1.0)) / (bS + (double)c.tw);
        c.r4 = (beta + (double)c.g0) / (beta + (double)c.gw);
        c.r5 = (bS + (double)c.tw) / (bS + (double)c.t0);
        const double ui = U3 * span;
        bool known = false;
        if (ui < flen) {
          c.idx = min((int)ui, len - 1);
          if (c.idx >= t) { c.dt = p.z[beg + c.idx]; known = true; }               // not written before this token's turn
        } else {
          int k = (int)(((ui - flen) / alpha_sum) * fK);
          if (k >= K) { atomicOr(p.status, ST_INVALID_TOPIC); k = K - 1; }
          c.dt = max(k, 0); known = true;
        }
        if (known) doc_quotients(c);
      }
      return c;
    };
    Chunk ch = load_chunk(0), chn = len > 64 ? load_chunk(64) : ch;
    int newz = 0, n_word = 0, n_doc = 0;

    for (int t = 0; t < len; ++t) {
      const int tl = t & 63, t0 = t - tl;
      const int z0 = __builtin_amdgcn_readlane(ch.z0, tl), wp = __builtin_amdgcn_readlane(ch.wp, tl), idx = __builtin_amdgcn_readlane(ch.idx, tl);
      int dt = __builtin_amdgcn_readlane(ch.dt, tl);
      const bool fresh = idx >= t0 && idx < t;                                     // an earlier token of this chunk: its new topic
      int gd = 0, td = 0;
      if (fresh) {
        dt = __builtin_amdgcn_readlane(newz, idx - t0);
        gd = p.n_wk[(size_t)__builtin_amdgcn_readlane(ch.w, tl) * K + dt];
        td = p.n_k[dt];
      }
      // (one wave per workgroup: its LDS operations execute in program order; the barriers keep the COMPILER to it)
      const int c0 = cnt[z0], cw = cnt[wp], cd = cnt[dt];
      __builtin_amdgcn_wave_barrier();

      // word proposal: s = z0, ni[s] = c0 - 1, ni[wp] = cw
      int acc_w = 0;
      if (wp != z0) {
        const double a0 = read_lane(ch.a0, tl);
        double pi_w = (a0 + (double)cw) / (a0 + (double)(c0 - 1));
        pi_w = pi_w * read_lane(ch.r2, tl);
        pi_w = pi_w * read_lane(ch.r3, tl);
        pi_w = pi_w * read_lane(ch.r4, tl);
        pi_w = pi_w * read_lane(ch.r5, tl);
        acc_w = (pi_w > 1.0 || read_lane(ch.U2, tl) < pi_w) ? 1 : 0;
      }
      acc_w = __builtin_amdgcn_readfirstlane(acc_w);
      const int s = acc_w ? wp : z0;
      const int n_s = acc_w ? cw + 1 : c0;                                         // with the token in flight
      // document proposal
      int nt = z0, acc_d = 0;                                                      // t == s: the reference's newTopic is still z0
      if (dt != s) {
        const double as = read_lane(acc_w ? ch.aw : ch.a0, tl);
        const int n_t = cd - ((acc_w && dt == z0) ? 1 : 0);                        // = ni[t]: t is not s
        double q2, q3;
        if (fresh) {
          if (acc_w) q_b(__builtin_amdgcn_readlane(ch.gw, tl), __builtin_amdgcn_readlane(ch.tw, tl), gd, td, dt == z0, q2, q3);
          else q_a(__builtin_amdgcn_readlane(ch.g0, tl), __builtin_amdgcn_readlane(ch.t0, tl), gd, td, q2, q3);
        } else {
          q2 = read_lane(acc_w ? ch.qb2 : ch.qa2, tl);
          q3 = read_lane(acc_w ? ch.qb3 : ch.qa3, tl);
        }
        double pi_d = (as + (double)n_t) / (as + (double)(n_s - 1));
        pi_d = pi_d * q2;
        pi_d = pi_d * q3;
        pi_d = pi_d * ((as + (double)n_s) / (as + (double)n_t));
        acc_d = (pi_d > 1.0 || read_lane(ch.U4, tl) < pi_d) ? 1 : 0;
        nt = acc_d ? dt : s;
      }
      nt = __builtin_amdgcn_readfirstlane(nt);
      acc_d = __builtin_amdgcn_readfirstlane(acc_d);
      if (nt != z0) {
        if (lane == 0) { cnt[z0] = c0 - 1; cnt[nt] = (acc_d ? cd : cw) + 1; }      // accepted from the document: nt = dt != z0; else nt = wp
        if (acc_d) n_doc += 1; else n_word += 1;
      } else if (acc_d) {
        n_doc += 1;                                                                // the document proposed z0 after an accepted word proposal
      }
      __builtin_amdgcn_wave_barrier();
      newz = lane == tl ? nt : newz;

      if (tl == 63 || t == len - 1) {
        if (t0 + lane <= t) {
          __hip_atomic_store(&p.z[beg + t0 + lane], newz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          p.zw[ch.ip] = newz;
        }
        if (t + 1 < len) {
          ch = chn;
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // the chunk's z is in memory before anything reads it
          if (t + 1 + lane < len && ch.idx >= 0 && ch.idx <= t) {                  // (int)ui in an earlier chunk: this sweep's topic
            ch.dt = __hip_atomic_load(&p.z[beg + ch.idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            doc_quotients(ch);
          }
          if (t + 1 + 64 < len) chn = load_chunk(t + 1 + 64);
        }
      }
    }
    if (lane == 0) {                                                               // once per document
      if (n_word) atomicAdd(&lp.mh[0], (unsigned long long)n_word);
      if (n_doc) atomicAdd(&lp.mh[1], (unsigned long long)n_doc);
      if (len - n_word - n_doc) atomicAdd(&lp.mh[2], (unsigned long long)(len - n_word - n_doc));
    }
  }
}

}  // namespace ggs
