// ggs_z_lightpcw2.hpp -- the z loop of scheme=lightpcldaw2 (LightPCLDAtypeTopicProposal.java:101-274; ParallelLDA.createModel's
// "lightpcldaw2"): the LightLDA sampler of Yuan et al. over the partially collapsed model -- Phi is drawn, as under pcgs -- with
// scheme=lightcollapsed's word proposal: the word's alias table over its type-topic counts plus a beta * K smoothing branch.
// Per token two Metropolis-Hastings proposals, each accepted on a quotient of two short products: O(1) per token, whatever K.
//
// The tables are the ones the class declares.  LightPCLDAtypeTopicProposal.java:72-77 declares a
// TypeTopicTableBuilderFactory and installs it nowhere (`tbFactory` exists only in CollapsedLightLDA), so a JVM run inherits
// spalias's alpha * phi tables of K entries and uses the drawn TOPIC as a POSITION in nonZeroTypeTopics[type][.] (:153), which
// beyond nnz_w holds what insert-at-end and swap-remove left behind, by thread timing.  That cannot be restated and is not the
// proposal calculateWordAcceptanceProbability corrects for.  This build runs what the class and TypeTopicParallelTableBuilder
// declare: p_i = n_w,L[i] / topicCountBetaHat[L[i]] over the word's ascending list L -- count_alias_build_kernel
// (ggs_z_lightcollapsed.hpp), unchanged, at the head of every z step on the sweep-start counts.
//
// Per non-empty document: n[k] = the topic histogram of the document's z; ni[k] is n[k] without the token in flight.  G[w][k] are
// the sweep-start type-topic counts and bhat[k] = (double)n_k + betaSum of the sweep start: unlike lightcollapsed nothing moves
// them for the token in flight (the reference's typeTopicCounts change in updateCounts only).  For each position in order, w the
// word, z0 = s = z[pos], (U1, U2, U3, U4) the token's uniforms:
//   word proposal   u_w = U1 * (tokensPerType[w] + beta * K).  u_w < tokensPerType[w]: t = L_w[generateSample(u_w /
//                   tokensPerType[w])] on the word's table of nnz_w entries; otherwise t = (int)(((u_w - tokensPerType[w]) /
//                   (beta * K)) * K) (:148-156).  If t != s (:270-272):
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (beta + G[w][s]) * bhat[t]
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (beta + G[w][t]) * bhat[s],   pi_w = nom / den
//                   (left to right, fp64, counts converted first); accepted if pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--,
//                   n[t]++, s = t.
//   doc proposal    LightPCLDA's, word for word (ggs_z_lightpc.hpp): ui = U3 * (len + alphaSum), z[doc][(int)ui] -- this sweep's
//                   topics before pos, the old ones from pos on, pos itself still z0 -- or the alpha branch; if t != s
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (alpha[s] + n[s])
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (alpha[s] + n[t]),   new = t if nom / den > 1, else if U4 < it, else s.
//                   If t == s, new = z0 (`newTopic` keeps its initial value, :130): that undoes an accepted word proposal.
//   n[s]--, z[pos] = new, n[new]++.
// IEEE as it falls: 0/0 is NaN and accepts nothing, x/0 is inf and accepts.  It is alpha[s] everywhere, and the word proposal
// weighs tokensPerType against beta * K while its acceptance assumes n_wk / bhat: the chain is approximate as written and nothing
// of it is repaired here.
//
// Ours: the uniforms are lightpclda's (U1, U2 from Philox block 0, U3, U4 from block 1 of the token's Z stream, taken whether or
// not the branch that uses them runs).  A table draw with i == nnz_w, and a beta- or alpha-branch topic == K, are
// GGS_ERR_INVALID_TOPIC, the topic clamped to the last valid one.  The three counters (ggs_get_mh_stats) are lightpclda's classes.
//
// One WAVE per document over the pcgs kernels' length-sorted list, single-wave persistent workgroups, n[K] int32 in LDS: the chunk
// machinery of lightpc_wave_kernel and lightcollapsed_wave_kernel.  Everything a token needs that is independent of the tokens
// before it is computed for 64 tokens at once, lane-parallel, one chunk ahead: word, z0, word-sorted position, the uniforms, the
// branch of the word proposal with its table cell and list entry or the beta-branch topic, phi, beta + G, bhat and alpha at z0 and
// at the word proposal, (int)ui or the alpha-branch topic and -- where (int)ui is the token's own position or a later one -- the
// old topic there and its phi.  A chunk's new topics stay in a register and go out as one vector store when the chunk ends; at
// the head of the next chunk, after that store has completed (vmcnt(0); the read is at agent scope), the tokens whose (int)ui lies
// in an earlier chunk gather z there and phi of it.  The serial part per token is three count reads from LDS, two quotients of
// three- and four-factor products and the update.
#pragma once
#include "ggs_z_lightcollapsed.hpp"

namespace ggs {

struct LightpcW2Params {
  PcgsParams b;                // phiT; n_wk, n_k: the sweep-start counts; beta, beta_sum
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  const int32_t *tpt;          // [V]
  unsigned long long *mh;      // [3]: word proposal kept, document proposal accepted, left on z0
  double alpha_sum;
};

inline size_t lightpcw2_lds_bytes(int K) { return (size_t)K * 4; }

__global__ __launch_bounds__(64) void lightpcw2_wave_kernel(LightpcW2Params lp) {
  const PcgsParams &p = lp.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K;
  const double fK = (double)K, alpha_sum = lp.alpha_sum, beta = p.beta, bS = p.beta_sum, bK = beta * fK;
  int32_t *cnt = reinterpret_cast<int32_t *>(smem);                                // [K]

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

    // idx: (int)ui, or -1 on the alpha branch.  dt, phd: the document proposal and phi of it, known ahead on the alpha branch and
    // where idx is the token's own position or a later one (old topics).  bg*: beta + G[w][.], bh*: bhat[.], at z0 and at wp
    struct Chunk { int w, z0, ip, wp, idx, dt; double U2, U4, a0, aw, ph0, phw, phd, bg0, bgw, bh0, bhw; };
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
        const double *row = p.phiT + (size_t)c.w * p.Kp;
        c.a0 = p.alpha[c.z0]; c.aw = p.alpha[c.wp]; c.ph0 = row[c.z0]; c.phw = row[c.wp];
        c.bg0 = beta + (double)p.n_wk[wrow + c.z0]; c.bgw = beta + (double)p.n_wk[wrow + c.wp];
        c.bh0 = (double)p.n_k[c.z0] + bS; c.bhw = (double)p.n_k[c.wp] + bS;
        const double ui = U3 * span;
        if (ui < flen) {
          c.idx = min((int)ui, len - 1);
          if (c.idx >= t) { c.dt = p.z[beg + c.idx]; c.phd = row[c.dt]; }          // not written before this token's turn
        } else {
          int k = (int)(((ui - flen) / alpha_sum) * fK);
          if (k >= K) { atomicOr(p.status, ST_INVALID_TOPIC); k = K - 1; }
          c.dt = max(k, 0); c.phd = row[c.dt];
        }
      }
      return c;
    };
    Chunk ch = load_chunk(0), chn = len > 64 ? load_chunk(64) : ch;
    int newz = 0, n_word = 0, n_doc = 0;

    for (int t = 0; t < len; ++t) {
      const int tl = t & 63, t0 = t - tl;
      const int z0 = __builtin_amdgcn_readlane(ch.z0, tl), wp = __builtin_amdgcn_readlane(ch.wp, tl), idx = __builtin_amdgcn_readlane(ch.idx, tl);
      int dt = __builtin_amdgcn_readlane(ch.dt, tl);
      double phd = read_lane(ch.phd, tl);
      if (idx >= t0 && idx < t) {                                                  // an earlier token of this chunk: its new topic
        dt = __builtin_amdgcn_readlane(newz, idx - t0);
        phd = p.phiT[(size_t)__builtin_amdgcn_readlane(ch.w, tl) * p.Kp + dt];
      }
      // (one wave per workgroup: its LDS operations execute in program order; the barriers keep the COMPILER to it)
      const int c0 = cnt[z0], cw = cnt[wp], cd = cnt[dt];
      __builtin_amdgcn_wave_barrier();

      // word proposal: s = z0, ni[s] = c0 - 1, ni[wp] = cw
      int acc_w = 0;
      if (wp != z0) {
        const double a0 = read_lane(ch.a0, tl);
        const double nom = read_lane(ch.phw, tl) * (a0 + (double)cw) * read_lane(ch.bg0, tl) * read_lane(ch.bhw, tl);
        const double den = read_lane(ch.ph0, tl) * (a0 + (double)(c0 - 1)) * read_lane(ch.bgw, tl) * read_lane(ch.bh0, tl);
        const double pi_w = nom / den;
        acc_w = (pi_w > 1.0 || read_lane(ch.U2, tl) < pi_w) ? 1 : 0;
      }
      acc_w = __builtin_amdgcn_readfirstlane(acc_w);
      const int s = acc_w ? wp : z0;
      const int n_s = acc_w ? cw + 1 : c0;                                         // with the token in flight
      // document proposal
      int nt = z0, acc_d = 0;                                                      // t == s: the reference's newTopic is still z0
      if (dt != s) {
        const double as = read_lane(acc_w ? ch.aw : ch.a0, tl), phs = read_lane(acc_w ? ch.phw : ch.ph0, tl);
        const int n_t = cd - ((acc_w && dt == z0) ? 1 : 0);                        // = ni[t]: t is not s
        const double nom = phd * (as + (double)n_t) * (as + (double)n_s);
        const double den = phs * (as + (double)(n_s - 1)) * (as + (double)n_t);
        const double ratio = nom / den;
        acc_d = (ratio > 1.0 || read_lane(ch.U4, tl) < ratio) ? 1 : 0;
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
            ch.phd = p.phiT[(size_t)ch.w * p.Kp + ch.dt];
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
