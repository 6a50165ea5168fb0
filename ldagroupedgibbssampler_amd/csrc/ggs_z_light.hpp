// ggs_z_light.hpp -- light_wave_body: the one body of the three Metropolis-Hastings wave-per-document z kernels,
//   Light::pc         lightpc_wave_kernel         scheme=lightpclda      ggs_z_lightpc.hpp
//   Light::w2         lightpcw2_wave_kernel       scheme=lightpcldaw2    ggs_z_lightpcw2.hpp
//   Light::collapsed  lightcollapsed_wave_kernel  scheme=lightcollapsed  ggs_z_lightcollapsed.hpp
// whose headers say what each scheme computes and where the reference says so.  The three are the same program: per token a
// word proposal t accepted on pi_w, then a document proposal t accepted on pi_d, then n[s]--, z[pos] = new, n[new]++.  They
// differ in where the word proposal is drawn (two draws, below) and in the factors of pi_w and pi_d; every such place is an
// `if constexpr (L ...)` or a LightChunk<L> field.
//
// The uniforms (U1, U2, U3, U4) of a token: U1, U2 are the two doubles of Philox block 0 and U3, U4 those of block 1 of its Z
// stream (purpose Z, element = global token index), taken at these positions whether or not the branch that uses them runs.
// U1 draws the word proposal, U2 accepts it, U3 draws the document proposal, U4 accepts it.  The three counters (lp.mh,
// ggs_get_mh_stats) classify a token by where its new topic came from: [1] the document proposal accepted; else [0] the word
// proposal accepted and kept; else [2] left on z0.  They are counted in registers and added once per document.
//
// The chunk machinery.  One WAVE per document over the pcgs kernels' length-sorted list, single-wave persistent workgroups,
// n[K] int32 in LDS.  No running sums, no lists, no margins: every comparison is on values computed by the same few IEEE
// operations in the reference's order, so there is no replay path.  Nearly everything a token needs is independent of the
// tokens before it and is computed for 64 tokens at once, lane-parallel, one chunk ahead (load_chunk: lane i holds token i):
// word, z0, word-sorted position, the uniforms, the word proposal, alpha at z0 and at the word proposal, what pi_w and pi_d
// need there (at_z0_and_wp), (int)ui or the alpha-branch topic and -- where the document proposal is KNOWN AHEAD: the alpha
// branch, or (int)ui the token's own position or a later one, which still holds its old topic at the token's turn -- that
// topic and what pi_d needs of it (doc_known).  The serial part per token is three count reads from LDS, the two quotients
// and the update.  A token whose (int)ui is an earlier position of the SAME chunk (about 32 / len of them) takes the fresh
// topic from the register newz and makes the dependent loads of doc_known's operands itself.
// Ordering.  A chunk's new topics stay in newz and go out as one vector store when the chunk ends.  At the head of the next
// chunk the tokens whose (int)ui lies in an EARLIER chunk gather this sweep's z there.  That read must see the store: the
// s_waitcnt vmcnt(0) between them lets no read start behind a store in flight, and both are relaxed atomics at agent scope,
// so the read goes past the L1, which a plain load of a line fetched by load_chunk's p.z[beg + c.idx] need not.  Only then is
// the chunk after next loaded: its known-ahead reads of z are of positions >= its own, which no store has reached.
//
// Settled here for all three (the copies had drifted):
//   c.idx = (int)ui, no min(., len - 1): ui < flen, flen an exact integer and U3 >= 0 give 0 <= (int)ui <= len - 1.
//   No max(k, 0) on an alpha- or beta-branch topic k = (int)(((u - m) / r) * K): the branch is taken on !(u < m), so u - m >= 0
//   or NaN; r < 0 would need u = U * (m + r) >= m with m >= 0, which only u = m = 0 allows, and then k = 0; the conversion of
//   NaN is 0.  So k >= 0 whatever the priors are, and the clamp from above (k >= K) is the only one that can act.
//   One Chunk initialisation: value-initialised, idx = -1.
// Codegen.  The body is a __forceinline__ template with lambdas inside, as sparse_wave_body; the two draws are function
// templates.  lightpc_wave_kernel's registers, scratch and waves per SIMD are the former kernel's (111 VGPRs, 4 waves); the
// other two lost the instructions of the two clamps above (ggs_resource_summary.txt, profiles/light_wave_refactor_ab.txt).
#pragma once
#include "ggs_z_pcgs.hpp"

namespace ggs {

struct LightpcParams {          // LightCountParams adds the words' lists over the counts
  PcgsParams b;                // w2, collapsed: n_wk, n_k are the sweep-start counts; beta, beta_sum
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  unsigned long long *mh;      // [3]: word proposal kept, document proposal accepted, left on z0
  double alpha_sum;
};
struct LightCountParams : LightpcParams {   // count_alias_build_kernel's tables (ggs_alias.hpp): a row's first nw[w] entries
  const uint16_t *nzw;         // [V][K]
  const int32_t *nw;           // [V]
  const int32_t *tpt;          // [V]
};

inline size_t light_lds_bytes(int K) { return (size_t)K * 4; }

enum class Light { pc, w2, collapsed };

// idx: (int)ui, or -1 on the alpha branch.  dt: the document proposal where it is known ahead, or gathered at the chunk head
struct LightChunkBase { int w, z0, ip, wp, idx, dt; double U2, U4, a0, aw; };
template <Light L> struct LightChunk;
template <> struct LightChunk<Light::pc> : LightChunkBase { double ph0, phw, phd; };   // phi at z0, at wp, at dt
template <> struct LightChunk<Light::w2> : LightChunkBase { double ph0, phw, phd, bg0, bgw, bh0, bhw; };   // bg*: beta + G[w][.], bh*: bhat[.]
// g*, t*: the cells n_wk[w][.], n_k[.]; r2..r5: pi_w's quotients two to five; qa*, qb*: pi_d's two count quotients for s = z0, s = wp
template <> struct LightChunk<Light::collapsed> : LightChunkBase { int g0, gw, t0, tw; double r2, r3, r4, r5, qa2, qa3, qb2, qb3; };

// The word proposal of lightpclda: the cell of spalias's K-entry table at U1 (generateSample, as spalias's sample(w, x)).
// i == K is GGS_ERR_INVALID_TOPIC, the topic K - 1.
template <class Params>
__device__ __forceinline__ int light_draw_alias_cell(const Params &lp, const int w, const double U1, const double fK) {
  const int K = lp.b.K;
  const double ups = U1 * fK;
  const int i = (int)ups;
  if (i >= K) {
    atomicOr(lp.b.status, ST_INVALID_TOPIC);
    return K - 1;
  }
  const size_t o = (size_t)w * K + i;
  return (ups - (double)i) > lp.ps[o] ? lp.a[o] : i;
}

// The word proposal of lightcollapsed and lightpcldaw2: u_w = U1 * (tokensPerType[w] + beta * K); below tokensPerType[w] the
// word's table over its counts (nnz entries, then its list), otherwise the beta branch.  i == nnz and k == K are
// GGS_ERR_INVALID_TOPIC, the topic clamped to the last valid one; the other clamps keep a torn table inside the row.
template <class Params>
__device__ __forceinline__ int light_draw_count_table(const Params &lp, const int w, const double U1, const double fK, const double bK) {
  const int K = lp.b.K;
  const size_t wrow = (size_t)w * K;
  const int nnz = lp.nw[w];
  const double ftpt = (double)lp.tpt[w];
  const double u_w = U1 * (ftpt + bK);
  if (u_w < ftpt) {                                                                // the table over the word's counts
    const double ups = (u_w / ftpt) * (double)nnz;                                 // generateSample(u), k = nnz
    int i = (int)ups;
    if (i >= nnz || nnz <= 0) {
      atomicOr(lp.b.status, ST_INVALID_TOPIC);
      i = max(nnz - 1, 0);
    } else if ((ups - (double)i) > lp.ps[wrow + i]) {
      i = min(max(lp.a[wrow + i], 0), nnz - 1);
    }
    return min((int)lp.nzw[wrow + i], K - 1);
  }
  int k = (int)(((u_w - ftpt) / bK) * fK);
  if (k >= K) { atomicOr(lp.b.status, ST_INVALID_TOPIC); k = K - 1; }
  return k;
}

template <Light L, class Params>
__device__ __forceinline__ void light_wave_body(const Params &lp) {
  constexpr bool PHI = L != Light::collapsed;                                      // pi_w / pi_d have a phi factor; else count quotients
  using Chunk = LightChunk<L>;
  const PcgsParams &p = lp.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K;
  const double fK = (double)K, alpha_sum = lp.alpha_sum, beta = p.beta, bS = p.beta_sum, bK = beta * fK;   // beta*: not Light::pc
  int32_t *cnt = reinterpret_cast<int32_t *>(smem);                                // [K]

  // collapsed: the two count quotients of pi_d, t = the document proposal with cells (gd, td), for s = z0 (A) and s = the word proposal (B)
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

    auto at_z0_and_wp = [&](Chunk &c) {
      if constexpr (PHI) {
        const double *row = p.phiT + (size_t)c.w * p.Kp;
        c.ph0 = row[c.z0]; c.phw = row[c.wp];
      }
      if constexpr (L == Light::w2) {
        const size_t wrow = (size_t)c.w * K;
        c.bg0 = beta + (double)p.n_wk[wrow + c.z0]; c.bgw = beta + (double)p.n_wk[wrow + c.wp];
        c.bh0 = (double)p.n_k[c.z0] + bS; c.bhw = (double)p.n_k[c.wp] + bS;
      }
      if constexpr (L == Light::collapsed) {
        const size_t wrow = (size_t)c.w * K;
        c.g0 = p.n_wk[wrow + c.z0]; c.gw = p.n_wk[wrow + c.wp]; c.t0 = p.n_k[c.z0]; c.tw = p.n_k[c.wp];
        // s = z0, t = the word proposal (unused where they are equal)
        c.r2 = (beta + (double)c.gw) / (beta + ((double)c.g0 - 1.0));
        c.r3 = (bS + ((double)c.t0 - 1.0)) / (bS + (double)c.tw);
        c.r4 = (beta + (double)c.g0) / (beta + (double)c.gw);
        c.r5 = (bS + (double)c.tw) / (bS + (double)c.t0);
      }
    };
    auto doc_known = [&](Chunk &c) {                                               // of c.dt
      if constexpr (PHI) {
        c.phd = p.phiT[(size_t)c.w * p.Kp + c.dt];
      } else {
        const int gd = p.n_wk[(size_t)c.w * K + c.dt], td = p.n_k[c.dt];
        q_a(c.g0, c.t0, gd, td, c.qa2, c.qa3);
        q_b(c.gw, c.tw, gd, td, c.dt == c.z0, c.qb2, c.qb3);
      }
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
        if constexpr (L == Light::pc) c.wp = light_draw_alias_cell(lp, c.w, U1, fK);
        else c.wp = light_draw_count_table(lp, c.w, U1, fK, bK);
        c.a0 = p.alpha[c.z0]; c.aw = p.alpha[c.wp];
        at_z0_and_wp(c);
        const double ui = U3 * span;
        if (ui < flen) {
          c.idx = (int)ui;
          if (c.idx >= t) { c.dt = p.z[beg + c.idx]; doc_known(c); }               // not written before this token's turn
        } else {
          int k = (int)(((ui - flen) / alpha_sum) * fK);
          if (k >= K) { atomicOr(p.status, ST_INVALID_TOPIC); k = K - 1; }
          c.dt = k; doc_known(c);
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
      const bool fresh = idx >= t0 && idx < t;                                     // an earlier token of this chunk: its new topic
      [[maybe_unused]] double phd = 0.0;
      [[maybe_unused]] int gd = 0, td = 0;
      if constexpr (PHI) phd = read_lane(ch.phd, tl);
      if (fresh) {
        dt = __builtin_amdgcn_readlane(newz, idx - t0);
        const int w = __builtin_amdgcn_readlane(ch.w, tl);
        if constexpr (PHI) {
          phd = p.phiT[(size_t)w * p.Kp + dt];
        } else {
          gd = p.n_wk[(size_t)w * K + dt];
          td = p.n_k[dt];
        }
      }
      // (one wave per workgroup: its LDS operations execute in program order; the barriers keep the COMPILER to it)
      const int c0 = cnt[z0], cw = cnt[wp], cd = cnt[dt];
      __builtin_amdgcn_wave_barrier();

      // word proposal: s = z0, ni[s] = c0 - 1, ni[wp] = cw
      int acc_w = 0;
      if (wp != z0) {
        const double a0 = read_lane(ch.a0, tl);
        double pi_w;
        if constexpr (L == Light::pc) {
          pi_w = (a0 + (double)cw) / (a0 + (double)(c0 - 1));
        } else if constexpr (L == Light::w2) {
          const double nom = read_lane(ch.phw, tl) * (a0 + (double)cw) * read_lane(ch.bg0, tl) * read_lane(ch.bhw, tl);
          const double den = read_lane(ch.ph0, tl) * (a0 + (double)(c0 - 1)) * read_lane(ch.bgw, tl) * read_lane(ch.bh0, tl);
          pi_w = nom / den;
        } else {
          pi_w = (a0 + (double)cw) / (a0 + (double)(c0 - 1));
          pi_w = pi_w * read_lane(ch.r2, tl);
          pi_w = pi_w * read_lane(ch.r3, tl);
          pi_w = pi_w * read_lane(ch.r4, tl);
          pi_w = pi_w * read_lane(ch.r5, tl);
        }
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
        double pi_d;
        if constexpr (PHI) {
          const double phs = read_lane(acc_w ? ch.phw : ch.ph0, tl);
          const double nom = phd * (as + (double)n_t) * (as + (double)n_s);
          const double den = phs * (as + (double)(n_s - 1)) * (as + (double)n_t);
          pi_d = nom / den;
        } else {
          double q2, q3;
          if (fresh) {
            if (acc_w) q_b(__builtin_amdgcn_readlane(ch.gw, tl), __builtin_amdgcn_readlane(ch.tw, tl), gd, td, dt == z0, q2, q3);
            else q_a(__builtin_amdgcn_readlane(ch.g0, tl), __builtin_amdgcn_readlane(ch.t0, tl), gd, td, q2, q3);
          } else {
            q2 = read_lane(acc_w ? ch.qb2 : ch.qa2, tl);
            q3 = read_lane(acc_w ? ch.qb3 : ch.qa3, tl);
          }
          pi_d = (as + (double)n_t) / (as + (double)(n_s - 1));
          pi_d = pi_d * q2;
          pi_d = pi_d * q3;
          pi_d = pi_d * ((as + (double)n_s) / (as + (double)n_t));
        }
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
            doc_known(ch);
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
