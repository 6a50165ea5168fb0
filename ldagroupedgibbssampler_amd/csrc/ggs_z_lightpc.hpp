// ggs_z_lightpc.hpp -- the z loop of scheme=lightpclda (LightPCLDA.java:86-221; ParallelLDA.java:469-473): the LightLDA
// sampler of Yuan et al. over the partially collapsed model.  Per token two Metropolis-Hastings proposals, one from the
// word's alias table and one from the document's own indicator array, each accepted on a ratio of a handful of numbers:
// O(1) per token, whatever K.
//
// The tables are spalias's.  LightPCLDA.java:50-83 declares a PhiTableBuilderFactory, but nothing installs it (`tbFactory`
// exists only in CollapsedLightLDA); the inherited doPreIterationTableBuling (SpaliasUncollapsedParallelLDA.java:83-115)
// builds PhiAlphaParallelTableBuilder tables, so a running LightPCLDA draws its word proposal from
// pi[k] = phi[k][w] * alpha[k] -- alias_build_kernel (ggs_alias.hpp), unchanged.
//
// The reference as it runs, per non-empty document: n[k] = the topic histogram of the document's z; ni[k] is n[k] without
// the token in flight (the reference keeps it as a second array of doubles; here it is n[k] - (k == s), no array).  For
// each position in order, w the word, z0 = s = z[pos], (U1, U2, U3, U4) the token's uniforms:
//   word proposal   t = the alias draw of w at U1.  If t != s: pi_w = (alpha[s] + ni[t]) / (alpha[s] + ni[s]); accepted if
//                   pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--, n[t]++, s = t.
//   doc proposal    ui = U3 * (len + alphaSum).  ui < len: t = z[doc][(int)ui] -- the array holds this sweep's new topics
//                   before pos and the old ones from pos on, position pos itself still z0, not s.  Otherwise
//                   t = (int)(((ui - len) / alphaSum) * K).  If t != s:
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (alpha[s] + n[s])
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (alpha[s] + n[t]),   ratio = nom / den
//                   (left to right, fp64, counts converted first); new = t if ratio > 1, else if U4 < ratio, else s.
//                   If t == s the reference assigns nothing and `newTopic` still holds its initial value (LightPCLDA.java:115):
//                   new = z0, which undoes an accepted word proposal.  IEEE as it falls: 0/0 is NaN and accepts nothing,
//                   x/0 is inf and accepts.
//   n[s]--, z[pos] = new, n[new]++.
// It is alpha[s] everywhere (right for symmetric alpha only), the document proposal is treated as state independent and
// reads z0 after an accepted word proposal: the chain is approximate by design and nothing of it is repaired here.
//
// Ours: U1, U2 are the two doubles of Philox block 0 and U3, U4 those of block 1 of the token's Z stream (purpose Z,
// element = global token index), taken at these positions whether or not the branch that uses them runs; U1 is the
// uniform every other scheme's token draws.  alphaSum is the k-order sum of alpha.  An alias draw with i == K, and an
// alpha-branch topic == K (ui rounded up to len + alphaSum; Java would index out of bounds), are GGS_ERR_INVALID_TOPIC, the
// topic clamped to K - 1.  The three counters (ggs_get_mh_stats) classify a token by where its new topic came from: the
// document proposal accepted; else the word proposal accepted and kept; else left on z0.
//
// One WAVE per document over the pcgs kernels' length-sorted list, single-wave persistent workgroups, n[K] int32 in LDS.
// No running sums, no lists, no margins: every comparison is on values computed by the same few IEEE operations in the
// reference's order, so there is no replay path.  Nearly everything a token needs is independent of the tokens before it
// and is computed for 64 tokens at once, lane-parallel, one chunk ahead: word, z0, word-sorted position, the uniforms,
// the alias cell and hence the word proposal, alpha and phi of z0 and of the word proposal, (int)ui or the alpha-branch
// topic, and -- where (int)ui is the token's own position or a later one -- the old topic there and its phi.  A chunk's
// new topics stay in a register (lane i: token i) and go out as one vector store when the chunk ends; at the head of the
// next chunk, after that store has completed (vmcnt(0): no read behind a store in flight, and the read is at agent scope,
// past the L1), the tokens whose (int)ui lies in an earlier chunk gather z there and phi of it.  The serial part per token
// is three count reads from LDS, two ratios and the update.  A token whose (int)ui is an earlier position of the SAME
// chunk (about 32 / len of them) takes the fresh topic from the register and makes one dependent phi load.
#pragma once
#include "ggs_z_pcgs.hpp"

namespace ggs {

struct LightpcParams {
  PcgsParams b;
  const double *ps;            // [V][K]
  const int32_t *a;            // [V][K]
  unsigned long long *mh;      // [3]: word proposal kept, document proposal accepted, left on z0
  double alpha_sum;
};

inline size_t lightpc_lds_bytes(int K) { return (size_t)K * 4; }

__global__ __launch_bounds__(64) void lightpc_wave_kernel(LightpcParams lp) {
  const PcgsParams &p = lp.b;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x, K = p.K;
  const double fK = (double)K, alpha_sum = lp.alpha_sum;
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

    // idx: (int)ui, or -1 on the alpha branch.  dt, phd: the document proposal and phi of it, known ahead on the alpha
    // branch and where idx is the token's own position or a later one (old topics)
    struct Chunk { int w, z0, ip, wp, idx, dt; double U2, U4, a0, aw, ph0, phw, phd; };
    auto load_chunk = [&](int t0) {
      Chunk c{0, 0, 0, 0, -1, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
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
        const double ups = U1 * fK;                                                // generateSample, as spalias's sample(w, x)
        const int i = (int)ups;
        if (i >= K) {
          atomicOr(p.status, ST_INVALID_TOPIC);
          c.wp = K - 1;
        } else {
          const size_t o = (size_t)c.w * K + i;
          c.wp = (ups - (double)i) > lp.ps[o] ? lp.a[o] : i;
        }
        const double *row = p.phiT + (size_t)c.w * p.Kp;
        c.a0 = p.alpha[c.z0]; c.aw = p.alpha[c.wp]; c.ph0 = row[c.z0]; c.phw = row[c.wp];
        const double ui = U3 * span;
        if (ui < flen) {
          c.idx = (int)ui;
          if (c.idx >= t) { c.dt = p.z[beg + c.idx]; c.phd = row[c.dt]; }          // not written before this token's turn
        } else {
          int k = (int)(((ui - flen) / alpha_sum) * fK);
          if (k >= K) { atomicOr(p.status, ST_INVALID_TOPIC); k = K - 1; }
          c.dt = k; c.phd = row[k];
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
        const double pi_w = (a0 + (double)cw) / (a0 + (double)(c0 - 1));
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
