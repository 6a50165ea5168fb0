// ggs_z_pcgs.hpp -- the z loop of scheme=pcgs (LDAPartiallyCollapsedGibbsSampler; the loop itself
// is UncollapsedParallelLDA.sampleTopicAssignmentsParallel, UPLDA:1466-1544): theta is integrated
// out, score[k] = (n_dk + alpha_k) * phi[k][w] with the document's topic counts n_d. updated after
// every token.  The tokens of a document are therefore strictly sequential; documents are
// independent given Phi.  SURVEY.md section 8(f), item 1 ("next"); same Phi draw, same count
// rebuild and the same per-token Philox uniform (purpose Z, element = global token index) as GGS.
//
// One LANE per document: a single-wave workgroup takes 64 documents (the host sorts documents
// by length, longest first, so the 64 of a group are equally long) and walks their tokens in
// lockstep -- step t handles token t of each of the 64 documents, which is exactly the access
// pattern of a GGS chunk (64 tokens, 64 different phiT rows).  The rows stream through the
// slice ring of ggs_slice_ring.hpp (3 slots here) twice per step (pass 1 sums, pass 2 re-multiplies and
// walks; the product (n + alpha) * phi is the same two roundings in both passes: int + double,
// then the multiply), the next step's first slices are in flight while this step ends.
// Per-lane state: the document's K topic counts, int16, in LDS as [k][lane] (lane-contiguous,
// conflict-free), decremented before the scores and incremented after the draw (UPLDA:1494,1535).
#pragma once
#include "ggs_z_stream.hpp"

namespace ggs {

struct PcgsParams {
  const int32_t *tok;
  const int32_t *inv_perm;
  int32_t *z, *zw;
  const int64_t *doc_ptr;
  const int32_t *order;        // [D] local documents, longest first
  const double *alpha;
  const double *phiT;
  uint32_t *status;
  int64_t num_docs, tok_base;
  uint64_t seed;
  uint32_t iteration;
  int32_t K, Kp;
  // scheme=collapsed (pcgs_z_kernel<true>, ggs_z_collapsed.hpp): phiT holds psi[w][k] = (beta + n_wk)/(betaSum + n_k) of the
  // sweep-start counts; the entry of the token's own old topic is recomputed with the token removed
  const int32_t *n_wk;         // [V][K] sweep-start counts
  const int32_t *n_k;          // [K]
  double beta, beta_sum;
};

// (kPcgsMaxDocLen, the longest document the int16 counts hold: ggs_layout.hpp)
constexpr int kPcgsRingSlots = 3;      // two slices ahead: 24 KiB of ring, so that four waves fit a CU at K = 100
// LDS of pcgs_z_body (pcgs_z_kernel, polyaurn_z_kernel): the ring, the alpha row zero-padded to KT topics, the int16 document
// counts [KT][64]; KT = whole slices, at least the ring's depth (mirrors NS / alb / cnt below, whose K is a run-time parameter)
constexpr int pcgs_z_alpha_offset() { return kPcgsRingSlots * kSliceBytes; }
constexpr int pcgs_z_slices(const int K) { return imax(kPcgsRingSlots - 1, (K + kSliceTopics - 1) / kSliceTopics); }
constexpr int pcgs_z_lds_bytes(const int K) { return pcgs_z_alpha_offset() + pcgs_z_slices(K) * kSliceTopics * (8 + 128); }
// LDS of the score-register kernels (pcgs_sliced_body, below): the alpha row and the counts, then the ring
constexpr int pcgs_sliced_head_bytes(const int kmax) { return (kmax * 8 + kmax * 128 + 255) / 256 * 256; }
constexpr int pcgs_sliced_lds_bytes(const int K) { return pcgs_sliced_head_bytes((K + 7) / 8 * 8) + kPcgsRingSlots * kSliceBytes; }

// POLYAURN (scheme polyaurn, PolyaUrnSpaliasLDA.java:261-278): a document of one token, or a token whose scores sum to 0
// (the word's Phi column is all zero), draws floor(U * K) -- the reference's candidate list is empty there.  Every other
// token is drawn as pcgs draws it.
__device__ __forceinline__ int polyaurn_uniform_topic(const double U, const int K) { return min((int)(U * (double)K), K - 1); }

template <bool COLLAPSED, bool POLYAURN>
__device__ __forceinline__ void pcgs_z_body(PcgsParams &p) {
  constexpr int kAhead = kPcgsRingSlots - 1;
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int K = p.K;
  const int NS = max(kAhead, (K + kSliceTopics - 1) / kSliceTopics);   // slices per pass; at least kAhead (padding topics score 0)
  const int KT = NS * kSliceTopics;
  double *alb = reinterpret_cast<double *>(smem + pcgs_z_alpha_offset());   // alpha, zero padded to KT
  int16_t *cnt = reinterpret_cast<int16_t *>(alb + KT);                              // [KT][64]
  const unsigned char *phib = reinterpret_cast<const unsigned char *>(p.phiT);
  const size_t rowbytes = (size_t)p.Kp * 8;
  const unsigned char *my_row = ring_lane_row(smem, lane);        // the ring (ggs_slice_ring.hpp) starts the workgroup's LDS
  const int rot = ring_lane_rotation(lane);

  for (int k = lane; k < KT; k += 64) alb[k] = k < K ? p.alpha[k] : 0.0;

  const int64_t groups = (p.num_docs + 63) / 64;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t di = g * 64 + lane;
    const int d = di < p.num_docs ? p.order[di] : -1;
    const int64_t beg = d >= 0 ? p.doc_ptr[d] : 0;
    const int len = d >= 0 ? (int)(p.doc_ptr[d + 1] - beg) : 0;
    const int steps = __shfl(len, 0);                              // lane 0 holds the group's longest document
    if (steps == 0) break;                                         // sorted: every later group is empty too
    // UPLDA:1482-1485 localTopicCounts
    for (int k = 0; k < KT; ++k) cnt[k * 64 + lane] = 0;
    for (int t = 0; t < len; ++t) cnt[p.z[beg + t] * 64 + lane] += 1;

    int w = len > 0 ? p.tok[beg] : 0;
    const unsigned char *ra[8], *ran[8];
    ring_row_addresses(phib, rowbytes, w, lane, ra);
    int gs = 0;                                                   // ring slot of this step's first slice
#pragma unroll
    for (int s = 0; s < kAhead; ++s) ring_issue(smem, s, s, ra);
    // the token's old topic and (COLLAPSED) psi of that topic with the token itself removed (MSLDA:185-190), both
    // fetched one step ahead: z[beg + t + 1] is not written before step t + 1, the counts are the sweep-start ones
    int znext = len > 0 ? p.z[beg] : 0;
    auto own_of = [&](const int word, const int topic) {
      return (p.beta + (double)(p.n_wk[(size_t)word * K + topic] - 1)) / (p.beta_sum + (double)(p.n_k[topic] - 1));
    };
    double own_next = (COLLAPSED && len > 0) ? own_of(w, znext) : 0.0;

    for (int t = 0; t < steps; ++t) {
      const bool active = t < len, has1 = t + 1 < steps;
      const int zold = znext;
      const double own = own_next;
      const int ip = active ? p.inv_perm[beg + t] : 0;
      const int w1 = (t + 1 < len) ? p.tok[beg + t + 1] : 0;
      znext = (t + 1 < len) ? p.z[beg + t + 1] : 0;
      if (COLLAPSED && t + 1 < len) own_next = own_of(w1, znext);
      if (has1) ring_row_addresses(phib, rowbytes, w1, lane, ran);
      if (active) cnt[zold * 64 + lane] -= 1;                      // UPLDA:1494 (a count below zero cannot arise: it was built from z above)
      asm volatile("" ::: "memory");

      double sum = 0.0, tt = 0.0, U = 0.0;
      int newc = 0;
      for (int j = 0; j < 2 * NS; ++j) {
        const int s = j < NS ? j : j - NS;
        const int cur = (gs + j) % kPcgsRingSlots;
        const int nxt = (gs + j + kAhead) % kPcgsRingSlots;
        const int ja = j + kAhead;
        if (ja < 2 * NS) ring_issue(smem, ja < NS ? ja : ja - NS, nxt, ra);
        else if (has1) ring_issue(smem, ja - 2 * NS, nxt, ran);
        // kAhead slices follow slice j; at the tail of the last step fewer
        if (has1 || ja < 2 * NS) ring_wait_all_but<kAhead>();
        else ring_wait_all_but<kAhead - 1>(2 * NS - 1 - j);
        if (active) {
          const unsigned char *rb = my_row + cur * kSliceBytes;
          const unsigned char *ab = reinterpret_cast<const unsigned char *>(alb) + s * kSliceTopics * 8;
          const int16_t *cb = cnt + (s * kSliceTopics) * 64 + lane;
          D2 ph[kSliceUnits], al[kSliceUnits];
          int n[kSliceTopics];
#pragma unroll
          for (int u = 0; u < kSliceUnits; ++u) {
            ph[u] = lds_d2(rb + ring_unit_offset(u, rot));
            al[u] = lds_d2(ab + u * 16);
            n[2 * u] = cb[(2 * u) * 64];
            n[2 * u + 1] = cb[(2 * u + 1) * 64];
          }
          if (COLLAPSED) {
            const int rel = zold - s * kSliceTopics;               // position of the old topic inside this slice, if any
#pragma unroll
            for (int u = 0; u < kSliceUnits; ++u) {
              if (rel == 2 * u) ph[u].a = own;
              if (rel == 2 * u + 1) ph[u].b = own;
            }
          }
          if (j < NS) {                                            // UPLDA:1509-1513 / MSLDA:196-203
#pragma unroll
            for (int u = 0; u < kSliceUnits; ++u) {
              sum += ((double)n[2 * u] + al[u].a) * ph[u].a;
              sum += ((double)n[2 * u + 1] + al[u].b) * ph[u].b;
            }
            if (j == NS - 1) {                                     // UPLDA:1519-1520; the walk runs negated, see ggs_z_sliced.hpp
              const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
              U = z_uniform(gtok, p.iteration, p.seed);
              tt = 0.0 - U * sum;
            }
          } else {                                                 // UPLDA:1522-1526
            uint32_t bits = 0;
#pragma unroll
            for (int u = 0; u < kSliceUnits; ++u) {
              bits = __builtin_amdgcn_alignbit(bits, (uint32_t)hi32(tt), 31);
              tt += ((double)n[2 * u] + al[u].a) * ph[u].a;
              bits = __builtin_amdgcn_alignbit(bits, (uint32_t)hi32(tt), 31);
              tt += ((double)n[2 * u + 1] + al[u].b) * ph[u].b;
            }
            newc += __popc(bits);
          }
        }
        ring_release_issued();
      }
      gs = (gs + 2 * NS) % kPcgsRingSlots;

      if (active) {
        int new_topic = newc - 1;
        if (POLYAURN && (len == 1 || sum == 0.0)) {                // the walk above ran in lockstep; its result is not used
          new_topic = polyaurn_uniform_topic(U, K);
        } else if (new_topic < 0 || hi32(tt) < 0) {                // UPLDA:1529-1531
          atomicOr(p.status, ST_INVALID_TOPIC);
          new_topic = new_topic < 0 ? 0 : K - 1;
        }
        cnt[new_topic * 64 + lane] += 1;                           // UPLDA:1535
        p.z[beg + t] = new_topic;
        p.zw[ip] = new_topic;
      }
      asm volatile("" ::: "memory");
      w = w1;
#pragma unroll
      for (int m = 0; m < 8; ++m) ra[m] = ran[m];
    }
  }
}
template <bool COLLAPSED>
__global__ __launch_bounds__(64) void pcgs_z_kernel(PcgsParams p) { pcgs_z_body<COLLAPSED, false>(p); }
__global__ __launch_bounds__(64) void polyaurn_z_kernel(PcgsParams p) { pcgs_z_body<false, true>(p); }

}  // namespace ggs

// ------------------------------------------------------------------------------------------------
// pcgs_sliced_kernel<KMAX>: the same z loop for K <= kSlicedMaxTopics with the token's K scores kept in
// registers (as the cold-chunk loop of ggs_z_sliced.hpp keeps them), so the rows stream through the ring
// ONCE per step: half the LDS-DMA instructions of pcgs_z_kernel, and those are what a step costs.
// Same lane-per-document groups, same int16 [k][lane] counts in LDS, same 3-slot ring with the slice
// offset as the DMA immediate (the ring therefore starts above the alpha row and the counts).
// One body, pcgs_sliced_body<KMAX, COLLAPSED, POLYAURN>, for pcgs_sliced_kernel and polyaurn_sliced_kernel, as pcgs_z_body
// is for the streaming pair.
namespace ggs {

template <int KMAX, bool COLLAPSED, bool POLYAURN>
__device__ __forceinline__ void pcgs_sliced_body(PcgsParams &p) {
  constexpr int NS = (KMAX + kSliceTopics - 1) / kSliceTopics;
  constexpr int kAhead = NS < kPcgsRingSlots - 1 ? NS : kPcgsRingSlots - 1;
  constexpr int kHead = pcgs_sliced_head_bytes(KMAX);              // alpha row + counts, below the ring (>= NS*128)
  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int K = p.K;
  double *alb = reinterpret_cast<double *>(smem);                  // alpha, zero padded to KMAX
  int16_t *cnt = reinterpret_cast<int16_t *>(smem + KMAX * 8);     // [KMAX][64]
  unsigned char *ring = smem + kHead;
  const unsigned char *phib = reinterpret_cast<const unsigned char *>(p.phiT);
  const size_t rowbytes = (size_t)p.Kp * 8;
  const unsigned char *my_row = ring_lane_row(ring, lane);
  const int rot = ring_lane_rotation(lane);
  const int16_t *my_cnt = cnt + lane;

  for (int k = lane; k < KMAX; k += 64) alb[k] = k < K ? p.alpha[k] : 0.0;

  const int64_t groups = (p.num_docs + 63) / 64;
  for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
    const int64_t di = g * 64 + lane;
    const int d = di < p.num_docs ? p.order[di] : -1;
    const int64_t beg = d >= 0 ? p.doc_ptr[d] : 0;
    const int len = d >= 0 ? (int)(p.doc_ptr[d + 1] - beg) : 0;
    const int steps = __shfl(len, 0);                              // lane 0 holds the group's longest document
    if (steps == 0) break;                                         // sorted: every later group is empty too
    for (int k = 0; k < KMAX; ++k) cnt[k * 64 + lane] = 0;         // UPLDA:1482-1485 localTopicCounts
    for (int t = 0; t < len; ++t) cnt[p.z[beg + t] * 64 + lane] += 1;

    int w = len > 0 ? p.tok[beg] : 0;
    const unsigned char *ra[8], *ran[8];
    ring_row_addresses(phib, rowbytes, w, lane, ra);
    int gs = 0;
    static_for<0, kAhead>([&](auto sc) { ring_issue<decltype(sc)::value>(ring, decltype(sc)::value % kPcgsRingSlots, ra); });
    int znext = len > 0 ? p.z[beg] : 0;                            // old topic and (COLLAPSED) its own-token psi, one step ahead (see pcgs_z_kernel)
    auto own_of = [&](const int word, const int topic) {
      return (p.beta + (double)(p.n_wk[(size_t)word * K + topic] - 1)) / (p.beta_sum + (double)(p.n_k[topic] - 1));
    };
    double own_next = (COLLAPSED && len > 0) ? own_of(w, znext) : 0.0;

    for (int t = 0; t < steps; ++t) {
      const bool active = t < len, has1 = t + 1 < steps;
      gs = __builtin_amdgcn_readfirstlane(gs);
      const int zold = znext;
      const double own = own_next;
      const int ip = active ? p.inv_perm[beg + t] : 0;
      const int w1 = (t + 1 < len) ? p.tok[beg + t + 1] : 0;
      znext = (t + 1 < len) ? p.z[beg + t + 1] : 0;
      if (COLLAPSED && t + 1 < len) own_next = own_of(w1, znext);
      if (has1) ring_row_addresses(phib, rowbytes, w1, lane, ran);
      if (active) cnt[zold * 64 + lane] -= 1;                      // UPLDA:1494
      asm volatile("" ::: "memory");

      double sc[KMAX];
      double sum = 0.0;
      static_for<0, NS>([&](auto sidx) {                           // UPLDA:1509-1513
        constexpr int s = decltype(sidx)::value;
        const int cur = (gs + s) % kPcgsRingSlots;
        const int nxt = (gs + s + kAhead) % kPcgsRingSlots;
        if constexpr (s + kAhead < NS) ring_issue<s + kAhead>(ring, nxt, ra);
        else if (has1) ring_issue<s + kAhead - NS>(ring, nxt, ran);
        ring_wait<kAhead, NS, s>(has1);
        if (active) {
          const unsigned char *rb = my_row + cur * kSliceBytes;
          D2 ph[kSliceUnits], al[kSliceUnits];
          int n[kSliceTopics];
#pragma unroll
          for (int u = 0; u < kSliceUnits; ++u)
            if (s * kSliceTopics + 2 * u + 1 < KMAX) {
              ph[u] = lds_d2(rb + ring_unit_offset(u, rot));
              al[u] = lds_d2(reinterpret_cast<const unsigned char *>(alb) + (s * kSliceTopics + 2 * u) * 8);
              n[2 * u] = my_cnt[(s * kSliceTopics + 2 * u) * 64];
              n[2 * u + 1] = my_cnt[(s * kSliceTopics + 2 * u + 1) * 64];
            }
          if constexpr (COLLAPSED) {
            const int rel = zold - s * kSliceTopics;               // position of the old topic inside this slice, if any
#pragma unroll
            for (int u = 0; u < kSliceUnits; ++u) {
              if (rel == 2 * u) ph[u].a = own;
              if (rel == 2 * u + 1) ph[u].b = own;
            }
          }
#pragma unroll
          for (int u = 0; u < kSliceUnits; ++u) {
            constexpr int k0 = s * kSliceTopics;
            const int k = k0 + 2 * u;
            if (k + 1 < KMAX) {
              sc[k] = ((double)n[2 * u] + al[u].a) * ph[u].a;
              sum += sc[k];
              sc[k + 1] = ((double)n[2 * u + 1] + al[u].b) * ph[u].b;
              sum += sc[k + 1];
            }
          }
        }
        ring_release_issued();
      });
      gs = (gs + NS) % kPcgsRingSlots;

      if (active) {
        const uint64_t gtok = (uint64_t)(p.tok_base + beg + t);
        const U4 o = philox4x32_10((uint32_t)gtok, (uint32_t)(gtok >> 32), (uint32_t)GGS_PURPOSE_Z << 24, p.iteration,
                                   (uint32_t)p.seed, (uint32_t)(p.seed >> 32));
        double tt = 0.0 - u53(o.x, o.y) * sum;                     // UPLDA:1519-1526, negated walk (see ggs_z_sliced.hpp)
        if constexpr (POLYAURN)                                    // decided before the walk (pcgs_z_body): a walk from +0 stops at once
          if (len == 1 || sum == 0.0) tt = 0.0;
        int newc = 0;
        bool live = true;
#pragma unroll
        for (int kb = 0; kb < KMAX; kb += 16) {
          if (live) {
            uint32_t bits = 0;
#pragma unroll
            for (int j = 0; j < 16; ++j)
              if (kb + j < KMAX) {
                bits = __builtin_amdgcn_alignbit(bits, (uint32_t)hi32(tt), 31);
                tt += sc[kb + j];
              }
            newc += __popc(bits);
            live = __any(hi32(tt) < 0);
          }
        }
        int new_topic = newc - 1;
        if (POLYAURN && (len == 1 || sum == 0.0)) {
          new_topic = polyaurn_uniform_topic(u53(o.x, o.y), K);
        } else if (new_topic < 0 || hi32(tt) < 0) {                // UPLDA:1529-1531
          atomicOr(p.status, ST_INVALID_TOPIC);
          new_topic = new_topic < 0 ? 0 : K - 1;
        }
        cnt[new_topic * 64 + lane] += 1;                           // UPLDA:1535
        p.z[beg + t] = new_topic;
        p.zw[ip] = new_topic;
      }
      asm volatile("" ::: "memory");
      w = w1;
#pragma unroll
      for (int m = 0; m < 8; ++m) ra[m] = ran[m];
    }
  }
}
template <int KMAX, bool COLLAPSED = false>
__global__ __launch_bounds__(64) void pcgs_sliced_kernel(PcgsParams p) { pcgs_sliced_body<KMAX, COLLAPSED, false>(p); }
template <int KMAX>
__global__ __launch_bounds__(64) void polyaurn_sliced_kernel(PcgsParams p) { pcgs_sliced_body<KMAX, false, true>(p); }

}  // namespace ggs
