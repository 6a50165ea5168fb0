// ggs_host_plan.hpp -- the launch planner: which kernel instantiation serves a K (the *_kernel_for selectors), plan_launches (every
// launch a handle of (K, V, scheme) can make), the scheme's own plan entry (pcgs_entry) and scheme_of (ggs_config::flags -> Scheme).
#pragma once
#include "ggs_host_state.hpp"

namespace {
// z_sliced_kernel<KMAX> / z_hot_kernel<KMAX> for KMAX = K rounded up to a multiple of 8
#define GGS_KMAX_SWITCH(KERNEL)                                                                                                     \
  switch ((K + 7) / 8) {                                                                                                            \
    case 1: return reinterpret_cast<const void *>(KERNEL<8>);      case 2: return reinterpret_cast<const void *>(KERNEL<16>);       \
    case 3: return reinterpret_cast<const void *>(KERNEL<24>);     case 4: return reinterpret_cast<const void *>(KERNEL<32>);       \
    case 5: return reinterpret_cast<const void *>(KERNEL<40>);     case 6: return reinterpret_cast<const void *>(KERNEL<48>);       \
    case 7: return reinterpret_cast<const void *>(KERNEL<56>);     case 8: return reinterpret_cast<const void *>(KERNEL<64>);       \
    case 9: return reinterpret_cast<const void *>(KERNEL<72>);     case 10: return reinterpret_cast<const void *>(KERNEL<80>);      \
    case 11: return reinterpret_cast<const void *>(KERNEL<88>);    case 12: return reinterpret_cast<const void *>(KERNEL<96>);      \
    case 13: return reinterpret_cast<const void *>(KERNEL<104>);   case 14: return reinterpret_cast<const void *>(KERNEL<112>);     \
    case 15: return reinterpret_cast<const void *>(KERNEL<120>);   case 16: return reinterpret_cast<const void *>(KERNEL<128>);     \
    case 17: return reinterpret_cast<const void *>(KERNEL<136>);   case 18: return reinterpret_cast<const void *>(KERNEL<144>);     \
    case 19: return reinterpret_cast<const void *>(KERNEL<152>);   case 20: return reinterpret_cast<const void *>(KERNEL<160>);     \
    case 21: return reinterpret_cast<const void *>(KERNEL<168>);   case 22: return reinterpret_cast<const void *>(KERNEL<176>);     \
    case 23: return reinterpret_cast<const void *>(KERNEL<184>);   default: return reinterpret_cast<const void *>(KERNEL<192>);     \
  }
const void *sliced_kernel_for(int K) { GGS_KMAX_SWITCH(z_sliced_kernel) }
const void *sliced32_kernel_for(int K) { GGS_KMAX_SWITCH(z_sliced32_kernel) }

const void *hot_kernel_for(int K) { GGS_KMAX_SWITCH(z_hot_kernel) }
const void *warm_kernel_for(int K) { GGS_KMAX_SWITCH(z_warm_kernel) }
const void *pairs_kernel_for(int K) { GGS_KMAX_SWITCH(z_pairs_kernel) }
const void *pcgs_kernel_for(int K) { GGS_KMAX_SWITCH(pcgs_sliced_kernel) }
const void *polyaurn_kernel_for(int K) { GGS_KMAX_SWITCH(polyaurn_sliced_kernel) }
const void *collapsed_kernel_for(int K) {
  switch ((K + 7) / 8) {
#define GGS_CK(N) case N: return reinterpret_cast<const void *>(pcgs_sliced_kernel<8 * N, true>);
    GGS_CK(1) GGS_CK(2) GGS_CK(3) GGS_CK(4) GGS_CK(5) GGS_CK(6) GGS_CK(7) GGS_CK(8) GGS_CK(9) GGS_CK(10) GGS_CK(11) GGS_CK(12)
    GGS_CK(13) GGS_CK(14) GGS_CK(15) GGS_CK(16) GGS_CK(17) GGS_CK(18) GGS_CK(19) GGS_CK(20) GGS_CK(21) GGS_CK(22) GGS_CK(23)
#undef GGS_CK
    default: return reinterpret_cast<const void *>(pcgs_sliced_kernel<192, true>);
  }
}

// pcgs_wave_kernel<NB, COLLAPSED> (scheme polyaurn: polyaurn_wave_kernel<NB>) for NB = blocks of 128 topics, rounded up to a
// power of two
const void *pcgs_wave_kernel_for(int nb, bool collapsed, bool polyaurn) {
#define GGS_WK(N) if (nb <= N) return polyaurn ? reinterpret_cast<const void *>(polyaurn_wave_kernel<N>) : collapsed ? reinterpret_cast<const void *>(pcgs_wave_kernel<N, true>) : reinterpret_cast<const void *>(pcgs_wave_kernel<N, false>);
  GGS_WK(1) GGS_WK(2) GGS_WK(4) GGS_WK(8) GGS_WK(16)
#undef GGS_WK
  return polyaurn ? reinterpret_cast<const void *>(polyaurn_wave_kernel<32>) : collapsed ? reinterpret_cast<const void *>(pcgs_wave_kernel<32, true>) : reinterpret_cast<const void *>(pcgs_wave_kernel<32, false>);
}
constexpr int kPcgsWaveMaxTopics = 32 * 128;          // 4096: two rows of K/64 doubles per lane in registers
// Where the wave-per-document kernel takes over from the lane-per-document score-register kernels (which exist up to 192
// topics; their 176..192 variants spill 12-164 bytes per lane to scratch).  Measured on the benchmark corpus, z step in ms,
// lane-per-document / wave-per-document (round 4, after the wave kernel's rework; the wave kernel's time steps with the
// number of 128-topic blocks: flat up to 128 topics, flat from 129 to 256):
//   pcgs       K = 100: 2.51 / 3.33, 128: 3.69 / 3.3, 144: 4.02 / 4.9, 160: 4.28 / 4.9, 176: 4.69 / 4.9, 192: 6.04 / 5.0
//   collapsed  K = 100: 3.60 / 3.74, 128: 6.31 / 3.71, 144: 6.96 / 5.6, 160: 7.63 / 5.6, 176: 8.62 / 5.6, 192: 11.4 / 5.6
constexpr int kPcgsWaveFromTopics = 176, kCollapsedWaveFromTopics = 96;
// scheme polyaurn: the lane-per-document kernels up to 168 topics -- polyaurn_sliced_kernel<176> spills to scratch where
// pcgs_sliced_kernel<176> spills less, and the two kernels' times are within 10 % of each other there (pcgs above)
constexpr int kPolyaurnWaveFromTopics = 168;

const void *tile_kernel_for(int K) {
  const int nt = (K + 63) / 64;
  return nt <= 1 ? reinterpret_cast<const void *>(z_kernel<1>) : nt <= 2 ? reinterpret_cast<const void *>(z_kernel<2>)
       : nt <= 4 ? reinterpret_cast<const void *>(z_kernel<4>) : nt <= 8 ? reinterpret_cast<const void *>(z_kernel<8>)
       : nt <= 16 ? reinterpret_cast<const void *>(z_kernel<16>) : reinterpret_cast<const void *>(z_kernel<20>);
}
const void *stream_kernel_for(bool two_pass, bool regck, int group) {
  if (two_pass) return reinterpret_cast<const void *>(z_stream_kernel);
  if (!regck) return reinterpret_cast<const void *>(z_stream1_kernel<false, 4>);
  return group == 1 ? reinterpret_cast<const void *>(z_stream1_kernel<true, 1>) : group == 2 ? reinterpret_cast<const void *>(z_stream1_kernel<true, 2>)
                                                                                             : reinterpret_cast<const void *>(z_stream1_kernel<true, 4>);
}
// the lane-per-document kernel of a scheme: scores in registers (K <= 192), or streamed
const void *pcgs_lane_kernel_for(int K, bool sliced, bool collapsed, bool polyaurn) {
  if (sliced) return collapsed ? collapsed_kernel_for(K) : polyaurn ? polyaurn_kernel_for(K) : pcgs_kernel_for(K);
  return collapsed ? reinterpret_cast<const void *>(pcgs_z_kernel<true>) : polyaurn ? reinterpret_cast<const void *>(polyaurn_z_kernel) : reinterpret_cast<const void *>(pcgs_z_kernel<false>);
}

// The resident single-wave workgroups per CU of a persistent grid (exactly what is resident: a workgroup that is not would walk
// its share only after the others have finished theirs): what the kernel's registers allow (asked of the runtime, whose answer
// ignores the LDS allocation granule) and what LDS allows, at most the CU's 32.
int resident_waves_per_cu(const void *fn, int lds) {
  int by_regs = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&by_regs, fn, 64, (size_t)lds) != hipSuccess || by_regs < 1) by_regs = 1;
  return lds_workgroups_per_cu(lds, std::min(by_regs, 32));
}

// Every launch a handle of (K, V, scheme) can make on the device: which kernel, how much LDS (the layout functions beside
// the kernels), how many workgroups per CU.  No environment, no handle; the only HIP calls are the occupancy queries of the
// two wave-per-document kernels.
int plan_launches(const int K, const int V, const Scheme scheme, const Knobs &kn, LaunchPlan &pl) {
  const int Kp = (K + 1) & ~1, pitch16 = (Kp / 2) | 1;
  // ---- the histograms of the hyperparameter step, whatever the scheme: four waves per workgroup, a document or a run of cells per wave and trip
  if (doc_hist_lds_bytes(K) <= (size_t)kMaxLdsBytes) {
    pl.dochist = {reinterpret_cast<const void *>(doc_topic_hist_kernel), kHistBlock, (int)doc_hist_lds_bytes(K), 0};
    pl.dochist.per_cu = lds_workgroups_per_cu(pl.dochist.lds, kHistPerCu);
  }
  pl.cellhist = {reinterpret_cast<const void *>(cell_hist_kernel), kHistBlock, kCellHistLdsBytes, kHistPerCu};
  if (scheme == Scheme::ggs) {                        // ---- the ggs z step
    // score-register kernels up to K = 160: measured on the benchmark corpus (sweep, ms; round 3) K=136: 2.13 sliced / 2.40
    // streaming, 152: 2.33 / 2.56, 160: 2.40 / 2.50, 164: 3.06 / 2.83, 168: 3.06 / 2.75, 184: 3.24 / 2.94 (round 2: 184: 3.55 /
    // 3.64, 192: 4.22 / 3.59) -- from KMAX = 168 on the cold kernel fills the whole register file (256 + 256) and the one-pass
    // streaming kernel with the next theta drawn beside it wins (the sliced kernels can take K up to kSlicedMaxTopics = 192:
    // GGS_DEBUG_ZKERNEL=1).  The sliced kernel tags chunk tokens (word ids) in bit 30.
    const bool sliced_ok = K <= kSlicedMaxTopics && V < (1 << kSlotShift);
    bool sliced = sliced_ok && K <= kSlicedDefaultTopics, stream = !sliced && K > 2 * kSliceTopics, two_pass = false;
    if (kn.zkernel.set) {          // 0: whole-row tile kernel, 1: sliced where possible, 2: streaming kernel where it applies, 3: its two-pass form
      const int mode = kn.zkernel.v;
      sliced = sliced_ok && mode == 1;
      stream = (mode == 2 || mode == 3) ? K > 2 * kSliceTopics : (stream && mode != 0);
      two_pass = mode == 3;
      if (sliced) stream = false;
    }
    pl.kernel = sliced ? 1 : stream ? (two_pass ? 3 : 2) : 0;
    // The z waves are persistent and stride the chunk table statically, so a grid is what is truly co-resident
    // (lds_workgroups_per_cu); the passes are latency chains, so waves in flight matter more than lanes in use.
    if (stream) {
      // 64-token chunks, a 2-slot slice ring + the theta row zero-padded to whole slices (one-pass kernel: to whole
      // checkpoint groups, plus a checkpoint per group and lane); no score registers, so 8 waves per CU fit the
      // register file and LDS bounds the residency
      const int ns = stream_slices(K);
      // checkpoint group: the smallest that keeps the checkpoints in registers (K <= 256: one slice, <= 512: two, <= 1024: four); beyond, four slices and LDS
      int group = ns <= kRegCheckpoints ? 1 : ns <= 2 * kRegCheckpoints ? 2 : 4;
      if (kn.group.set && (kn.group.v == 1 || kn.group.v == 2 || kn.group.v == 4)) group = kn.group.v;
      bool regck = !two_pass && z_stream1_groups(K, group) <= kRegCheckpoints;          // checkpoints in registers or in LDS
      if (kn.regck.set) regck = regck && kn.regck.v != 0;
      if (!regck) group = 4;                               // the LDS-checkpoint kernel is instantiated for groups of four
      // Chunks of 64 consecutive tokens across ONE document boundary (two theta rows per wave) instead of near-equal
      // cuts of single documents: 98 % of the lanes busy instead of 78 % at 200-token documents.  Where the second row
      // would cost resident waves (K > 512: 8 KiB at K = 1024) the single-document chunks stay.
      pl.two_rows = !two_pass && (kn.tworows.set ? kn.tworows.v != 0 : K <= 512);
      pl.z.fn = stream_kernel_for(two_pass, regck, group);
      pl.z.lds = two_pass ? z_stream_lds_bytes(K) : z_stream1_lds_bytes(K, group, pl.two_rows, regck);
      if (pl.z.lds > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;   // K > ~16000: the theta row itself would need slicing
    } else if (sliced) {
      // 64-token chunks; one 4-wave workgroup per CU (a wave per SIMD: the score registers take most of the 512-entry file),
      // per wave the two theta rows and the slice ring, per workgroup the hot-word table.  The cold chunks from phiT32 (a
      // 32-topic slice per 128 bytes); its wave LDS is the fp64 form's: the ring, then two float32 theta rows and the
      // replay's KMAX products where the two fp64 theta rows were
      pl.f32 = !kn.phi64.is(1);
      pl.Kp32 = round_up(K, kSlice32Topics);
      pl.ring_base = sliced_ring_base(K); pl.wave_lds = sliced_wave_lds(K); pl.hot_pitch = table_row_pitch(K);
      pl.hot_wave_lds = hot_wave_lds(K); pl.warm_wave_lds = warm_wave_lds(K);
      if (kn.split.set) { pl.split = kn.split.v != 0; pl.split_forced = kn.split.v == 2; }
      // split: the two workgroups must fit one CU together
      // the hot words by pair-chunks wherever the split form can run; the pairs' records take LDS the table had (K = 100: 79 rows
      // for 96), and the rows given up are the head of the first warm tier.  Set where the split form is merely possible: if the
      // first z step's timed comparison then keeps the fused form, the run has the smaller table and the pair lists were built
      // and uploaded for the comparison's split steps alone (the benchmark keeps the split form)
      pl.hot_pairs = pl.split && !kn.hot_pairs.is(0);
      pl.pairs_wave_lds = pairs_wave_lds(K);
      pl.hot_cap = !pl.split ? table_rows_fused(K) : table_rows_beside_cold(K, pl.hot_pairs ? std::max(pl.hot_wave_lds, pl.pairs_wave_lds) : pl.hot_wave_lds);
      if (kn.hot.set) pl.hot_cap = std::max(0, std::min(pl.hot_cap, kn.hot.v));
      pl.cold = {pl.f32 ? sliced32_kernel_for(K) : sliced_kernel_for(K), kSlicedWaves * 64, sliced_cold_lds(K), 1};
      pl.hot = {hot_kernel_for(K), kSlicedWaves * 64, table_lds(K, pl.hot_wave_lds, 0), 1};
      if (pl.hot_pairs) pl.pairs = {pairs_kernel_for(K), kSlicedWaves * 64, table_lds(K, pl.pairs_wave_lds, 0), 1};
      // the warm tiers: the same LDS beside the cold kernel's workgroup, more of it for theta rows (warm_docs per wave), the rest a table
      pl.warm = {warm_kernel_for(K), kSlicedWaves * 64, table_lds(K, pl.warm_wave_lds, 0), 1};
      pl.warm_docs = warm_docs_for(sliced_kmax(K));
      pl.warm_cap = table_rows_beside_cold(K, pl.warm_wave_lds);
      if (pl.warm_cap < 16) pl.warm_cap = 0;               // the table loads and barriers of a tier want tokens to pay them
      if (kn.warm.set) pl.warm_tiers_max = std::max(0, std::min(kWarmMaxTiers, kn.warm.v));
      if (kn.warm_rows.set) pl.warm_cap = std::max(0, std::min(pl.warm_cap, kn.warm_rows.v));
      if (kn.warm_fill.set) pl.warm_min_fill_pct = std::max(1, std::min(100, kn.warm_fill.v));
      if (kn.warm_cpw.set) pl.warm_min_chunks_per_wave = std::max(0, kn.warm_cpw.v);
    } else {
      // a tile of T token rows + one theta row per wave: the largest tile that still lets 6 single-wave workgroups share a
      // CU, but at least 8 rows
      int T = z_tile_rows_in(kMaxLdsBytes / 6 / kLdsGranule * kLdsGranule, Kp, pitch16);
      if (kn.tile.set) T = kn.tile.v;
      pl.tile_tokens = std::max(8, std::min(64, T));
      pl.z.fn = tile_kernel_for(K);
      pl.z.lds = z_tile_lds_bytes(Kp, pitch16, pl.tile_tokens);
      if (pl.z.lds > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;   // K > ~2400 needs a K-sliced kernel
    }
    if (!sliced) {
      pl.z.per_cu = lds_workgroups_per_cu(pl.z.lds, 8);
      if (kn.wpc.set) pl.z.per_cu = std::max(1, kn.wpc.v);
    }
  }
  // ---- the theta draw: of every sweep for scheme ggs, of the log posterior's diagnostic theta for the pcgs family
  // The documents per workgroup: by the cells alone (theta_cells_lds_bytes: the 32 KiB were measured before the cell list
  // and the class-A table came beside the cells); 32 or more are halved where the whole workgroup would pass the quarter
  // of the CU's LDS below (K = 96 - 115: 16 instead of 32, at K = 100 35.4 KiB; K = 46 - 57: 32 instead of 64).  Not below 16: with 8
  // documents the two serial K-chains of a workgroup take over (K = 200, 18 846 documents: the draw 0.48 ms instead of 0.25).
  const int theta_quarter = (kMaxLdsBytes - 24 * 1024) / 4;
  int B = 64;
  while (B > 1 && (theta_cells_lds_bytes(K, B) > 32 * 1024 || (B > 16 && theta_lds_bytes(K, B) > theta_quarter))) B >>= 1;
  if (theta_lds_bytes(K, B) > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;
  pl.theta.fn = reinterpret_cast<const void *>(theta_kernel<kThetaBlock>); pl.theta.block = kThetaBlock;
  // The request is padded to a quarter of the CU's LDS: at most 4 workgroups (16 waves) of the theta draw per CU.
  // It runs on the side stream beside the Phi phase, which is the critical path; stream priority orders dispatch,
  // not running waves, and measured with 5-6 resident workgroups theta finishes early (0.53 ms instead of 0.75)
  // while the Phi phase it starves gets longer (0.67 -> 0.72 ms).
  // ... and 24 KiB of every CU stay free for the main stream's own LDS users (the walk of the exact column sums,
  // 20.5 KiB of static LDS per workgroup, 22 KiB allocated: with the CU's LDS handed out to theta workgroups to the last
  // granule it waited for the theta draw to END -- 5 ms at K = 1024).  Workgroups of 16 documents at K = 193 - 227 pass
  // the quarter with their list (K = 200: 35.3 KiB, 36 allocated): four of them leave 16 KiB, and the walk takes the 36 KiB
  // that one of them frees when it ends.  That configuration draws theta only where the z step is in one part (D <= V: few
  // rounds of theta workgroups; measured there, 1.005 -> 0.989 ms per sweep against the build without the list).
  pl.cfg_plain = {1, pl.z.per_cu, B, std::max(theta_lds_bytes(K, B), theta_quarter), 0};
  // ... unless the theta draw is the critical leg itself (theta_main): then five workgroups per CU, of 16 documents
  // each.  Measured at K = 100 on one box, ms per sweep (documents per workgroup x workgroups per CU): 32x4 1.60-1.61,
  // 32x5 1.598-1.62, 24x5 1.593, 16x4 1.614, 16x5 1.568-1.587, 16x6 1.58, 16x8 1.598, 12x5 1.609, 8x8 1.635 -- the smaller
  // workgroups leave the Phi chain beside them its pace (0.39 ms against 0.44), so that it ends before the theta draw does.
  pl.theta_docs_main = kn.theta_b.set ? std::max(1, std::min(B, kn.theta_b.v)) : std::min(B, 16);
  pl.theta_lds_main = std::max(theta_lds_bytes(K, pl.theta_docs_main), (kMaxLdsBytes - 24 * 1024) / (kn.theta_wgs.set ? std::max(1, kn.theta_wgs.v) : 5));
  // K > 192 (one-pass streaming z kernel): theta workgroups small enough to sit BESIDE the z waves -- on the LDS the z
  // waves give up -- so that the next theta of a part of the documents is drawn while the following parts are sampled
  // (z_phase).  The padded request caps them at kBeside per CU while z runs.
  pl.cfg_parts = pl.cfg_plain;
  if (scheme == Scheme::ggs) {                        // the parts of the one-pass streaming kernel's z step (pl.kernel == 2)
    pl.parts_forced = kn.zparts.set;
    int parts = kn.zparts.set ? std::max(1, std::min(8, kn.zparts.v)) : pl.kernel == 2 ? 8 : 1;   // measured at K = 1024: 1 part 18.4 ms per sweep, 2: 18.1, 4: 16.5, 8: 15.9
    if (parts > 1 && pl.kernel == 2) {
      const int kBeside = kn.beside.set ? std::max(1, kn.beside.v) : 4;   // measured at K = 1024 (sweep): 2 -> 16.9 ms, 3 -> 16.1, 4 -> 15.0, 5 -> 15.0
      // The z waves and the documents per workgroup are the ones the cells alone allow (as measured, before the cell
      // list came beside the cells).  Where the list takes the request over a granule that the z waves' remainder does not
      // have four times (K = 161-164, 234-256, 513-572, 769-828, 1153-1280), three theta workgroups sit beside the z waves
      // instead of kBeside.  Measured against the other two ways at K = 161 / 256 / 520, ms per sweep (without the list
      // 2.881 / 3.600 / 8.993): this 2.884 / 3.581 / 8.704, a z wave less 2.969 / 3.674 / 8.931, half the documents 4.12 at 256.
      const int z_alloc = lds_alloc_of(pl.z.lds);
      auto z_waves_beside = [&](int theta_lds) { return std::min(pl.z.per_cu, (kMaxLdsBytes - kLdsGranule - kBeside * lds_alloc_of(theta_lds)) / z_alloc); };
      int Bt = 64;
      while (Bt > 1 && theta_cells_lds_bytes(K, Bt) > 10 * 1024) Bt >>= 1;
      const int zw = z_waves_beside(theta_cells_lds_bytes(K, Bt));
      const int t_lds = theta_lds_bytes(K, Bt);
      if (theta_cells_lds_bytes(K, Bt) <= 12 * 1024 && zw >= 2)
        pl.cfg_parts = {parts, zw, Bt, std::max(t_lds, theta_quarter), std::max(t_lds, (kMaxLdsBytes - kLdsGranule - zw * z_alloc) / kBeside / kLdsGranule * kLdsGranule)};
      else
        parts = 1;
    }
    pl.cfg_parts.parts = parts;
    return GGS_OK;
  }

  // ---- the pcgs family: a lane or a wave per document; the alias schemes' table build and their own z kernel
  const bool collapsed = scheme == Scheme::collapsed, polyaurn = scheme == Scheme::polyaurn;
  // the wave-per-document kernel: any K up to 4096, any document length.  Waves per CU (the grid is persistent: exactly what
  // is resident): what the kernel's registers allow (asked of the runtime) and what LDS allows (the runtime's answer
  // ignores the allocation granule)
  if (K <= kPcgsWaveMaxTopics) {
    const int nb = pcgs_wave_blocks(Kp);
    pl.wave.fn = pcgs_wave_kernel_for(nb, collapsed, polyaurn);
    pl.wave.lds = pcgs_wave_lds_bytes(nb);
    pl.wave.per_cu = resident_waves_per_cu(pl.wave.fn, pl.wave.lds);
  }
  pl.wave_forced = kn.pcgs_wave.set ? kn.pcgs_wave.v != 0 : K > (collapsed ? kCollapsedWaveFromTopics : polyaurn ? kPolyaurnWaveFromTopics : kPcgsWaveFromTopics);
  if (pl.wave_forced && !pl.wave.fn) return GGS_ERR_UNSUPPORTED;   // more than 4096 topics
  // the lane-per-document kernel: its waves per CU also size the padded document order, whichever kernel runs
  const bool lane_sliced = K <= kSlicedMaxTopics && !(kn.pcgs_stream.set && kn.pcgs_stream.v != 0);
  pl.lane.lds = lane_sliced ? pcgs_sliced_lds_bytes(K) : pcgs_z_lds_bytes(K);
  if (pl.lane.lds > kMaxLdsBytes && !pl.wave_forced) return GGS_ERR_UNSUPPORTED;
  pl.lane.per_cu = lds_workgroups_per_cu(pl.lane.lds, 8);
  if (!pl.wave_forced) pl.lane.fn = pcgs_lane_kernel_for(K, lane_sliced, collapsed, polyaurn);
  if (collapsed) pl.serial.fn = reinterpret_cast<const void *>(collapsed_serial_kernel);
  if (has_alias(scheme)) {
    pl.alias_wpb = alias_words_per_block(K);
    pl.alias = {reinterpret_cast<const void *>(alias_build_kernel), 64, (int)alias_lds_bytes(K, pl.alias_wpb), 0};
    pl.alias.per_cu = lds_workgroups_per_cu(pl.alias.lds, 16);
  }
  if (doubly_sparse(scheme)) pl.wordlist = {reinterpret_cast<const void *>(word_list_build_kernel), kWordListBlock, 0, 8};   // a wave per word, four to a workgroup
  // the z kernels of the sparse walks and of adlda: their LDS comes with the corpus
  if (scheme == Scheme::spalias) pl.spalias.fn = reinterpret_cast<const void *>(spalias_wave_kernel);
  if (scheme == Scheme::polyaurn_sparse) pl.pusparse.fn = reinterpret_cast<const void *>(polyaurn_sparse_wave_kernel);
  if (scheme == Scheme::nzvsspalias) {                 // the list build from the drawn cells, the chain's kernels (LDS by V, a workgroup per topic) and the z step
    pl.wordmask = {reinterpret_cast<const void *>(word_list_mask_kernel), kWordListBlock, 0, 8};
    pl.vsbits = {reinterpret_cast<const void *>(vs_bits_kernel), 64, 0, 32};
    const bool global = V > kVsLdsMaxV || (kn.vs_global.set && kn.vs_global.v != 0);
    pl.vschain = {global ? reinterpret_cast<const void *>(vs_chain_kernel<true>) : reinterpret_cast<const void *>(vs_chain_kernel<false>), kVsBlock,
                  global ? 0 : (int)vs_chain_lds_bytes((V + 31) / 32), 1};
    pl.nzvs.fn = reinterpret_cast<const void *>(nzvs_wave_kernel);
  }
  if (scheme == Scheme::lightpclda) {
    // as many resident waves as fit: a lone wave issues at a fraction of a SIMD's rate, and the step is a chain of dependent operations
    pl.lightpc = {reinterpret_cast<const void *>(lightpc_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightpc.per_cu = resident_waves_per_cu(pl.lightpc.fn, pl.lightpc.lds);
  }
  if (count_tables(scheme)) {
    // the tables over the counts: alias_build_kernel's words per workgroup and residency; the z step: lightpc's rule
    pl.alias_wpb = alias_words_per_block(K);
    pl.countalias = {reinterpret_cast<const void *>(count_alias_build_kernel), 64, (int)count_alias_lds_bytes(K, pl.alias_wpb), 0};
    pl.countalias.per_cu = lds_workgroups_per_cu(pl.countalias.lds, 16);
  }
  if (scheme == Scheme::lightpcldaw2) {
    pl.lightpcw2 = {reinterpret_cast<const void *>(lightpcw2_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightpcw2.per_cu = resident_waves_per_cu(pl.lightpcw2.fn, pl.lightpcw2.lds);
  }
  if (scheme == Scheme::lightcollapsed) {
    pl.lightcol = {reinterpret_cast<const void *>(lightcollapsed_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightcol.per_cu = resident_waves_per_cu(pl.lightcol.fn, pl.lightcol.lds);
  }
  if (scheme == Scheme::adlda) {                       // one wave for the head, a wave per word for the lists; the z kernel's LDS comes with the corpus
    pl.adhead = {reinterpret_cast<const void *>(adlda_head_kernel), 64, 0, 1};
    pl.adlists = {reinterpret_cast<const void *>(word_list_counts_kernel), kWordListBlock, 0, 8};
    pl.adlda.fn = reinterpret_cast<const void *>(adlda_wave_kernel);
  }
  return GGS_OK;
}

const KernelLaunch &pcgs_entry(const LaunchPlan &pl, Scheme s, bool wave) {
  return row_of(s).entry ? pl.*row_of(s).entry : wave ? pl.wave : pl.lane;
}

// The scheme a configuration asks for (`poisson_L`: polyaurn's alias_poisson_threshold), or what is wrong with the request:
// answered before any device is asked for.
int scheme_of(const ggs_config *cfg, Scheme &scheme, int32_t &poisson_L) {
  const int32_t f = cfg->flags;
  scheme = Scheme::ggs;
  for (int i = 0; i < kNumSchemes; ++i) {              // the rows stand in the order of their bits: the highest bit set names the scheme
    if (!(f & kSchemes[i].flag)) continue;
    if (f & kSchemes[i].refused) return GGS_ERR_BAD_ARG;
    scheme = (Scheme)i;
  }
  poisson_L = cfg->alias_poisson_threshold == 0 ? 100 : cfg->alias_poisson_threshold;   // LDAConfiguration.java:44
  if (poisson_phi(scheme) && ((f & GGS_FLAG_COLLAPSED) || poisson_L < 1 || poisson_L > kPoissonMaxThreshold)) return GGS_ERR_BAD_ARG;
  if (wave_only(scheme) && cfg->num_topics > kPcgsWaveMaxTopics) return GGS_ERR_UNSUPPORTED;
  return GGS_OK;
}
}  // namespace
