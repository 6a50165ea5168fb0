// ggs_host_sweep.hpp -- the sweep scheduler: the theta draw, the z launches of both families, z_phase (what runs beside what, on
// which stream), the sweep's end (finish_sweep*) and its settling (settle_sweeps), the iteration's bounds, java.util.Random.
#pragma once
#include "ggs_host_phi.hpp"

namespace {
// `lds`, `docs_per_block`: 0 = those of the corpus' configuration (plan.cfg_plain / cfg_parts)
int launch_theta(ggs_handle *h, hipStream_t stream, double *dst, int32_t iteration, int64_t d0 = 0, int64_t d1 = -1, int32_t lds = 0, int32_t docs_per_block = 0) {
  if (d1 < 0) d1 = h->D;
  if (d1 <= d0) return GGS_OK;
  if (docs_per_block <= 0) docs_per_block = h->cfg->theta_docs;
  ThetaParams tp{};
  tp.doc_ptr = h->d_doc_ptr + d0; tp.z = h->d_z; tp.alpha = h->d_alpha; tp.theta = dst + (size_t)d0 * h->K; tp.status = h->d_status;
  tp.num_docs = d1 - d0; tp.doc_base = h->doc_base + d0; tp.seed = h->seed; tp.iteration = (uint32_t)iteration;
  tp.K = h->K; tp.docs_per_block = docs_per_block; tp.queue_cap = std::min(kGammaQueue, h->gamma_queue_cap);
  tp.sym_alpha = h->alpha_symmetric ? 1 : 0;
  const int64_t grid = (d1 - d0 + docs_per_block - 1) / docs_per_block;
  void *args[] = {&tp};
  HIP_TRY(h, hipLaunchKernel(h->plan.theta.fn, dim3((unsigned)grid), dim3(kThetaBlock), args, (size_t)(lds ? lds : h->cfg->theta_lds), stream));
  return GGS_OK;
}

int launch_pcgs_z(ggs_handle *h) {
  if (h->N == 0) return GGS_OK;
  PcgsParams pp{};
  pp.tok = h->d_tok; pp.inv_perm = h->d_inv_perm; pp.z = h->d_z; pp.zw = h->d_zw; pp.doc_ptr = h->d_doc_ptr; pp.order = h->d_order;
  pp.alpha = h->d_alpha; pp.phiT = h->d_phiT; pp.status = h->d_status;
  pp.num_docs = h->pcgs_order_len; pp.tok_base = h->tok_base; pp.seed = h->seed; pp.iteration = (uint32_t)h->iteration;   // the length of the (padded) order list
  pp.K = h->K; pp.Kp = h->Kp;
  int rc;
  if (h->alias_stale && (rc = launch_alias_build(h))) return rc;   // the schemes with tables over Phi
  if (count_form(h->scheme) || count_tables(h->scheme)) {   // lightpcldaw2 too: Phi as it stands, the lists and tables of the corpus-wide sweep-start counts
    if ((rc = launch_sweep_head(h))) return rc;
    pp.n_wk = h->d_n_wk; pp.n_k = h->d_n_k; pp.beta = h->beta; pp.beta_sum = h->beta_sum;   // betaSum: beta * numTypes (MSLDA:136) until ggs_set_hyperparameters gives another
  }
  PolyaurnSparseParams sp{};                           // spalias's kernel takes its base, SpaliasParams
  LightCountParams lp{};                               // lightpclda's kernel takes its base, LightpcParams
  AdldaParams ad{};
  void *args[] = {&pp, &h->margin_scale};              // the wave-per-document kernel takes both, the lane-per-document kernels the first
  if (sparse_walk(h->scheme)) {
    // one wave per document over its non-zero topics (ggs_z_spalias.hpp), or over the word's where they are fewer
    // (ggs_z_polyaurn_sparse.hpp: the lists and the counters, null in a spalias handle)
    sp.b = pp; sp.ps = h->d_alias_ps; sp.a = h->d_alias_a; sp.type_norm = h->d_alias_tn; sp.cap = h->sp_cap; sp.margin_scale = h->margin_scale;
    sp.nzw = h->d_nzw; sp.nw = h->d_nw; sp.stats = h->d_ps_stats;
    args[0] = static_cast<SpaliasParams *>(&sp);
  } else if (has_mh(h->scheme)) {
    // one wave per document, two proposals per token (ggs_z_light.hpp): over spalias's tables (lightpclda), or over the lists and
    // tables of the sweep-start counts (lightcollapsed, lightpcldaw2; null in a lightpclda handle)
    lp.b = pp; lp.ps = h->d_alias_ps; lp.a = h->d_alias_a; lp.mh = h->d_mh; lp.alpha_sum = h->alpha_sum;
    lp.nzw = h->d_nzw; lp.nw = h->d_nw; lp.tpt = h->d_tpt;
    args[0] = static_cast<LightpcParams *>(&lp);
  } else if (h->scheme == Scheme::adlda) {             // one wave per document over den0, S0 and the lists of the sweep-start counts
    ad.b = pp; ad.den0 = h->d_ad_den0; ad.s0 = h->d_ad_s0; ad.nzw = h->d_nzw; ad.nw = h->d_nw; ad.stats = h->d_ps_stats; ad.cap = h->sp_cap; ad.margin_scale = h->margin_scale;
    args[0] = &ad;
  }
  HIP_TRY(h, launch(h, h->pcgs_z, h->pcgs_items, args, h->stream));
  return GGS_OK;
}

// `count`: with an exchange the sliced kernels add every token's new (word, topic) cell into the (zeroed) send buffer of the
// count reduce-scatter themselves; the timed comparison of the two z forms launches without it
// ... where few tokens share a cell: the atomics of different XCDs on one line serialise at the memory side.  Measured on the
// benchmark corpus split N ways (z step with / without them, and the count kernel they replace): N = 8 (50 tokens per word
// on the rank) 0.139 / 0.132 ms against 0.040 of count kernel; N = 4 (100) 0.290 / 0.26 against 0.05; N = 2 (200) 0.627 / 0.52
// against 0.07 -- they pay up to about 64 tokens per word (GGS_DEBUG_ZCOUNTS=2 forces them).
bool z_counts_itself(const ggs_handle *h) {
  return h->xg && h->z_counts && h->plan.sliced() && (h->z_counts_forced || h->N <= (int64_t)64 * h->V) && !use_sparse(h);
}
// `defer_join` (with `count`, split form): the hot words' count launch follows the hot kernel on ITS stream and the
// handle's stream is not made to wait for that stream here -- the caller does (join_hot_stream), behind the z step's end
// event, so that the hot chunks' count sits beside the tail of the cold kernel instead of behind it.
int launch_z(ggs_handle *h, bool force_fused = false, int64_t c0 = 0, int64_t c1 = -1, bool count = false, bool defer_join = false) {
  h->hot_join_pending = false;
  if (h->N == 0) return GGS_OK;
  const LaunchPlan &pl = h->plan;
  ZParams zp{};
  zp.tok = h->d_tok; zp.inv_perm = h->d_inv_perm; zp.z = h->d_z; zp.zw = h->d_zw; zp.chunk_start = h->d_chunk_start; zp.chunk_doc = h->d_chunk_doc; zp.chunk_len = h->d_chunk_len;
  zp.theta = h->d_theta; zp.phiT = h->d_phiT; zp.status = h->d_status;
  zp.tok_base = h->tok_base; zp.seed = h->seed; zp.iteration = (uint32_t)h->iteration;
  zp.K = h->K; zp.Kp = h->Kp; zp.pitch16 = h->pitch16; zp.tile_tokens = pl.tile_tokens;
  zp.margin_scale = h->margin_scale;
  zp.chunk_doc1 = h->d_chunk_doc1; zp.two_rows = (pl.two_rows && h->d_chunk_doc1) ? 1 : 0;
  zp.ct_tok = h->d_ct_tok; zp.ct_idx = h->d_ct_idx; zp.ct_ip = h->d_ct_ip; zp.c_docs = h->d_c_docs; zp.num_cold = h->Cc;
  zp.hot_words = h->d_hot_words; zp.num_hot = h->num_hot; zp.hot_pitch = pl.hot_pitch;
  zp.wave_lds = pl.wave_lds; zp.hot_off = kSlicedWaves * pl.wave_lds; zp.ring_base = pl.ring_base;
  zp.cnt_send = (count && z_counts_itself(h)) ? h->d_cnt_send : nullptr;
  zp.smap = h->smap;
  zp.ht_pack = reinterpret_cast<const int4 *>(h->d_ht_pack); zp.h_docs = h->d_h_docs;
  zp.wt_pack = reinterpret_cast<const int4 *>(h->d_wt_pack); zp.w_docs = h->d_w_docs; zp.warm_words = h->d_warm_words;
  zp.warm_meta = h->d_warm_meta; zp.warm_tiers = h->warm_tiers; zp.warm_rows = pl.warm_cap;
  zp.phiT32 = h->d_phiT32; zp.Kp32 = pl.Kp32; zp.replays = h->d_replays; zp.margin_scale32 = h->margin_scale32;
  void *args[] = {&zp};
  if (!pl.sliced()) {
    // a range of the chunk table (the one-document chunks are in document order); persistent single-wave workgroups stride it
    if (c1 < 0) c1 = h->C;
    if (c1 <= c0) return GGS_OK;
    zp.chunk_start += c0; zp.chunk_doc += c0; zp.chunk_len += c0; zp.num_chunks = c1 - c0;
    if (zp.chunk_doc1) zp.chunk_doc1 += c0;
    KernelLaunch z = pl.z;
    z.per_cu = h->cfg->z_per_cu;
    HIP_TRY(h, launch(h, z, zp.num_chunks, args, h->stream));
    return GGS_OK;
  }
  // one 4-wave workgroup per CU (a wave per SIMD), persistent; the hot-word table fills the LDS the rings leave
  zp.num_chunks = h->Cs;
  const int hot_rows_lds = h->num_hot * pl.hot_pitch;
  // the warm tiers (z_warm_kernel): behind the hot chunks on their stream, or behind the one kernel of the fused form
  ZParams wp = zp;
  wp.wave_lds = pl.warm_wave_lds; wp.hot_off = kSlicedWaves * pl.warm_wave_lds;
  void *wargs[] = {&wp};
  auto launch_warm = [&](hipStream_t st) { return h->Cw == 0 ? hipSuccess : launch(h, pl.warm, h->warm_chunks_max, wargs, st, h->warm_rows_max * pl.hot_pitch); };
  if (h->z_split && !force_fused && h->Cs > h->Cc && h->Cc > 0) {
    // cold chunks on the main stream, hot chunks beside them (z_hot_kernel): two waves per SIMD
    ZParams hp = zp;
    hp.wave_lds = pl.hot_wave_lds; hp.hot_off = kSlicedWaves * pl.hot_wave_lds;
    void *hargs[] = {&hp};
    if (h->hot_fork_from) {
      HIP_TRY(h, hipStreamWaitEvent(h->side_hot, h->hot_fork_from, 0));
    } else {
      HIP_TRY(h, hipEventRecord(h->ev_hot_fork, h->stream));
      HIP_TRY(h, hipStreamWaitEvent(h->side_hot, h->ev_hot_fork, 0));
    }
    zp.num_chunks = h->Cc; zp.num_hot = 0;
    HIP_TRY(h, launch(h, pl.cold, h->Cc, args, h->stream));
    if (pl.hot_pairs && h->Cp > 0) {                     // the same tokens as pair-chunks (z_pairs_kernel): the same z
      hp.wave_lds = pl.pairs_wave_lds; hp.hot_off = kSlicedWaves * pl.pairs_wave_lds;
      hp.hp_pair = h->d_hp_pair; hp.hp_docs = h->d_hp_docs; hp.hp_tok = reinterpret_cast<const int4 *>(h->d_hp_tok); hp.num_pair_chunks = h->Cp;
      HIP_TRY(h, launch(h, pl.pairs, h->Cp, hargs, h->side_hot, hot_rows_lds));
    } else {
      HIP_TRY(h, launch(h, pl.hot, h->Cs - h->Cc, hargs, h->side_hot, hot_rows_lds));
    }
    HIP_TRY(h, launch_warm(h->side_hot));
    if (defer_join && zp.cnt_send) {
      hipStream_t main_stream = h->stream;
      h->stream = h->side_hot;
      const int rc = launch_count_hot(h);
      h->stream = main_stream;
      if (rc) return rc;
      h->hot_counted = true;
    }
    HIP_TRY(h, hipEventRecord(h->ev_hot_join, h->side_hot));
    if (defer_join) h->hot_join_pending = true;
    else HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_hot_join, 0));
  } else {
    HIP_TRY(h, launch(h, pl.cold, std::max(h->Cc, h->Cs - h->Cc), args, h->stream, hot_rows_lds));
    HIP_TRY(h, launch_warm(h->stream));
  }
  if (pl.f32) ++h->z_f32_launches;
  return GGS_OK;
}

bool sample_phi_this_iteration(const ggs_handle *h) {  // UPLDA:1350-1352
  return h->phi_burn_in > 0 && h->iteration > h->phi_burn_in && (h->iteration % h->phi_thin) == 0;
}

// java.util.Random(seed).nextInt(bound), n times (JDK 8 javadoc algorithm: 48-bit LCG,
// next(31), power-of-two shortcut, modulo rejection loop otherwise).
uint64_t java_lcg_next_ints(int32_t seed, int32_t bound, int64_t n, int32_t *out) {   // returns the generator's state after the n draws
  constexpr uint64_t kMult = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
  uint64_t s = ((uint64_t)(int64_t)seed ^ kMult) & kMask;
  auto next31 = [&]() { s = (s * kMult + 0xBULL) & kMask; return (int32_t)(s >> 17); };
  const int32_t m = bound - 1;
  for (int64_t i = 0; i < n; ++i) {
    int32_t r = next31();
    if ((bound & m) == 0) r = (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
    else
      for (int32_t u = r;; u = next31()) {
        r = u % bound;
        if ((int32_t)((uint32_t)u - (uint32_t)r + (uint32_t)m) >= 0) break;
      }
    out[i] = r;
  }
  return s;
}

// The side-stream theta must not outlive the z it was drawn from.
int drop_theta_ahead(ggs_handle *h) {
  if (h->side) HIP_TRY(h, hipStreamSynchronize(h->side));
  h->theta_ahead_iter = INT64_MIN;
  return GGS_OK;
}

// waits for every enqueued sweep and adds its phase times to the timings
int settle_sweeps(ggs_handle *h) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int j = h->ev_pending - 1; j >= 0; --j) {
    const Events &E = ev_slot(h, j);
    float ms = 0;
    // a consumed ahead-draw: the stream waited on th1 before the z kernel, so both side-stream events are complete;
    // their span is the duration of a kernel that ran beside the previous sweep's Phi phase
    // (every event or barrier packet on the critical stream costs ~6 us of device time: a theta drawn on it starts at the
    // previous sweep's e[2])
    if (E.used_ahead && E.theta_on_main) { HIP_TRY(h, hipEventElapsedTime(&ms, ev_slot(h, j + 1).e[2], E.th1)); }
    else if (E.used_ahead) { HIP_TRY(h, hipEventElapsedTime(&ms, E.th0, E.th1)); }
    else { HIP_TRY(h, hipEventElapsedTime(&ms, E.e[0], E.e[1])); }
    h->tm.theta_ms += ms;
    HIP_TRY(h, hipEventElapsedTime(&ms, E.e[1], E.e[2])); h->tm.z_ms += ms;
    if (E.light) {                                       // the ends only: the phases in the last fully timed sweep's proportions
      HIP_TRY(h, hipEventElapsedTime(&ms, E.e[2], E.e[5]));
      h->tm.merge_ms += ms * h->frac[0];
      h->tm.exchange_rs_ms += ms * h->frac[1]; h->tm.exchange_ag_ms += ms * h->frac[3]; h->tm.exchange_ms += ms * (h->frac[1] + h->frac[3]);
      h->tm.phi_ms += ms * (h->frac[2] + h->frac[4]);
      h->tm.sweeps += 1;
      h->tm.tokens_sampled += h->N;
      continue;
    }
    HIP_TRY(h, hipEventElapsedTime(&ms, E.e[2], E.e[3])); h->tm.merge_ms += ms;
    if (E.exchanged) {
      float span = 0, part[5] = {ms, 0, 0, 0, 0};
      // reduce-scatter | slice draw (the first half's all-gather beneath it) | what is left of the all-gathers | repack
      HIP_TRY(h, hipEventElapsedTime(&part[1], E.e[E.e4_is_e3 ? 3 : 4], E.x[0])); HIP_TRY(h, hipEventElapsedTime(&part[2], E.x[0], E.x[1]));
      HIP_TRY(h, hipEventElapsedTime(&part[3], E.x[1], E.x[2])); HIP_TRY(h, hipEventElapsedTime(&part[4], E.x[2], E.e[5]));
      HIP_TRY(h, hipEventElapsedTime(&span, E.e[2], E.e[5]));
      if (span > 0) {
        // what lies between e[3] and e[4] in a split sweep (the caller's own work) is nobody's phase: renormalise
        const float sum = part[0] + part[1] + part[2] + part[3] + part[4];
        for (int q = 0; q < 5; ++q) h->frac[q] = sum > 0 ? part[q] / sum : 0.0;
        h->have_frac = true;
      }
      h->tm.exchange_ms += part[1]; h->tm.exchange_rs_ms += part[1]; h->tm.phi_ms += part[2];
      h->tm.exchange_ms += part[3]; h->tm.exchange_ag_ms += part[3]; h->tm.phi_ms += part[4];
    } else {
      HIP_TRY(h, hipEventElapsedTime(&ms, E.e[E.e4_is_e3 ? 3 : 4], E.e[5])); h->tm.phi_ms += ms;
    }
    h->tm.sweeps += 1;
    h->tm.tokens_sampled += h->N;
  }
  h->ev_pending = 0;
  return GGS_OK;
}

// the handle's launches go to another stream for a scope (the count rebuild and the Phi chain of a whole sweep)
struct StreamSwap {
  ggs_handle *h;
  hipStream_t user;
  StreamSwap(ggs_handle *h_, hipStream_t s) : h(h_), user(h_->stream) { h->stream = s; }
  ~StreamSwap() { h->stream = user; }
};

int z_phase(ggs_handle *h) {
  int rc;
  if (h->ev_pending >= kEvRing - 2 && (rc = settle_sweeps(h))) return rc;   // keep this slot and the next one free
  h->ev_head = (h->ev_head + 1) % kEvRing;
  Events &E = h->evs[h->ev_head];
  E.light = h->xg && h->have_frac && h->detail_every > 1 && !h->force_detail && (h->sweeps_enqueued % h->detail_every) != 0 && !count_form(h->scheme);
  h->sweeps_enqueued += 1;
  if (pcgs_family(h->scheme)) {                         // no theta: it is integrated out (UPLDA:1509-1513)
    E.used_ahead = false;
    HIP_TRY(h, hipEventRecord(E.e[0], h->stream));
    HIP_TRY(h, hipEventRecord(E.e[1], h->stream));
    if ((rc = launch_pcgs_z(h))) return rc;
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));
    if ((rc = launch_count_rebuild(h))) return rc;
    if (!E.light) HIP_TRY(h, hipEventRecord(E.e[3], h->stream));
    return GGS_OK;
  }
  E.used_ahead = h->theta_ahead_iter == (int64_t)h->iteration;
  h->hot_fork_from = nullptr;
  if (E.used_ahead) {
    if (E.theta_on_main) h->hot_fork_from = E.th1;          // drawn on this very stream: nothing to wait for, and the hot kernel's stream (which ran the Phi chain) forks from th1
    else HIP_TRY(h, hipStreamWaitEvent(h->stream, E.th1, 0));   // drawn during the previous iteration's Phi phase
    std::swap(h->d_theta, h->d_theta_next);
  } else {
    E.theta_on_main = false;
    if (h->side) HIP_TRY(h, hipStreamSynchronize(h->side));
    HIP_TRY(h, hipEventRecord(E.e[0], h->stream));
    if ((rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  HIP_TRY(h, hipEventRecord(E.e[1], h->stream));
  if (h->plan.sliced() && h->z_split && !h->z_split_tried && h->Cs > h->Cc && h->Cc > 0) {
    // Whether the guest kernel really runs beside the cold one depends on how the runtime maps streams to hardware
    // queues (measured: beside each other in a plain process, one after the other under torchrun + RCCL).  Both forms
    // write the same z, so the first z step of a corpus simply runs twice, timed, and the slower form is dropped.
    h->z_split_tried = true;
    float t_split = 0, t_fused = 0;
    ScopedEvents<3> timer;
    const hipEvent_t t0 = timer.make(), t1 = timer.make(), t2 = timer.make();
    if (timer.n < 3) return set_err(h, GGS_ERR_HIP, "hipEventCreate");
    if ((rc = launch_z(h, false)) || (rc = launch_z(h, true))) return rc;   // untimed: code upload, cold caches
    HIP_TRY(h, hipEventRecord(t0, h->stream));
    if ((rc = launch_z(h, false))) return rc;
    HIP_TRY(h, hipEventRecord(t1, h->stream));
    if ((rc = launch_z(h, true))) return rc;
    HIP_TRY(h, hipEventRecord(t2, h->stream));
    HIP_TRY(h, hipEventSynchronize(t2));
    HIP_TRY(h, hipEventElapsedTime(&t_split, t0, t1));
    HIP_TRY(h, hipEventElapsedTime(&t_fused, t1, t2));
    if (t_fused < t_split) h->z_split = false;
    HIP_TRY(h, hipEventRecord(E.e[1], h->stream));          // this sweep's z time: one launch of the form kept
  }
  if (!h->hot_fork_from) h->hot_fork_from = E.e[1];        // the event just recorded serves as the hot chunks' fork: one packet less
  h->theta_ahead_iter = INT64_MIN;
  const bool ahead = h->overlap_theta && h->side && h->D > 0 && h->iteration < INT32_MAX;   // there is no iteration behind the last
  const int32_t P = (int32_t)h->part_doc.size() - 1;   // 1 for a small corpus
  if (ahead && P > 1 && h->plan.stream()) {
    // part by part: z of part p on the main stream, then -- beside z of part p + 1 -- theta of iteration t+1 for the
    // documents of part p on the side stream; the last part's theta runs beside the counts and the Phi draw
    Events &N = ev_slot(h, -1);
    for (int32_t p = 0; p < P; ++p) {
      if ((rc = launch_z(h, false, h->part_chunk[(size_t)p], h->part_chunk[(size_t)p + 1]))) return rc;
      HIP_TRY(h, hipEventRecord(h->ev_part[p], h->stream));
      HIP_TRY(h, hipStreamWaitEvent(h->side, h->ev_part[p], 0));
      if (p == 0) { N.theta_on_main = false; HIP_TRY(h, hipEventRecord(N.th0, h->side)); }
      if ((rc = launch_theta(h, h->side, h->d_theta_next, h->iteration + 1, h->part_doc[(size_t)p], h->part_doc[(size_t)p + 1],
                             p + 1 < P ? h->cfg->theta_lds_beside_z : 0)))
        return rc;
    }
    HIP_TRY(h, hipEventRecord(N.th1, h->side));
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));
    h->theta_ahead_iter = (int64_t)h->iteration + 1;
  } else {
    const bool counting = z_counts_itself(h) && h->Cs > 0;
    if (counting && !h->cnt_send_zeroed && (rc = clear_send_buffer(h, h->stream))) return rc;   // nobody cleared it behind the last reduce-scatter (or none came): counts no z step asked for are overwritten, as a count rebuild overwrites them
    h->hot_counted = false;
    if ((rc = launch_z(h, false, 0, -1, counting, /*defer_join=*/counting))) return rc;
    if (counting) { h->z_counted = true; h->cnt_send_zeroed = false; h->counted_sparse = false; }
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));      // the cold kernel's end; the hot chunks' stream is joined below, and by the theta draw's stream
    h->chain_on_side = h->chain_on_side && ahead;
    if (ahead) {
      // theta of iteration t+1 from the z just drawn, concurrent with the counts and the Phi draw
      Events &N = ev_slot(h, -1);
      hipStream_t ts = h->chain_on_side ? h->stream : h->side;
      HIP_TRY(h, hipStreamWaitEvent(h->chain_on_side ? h->side_hot : h->side, E.e[2], 0));
      if (h->hot_join_pending) HIP_TRY(h, hipStreamWaitEvent(ts, h->ev_hot_join, 0));   // the theta draw reads the hot chunks' z as well
      N.theta_on_main = h->chain_on_side;
      if (!h->chain_on_side) HIP_TRY(h, hipEventRecord(N.th0, ts));
      if ((rc = launch_theta(h, ts, h->d_theta_next, h->iteration + 1, 0, -1, h->chain_on_side ? h->plan.theta_lds_main : 0, h->chain_on_side ? h->plan.theta_docs_main : 0))) return rc;
      HIP_TRY(h, hipEventRecord(N.th1, ts));
      h->theta_ahead_iter = (int64_t)h->iteration + 1;
    }
  }
  {
    StreamSwap on_chain(h, h->chain_on_side ? h->side_hot : h->stream);
    if (h->hot_join_pending) { HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_hot_join, 0)); h->hot_join_pending = false; }
    if (h->z_counted) {                              // the z kernels added the cold tokens' cells: the hot words' segments are left
      h->z_counted = false;
      if (h->hot_counted) { h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false; }   // ... and were counted on the hot chunks' stream
      else if ((rc = launch_count_hot(h))) return rc;
    } else if ((rc = launch_count_rebuild(h))) return rc;   // this shard's counts; summed across shards by the caller
    if (!E.light) HIP_TRY(h, hipEventRecord(E.e[3], h->stream));
    if (h->chain_on_side && !h->whole_sweep) HIP_TRY(h, hipEventRecord(h->ev_chain_done, h->stream));
  }
  // ggs_sweep_begin on its own: what the caller does on the handle's stream before ggs_sweep_end (a getter) sees the counts
  if (h->chain_on_side && !h->whole_sweep) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_chain_done, 0));
  return GGS_OK;
}

// `settle` = wait for the device, raise what the sweeps flagged and add their phase times to the timings.  A batch
// (ggs_sweep with n_sweeps > 1) settles once, after its last sweep: the device flags are sticky, and the ~40 us host
// round trip per sweep is 2 % of a 1.9 ms sweep.
int finish_sweep_enqueue_on(ggs_handle *h, bool with_phi) {
  int rc;
  Events &E = h->evs[h->ev_head];
  E.e4_is_e3 = h->whole_sweep;                         // one event packet less on the stream (~6 us each)
  if (!E.e4_is_e3 && !E.light) HIP_TRY(h, hipEventRecord(E.e[4], h->stream));
  bool acc = false;
  E.exchanged = false;
  if (with_phi) {
    acc = (h->flags & GGS_FLAG_SAVE_PHI_MEAN) && sample_phi_this_iteration(h);
    if (count_form(h->scheme)) {   // no Phi in the count form: the merge (with an exchange: the gather of the count slices) and tokensPerTopic
      acc = false;
      if ((rc = launch_magnitude(h))) return rc;
    } else {
      E.exchanged = h->xg != nullptr;
      if ((rc = launch_phi(h, false, acc, E.light ? nullptr : &E))) return rc;
    }
  }
  HIP_TRY(h, hipEventRecord(E.e[5], h->stream));
  if (acc) h->n_sampled_phi++;             // GGS:168-170
  h->ev_pending += 1;
  return GGS_OK;
}
int finish_sweep_enqueue(ggs_handle *h, bool with_phi) {
  if (!h->chain_on_side) return finish_sweep_enqueue_on(h, with_phi);
  int rc;
  {
    StreamSwap on_chain(h, h->side_hot);
    if ((rc = finish_sweep_enqueue_on(h, with_phi))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_chain_done, h->stream));
  }
  HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_chain_done, 0));   // behind the theta draw: the next z step, a getter, a synchronise see both legs
  return GGS_OK;
}
int finish_sweep_settle(ggs_handle *h) {
  int rc;
  if ((rc = check_status(h))) return rc;   // synchronises the stream
  if ((rc = settle_sweeps(h))) return rc;
  if (h->flags & GGS_FLAG_PARANOID) return ggs_check_invariants(h);
  return GGS_OK;
}
int finish_sweep(ggs_handle *h, bool with_phi, bool settle = true) {
  int rc = finish_sweep_enqueue(h, with_phi);
  if (rc) return rc;
  if (!settle && !(h->flags & GGS_FLAG_PARANOID)) return GGS_OK;
  return finish_sweep_settle(h);
}

// iterations are 0 ... INT32_MAX: a call whose steps would count past the end is refused as a whole, before anything is launched
int iteration_room(ggs_handle *h, int32_t steps) {
  if (steps > 0 && (int64_t)h->iteration + (int64_t)steps > (int64_t)INT32_MAX)
    return set_err(h, GGS_ERR_STATE, "the iteration number would pass INT32_MAX");
  return GGS_OK;
}
}  // namespace
