// ggs_api.hip -- the C-ABI of libggs_hip.so (include/ggs_hip.h): the extern "C" entry points and nothing else.  The host side behind
// them is in the ggs_host_*.hpp headers, by concern; this file is the one translation unit that includes them.
//
// Build (see Makefile): hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared
#include "ggs_host_state.hpp"
#include "ggs_host_plan.hpp"
#include "ggs_host_counts.hpp"
#include "ggs_host_phi.hpp"
#include "ggs_host_sweep.hpp"
#include "ggs_host_exchange.hpp"
#include "ggs_host_end_of_run.hpp"
#include "ggs_host_hyper.hpp"
#include "ggs_host_debug.hpp"
#include "ggs_host_similarity.hpp"

extern "C" {

int ggs_abi_version(void) { return GGS_ABI_VERSION; }

const char *ggs_last_error(const ggs_handle *h) { return h ? h->err.c_str() : "null handle"; }

int ggs_create(const ggs_config *cfg, ggs_handle **out) {
  if (!cfg || !out) return GGS_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(ggs_config)) return GGS_ERR_BAD_ARG;
  if (cfg->num_topics <= 0 || cfg->num_types <= 0 || !(cfg->beta > 0)) return GGS_ERR_BAD_ARG;
  Scheme scheme = Scheme::ggs; int32_t poisson_L = 0;
  if (const int rc = scheme_of(cfg, scheme, poisson_L)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device_id < 0 || cfg->device_id >= ndev) return GGS_ERR_HIP;
  ggs_handle *h = new (std::nothrow) ggs_handle();
  if (!h) return GGS_ERR_HIP;
  const Knobs kn;                                      // every GGS_DEBUG_* variable this call reads
  // 1. the model
  h->K = cfg->num_topics; h->V = cfg->num_types; h->device = cfg->device_id;
  h->Ks = h->Ksm = h->K; h->k0 = 0;
  h->Kp = (h->K + 1) & ~1;
  h->pitch16 = (h->Kp / 2) | 1;             // odd number of 16-byte units per LDS row
  h->beta = cfg->beta; h->beta_sum = cfg->beta * (double)cfg->num_types; h->seed = cfg->seed; h->flags = cfg->flags;
  h->scheme = scheme; h->pa_L = poisson_L;
  h->phi_burn_in = cfg->phi_burn_in; h->phi_thin = cfg->phi_mean_thin > 0 ? cfg->phi_mean_thin : 1;
  h->alpha.assign(h->K, cfg->alpha_scalar);
  if (cfg->alpha) std::copy(cfg->alpha, cfg->alpha + h->K, h->alpha.begin());
  for (double a : h->alpha)
    if (!(a > 0)) { delete h; return GGS_ERR_BAD_ARG; }
  for (double a : h->alpha) h->alpha_sum = h->alpha_sum + a;
  h->alpha_symmetric = std::all_of(h->alpha.begin(), h->alpha.end(), [&](double a) { return std::memcmp(&a, &h->alpha[0], sizeof a) == 0; });
  // 2. the handle's own switches
  // GGS_DEBUG_MARGIN: above 1 the margins force the exact replays in tests.  Below 1 voids the proof, so only the float32 cold
  // kernel takes it (its decided draw is a count of partial sums, always a topic < K); the checkpoint-and-refine walks of the
  // fp64 margin kernels keep >= 1, where a wrong slice could walk them out of it
  if (kn.margin.set) { h->margin_scale = std::max(1.0, kn.margin.f); h->margin_scale32 = std::max(0.0, kn.margin.f); }
  if (kn.chain.set) h->exact_sum = kn.chain.v == 0;
  if (kn.guided.set) h->sum_guided = kn.guided.v != 0;
  if (kn.no_overlap.set) h->overlap_theta = kn.no_overlap.v == 0;
  if (kn.theta_main.set) { h->theta_main = kn.theta_main.v != 0; h->theta_main_always = kn.theta_main.v == 2; }
  if (kn.gamma_queue.set) h->gamma_queue_cap = std::max(0, kn.gamma_queue.v);
  h->sum_nseg = (h->V + kSumSegRows - 1) / kSumSegRows;

  int rc = GGS_OK;
  auto bail = [&](int code) { ggs_destroy(h); return code; };
  // 3. the device and the launches this handle can make on it
  if (hipSetDevice(h->device) != hipSuccess) return bail(GGS_ERR_HIP);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return bail(GGS_ERR_HIP);
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // GGS_DEBUG_NUM_CUS: a smaller count for every persistent grid and list sized by it (it can only lower the count, and a
    // smaller grid is always resident; no kernel waits on another workgroup).  Results do not depend on it: the tests give
    // one CU many items per workgroup, which the real chip gets only from a large corpus
    if (kn.num_cus.set) h->num_cus = std::max(1, std::min(h->num_cus, kn.num_cus.v));
  }
  if ((rc = plan_launches(h->K, h->V, h->scheme, kn, h->plan))) return bail(rc);
  h->cfg = &h->plan.cfg_parts;
  h->z_split = h->plan.split;
  if (pcgs_family(h->scheme)) h->pcgs_z = pcgs_entry(h->plan, h->scheme, h->plan.wave_forced);
  // The attribute is process-global per kernel, not per handle: always the hardware maximum, so that a later handle
  // with a smaller K never lowers the cap under a live one.
  for (const KernelLaunch *l : h->plan.all())
    if (l->fn && hipFuncSetAttribute(l->fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return bail(GGS_ERR_HIP);
  // the document kernels of the two diagnostics: four K-long histograms per block pass 64 KiB from K = 4095
  for (const void *f : {reinterpret_cast<const void *>(ll_docs_kernel), reinterpret_cast<const void *>(lp_docs_kernel)})
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return bail(GGS_ERR_HIP);
  // 4. the model's buffers
  // (a lightcollapsed or adlda handle has no Phi: ggs_get_phi allocates the buffer of its point estimate when it is first asked for one)
  const bool with_phi = !counts_only(h->scheme);
  const size_t kv = (size_t)h->K * h->V, phi_elems = (size_t)h->V * h->Kp + kPhiTailPadBytes / 8;
  if ((rc = upload(h, &h->d_alpha, h->alpha)) || (with_phi && (rc = dev_alloc_zeroed(h, &h->d_phiT, phi_elems))) ||
      (rc = dev_alloc(h, &h->d_mag, h->K)) || (rc = dev_alloc(h, &h->d_tot, h->K)) || (rc = dev_alloc_zeroed(h, &h->d_n_wk, kv)) ||
      (rc = dev_alloc_zeroed(h, &h->d_n_k, h->K)) || (rc = dev_alloc_zeroed(h, &h->d_status, 4)))
    return bail(rc);
  if ((h->flags & GGS_FLAG_SAVE_PHI_MEAN) && (rc = dev_alloc_zeroed(h, &h->d_phi_mean, kv))) return bail(rc);
  if (h->plan.sliced() && h->plan.f32) {
    if ((rc = dev_alloc_zeroed(h, &h->d_phiT32, (size_t)h->V * h->plan.Kp32 + kPhiTailPadBytes / 4))) return bail(rc);
    if (kn.replays.is(1) && (rc = dev_alloc_zeroed(h, &h->d_replays, 1))) return bail(rc);
  }
  if (h->exact_sum && ((rc = dev_alloc(h, &h->d_sum_pref, ((size_t)h->sum_nseg + 1) * h->K)) ||
                       (rc = dev_alloc(h, &h->d_sum_fn, (size_t)h->sum_nseg * h->K * 4))))
    return bail(rc);
  // tables, lists and counters start zeroed: no entry is ever read that the build (adlda: the head) did not write
  if (has_tables(h->scheme) && ((rc = dev_alloc_zeroed(h, &h->d_alias_ps, kv)) || (rc = dev_alloc_zeroed(h, &h->d_alias_a, kv)) || (rc = dev_alloc_zeroed(h, &h->d_alias_tn, (size_t)h->V)))) return bail(rc);
  if (has_mh(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_mh, 3))) return bail(rc);
  if (has_word_lists(h->scheme) && ((rc = dev_alloc_zeroed(h, &h->d_nzw, kv)) || (rc = dev_alloc_zeroed(h, &h->d_nw, (size_t)h->V)))) return bail(rc);
  if (has_sparse_stats(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_ps_stats, 4))) return bail(rc);
  if (h->scheme == Scheme::nzvsspalias) {              // the chain's rows, the mask, its outputs
    h->vs_W = (h->V + 31) / 32; h->vs_pitch = (h->K + 31) / 32;
    h->vs_global = h->plan.vschain.lds == 0;
    const size_t kw = (size_t)h->K * h->vs_W, vm = (size_t)h->V * h->vs_pitch;
    if ((rc = dev_alloc(h, &h->d_vs_cz, kw)) || (rc = dev_alloc(h, &h->d_vs_pz, kw)) || (rc = dev_alloc_zeroed(h, &h->d_vs_und, kw)) ||
        (rc = dev_alloc_zeroed(h, &h->d_vs_mask, vm)) || (rc = dev_alloc(h, &h->d_vs_s_end, (size_t)h->K)) || (rc = dev_alloc_zeroed(h, &h->d_vs_rounds, (size_t)h->K)) ||
        (rc = dev_alloc(h, &h->d_vs_zero, 1)) || (h->vs_global && (rc = dev_alloc(h, &h->d_vs_work, 2 * kw))))
      return bail(rc);
  }
  if (poisson_phi(h->scheme)) {
    std::vector<double> T;
    build_poisson_table(h->beta, h->pa_L, T);
    h->pa_t00 = T[0];
    if ((rc = upload(h, &h->d_pa_table, T)) || (rc = dev_alloc(h, &h->d_pa_acc, (size_t)h->K * kPoissonAccStride))) return bail(rc);
  }
  if (count_tables(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_tpt, (size_t)h->V))) return bail(rc);
  if (h->scheme == Scheme::adlda && ((rc = dev_alloc_zeroed(h, &h->d_ad_den0, (size_t)h->K)) || (rc = dev_alloc_zeroed(h, &h->d_ad_s0, 1)))) return bail(rc);
  if (h->scheme == Scheme::collapsed && (rc = dev_alloc(h, &h->d_lcg, 2))) return bail(rc);
  // 5. events and streams
  for (auto &e : h->ev_part)
    if (make_event(h, &e, hipEventDisableTiming)) return bail(GGS_ERR_HIP);
  for (auto &E : h->evs)
    for (hipEvent_t *e : {&E.e[0], &E.e[1], &E.e[2], &E.e[3], &E.e[4], &E.e[5], &E.x[0], &E.x[1], &E.x[2], &E.th0, &E.th1})
      if (make_event(h, e)) return bail(GGS_ERR_HIP);
  {
    // lowest priority: the theta draw fills whatever the Phi phase (on the caller's stream) leaves idle
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    // (a CU-masked side stream was tried: hipExtStreamCreateWithCUMask gives a blocking stream that
    // serialises with the legacy default stream, so the overlap is lost -- priority alone it is)
    if (make_stream(h, &h->side, lo) || make_stream(h, &h->side_hot, hi) || make_event(h, &h->ev_hot_fork) || make_event(h, &h->ev_hot_join) ||
        make_event(h, &h->ev_chain_done, hipEventDisableTiming))
      return bail(GGS_ERR_HIP);
  }
  if (hipDeviceSynchronize() != hipSuccess) return bail(GGS_ERR_HIP);   // the memsets above ran on the null stream
  *out = h;
  return GGS_OK;
}

void ggs_destroy(ggs_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  if (h->d_replays) {                                  // GGS_DEBUG_REPLAYS: the undecided tokens of the float32 cold path, measured
    unsigned long long n = 0;
    if (hipMemcpy(&n, h->d_replays, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "[ggs] z replays: %llu tokens in %lld launches of z_sliced32_kernel (%.2f per launch)\n", n, (long long)h->z_f32_launches,
              h->z_f32_launches ? (double)n / (double)h->z_f32_launches : 0.0);
  }
  for (void **slot : h->owned)
    if (*slot) (void)hipFree(*slot);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  if (h->d_heldout_spill) (void)hipFree(h->d_heldout_spill);
  exchange_free(h->xg);                                // before its streams
  for (hipStream_t st : h->owned_streams) (void)hipStreamDestroy(st);
  for (hipEvent_t ev : h->owned_events) (void)hipEventDestroy(ev);
  delete h;
}

int ggs_set_stream(ggs_handle *h, void *hip_stream) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = drop_theta_ahead(h))) return rc;
  if (h->xg && !hip_stream) return set_err(h, GGS_ERR_BAD_ARG, "with an exchange attached the handle does not run on the legacy default stream");
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return GGS_OK;
}

int ggs_set_corpus(ggs_handle *h, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, int64_t doc_base, int64_t tok_base) {
  // 1. validate, before the handle is touched
  if (!h || D < 0 || !doc_ptr || doc_base < 0 || tok_base < 0) return set_err(h, GGS_ERR_BAD_ARG, "bad corpus arguments");
  if (doc_ptr[0] != 0) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr[0] must be 0");
  for (int64_t d = 0; d < D; ++d)
    if (doc_ptr[d + 1] < doc_ptr[d]) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr must be non-decreasing");
  const int64_t N = doc_ptr[D];
  if (N > 0 && !tokens) return set_err(h, GGS_ERR_BAD_ARG, "tokens is null");
  if (N >= (int64_t)1 << 31 || D >= (int64_t)1 << 31) return set_err(h, GGS_ERR_UNSUPPORTED, "more than 2^31-1 tokens or documents per device");
  for (int64_t i = 0; i < N; ++i)
    if (tokens[i] < 0 || tokens[i] >= h->V) return set_err(h, GGS_ERR_BAD_ARG, "token id outside [0, num_types)");
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = drop_theta_ahead(h))) return rc;

  // 2. what this corpus chooses between the plan's entries.  The parts of the z step pay where the theta draw (D x K
  // gammas) is longer than the Phi chain it otherwise hides beside (V x K gammas): the excess is what is drawn beside
  // the z parts.  Measured: D = 100 000, V = 50 000, K = 1 024: 1 part 18.4 ms per sweep, 2: 18.1, 4: 16.5, 8: 15.9;
  // D = 18 846, V = 60 000, K = 200: 8 parts 1.112, 4: 1.071, 2: 1.019, 1: 1.006 (every part costs an event packet, a launch
  // and the drain of the persistent z waves).
  const LaunchPlan &pl = h->plan;
  int32_t parts = pl.cfg_parts.parts;
  if (!pl.parts_forced && parts > 1) parts = D <= (int64_t)h->V ? 1 : D < 2 * (int64_t)h->V ? std::min(parts, 4) : parts;
  h->cfg = parts > 1 ? &pl.cfg_parts : &pl.cfg_plain;

  // 3. the lists, on the host (ggs_corpus_lists.hpp): the count rebuild's, and those of the z step the plan launches
  const bool pcgs = pcgs_family(h->scheme);
  CorpusShape shape;
  shape.V = h->V; shape.tile_tokens = pl.tile_tokens; shape.z_parts = parts;
  shape.pcgs = pcgs; shape.sliced = pl.sliced(); shape.two_rows = pl.two_rows;
  shape.hot_cap = pl.hot_cap; shape.warm_cap = pl.warm_cap; shape.warm_docs = pl.warm_docs;
  shape.warm_tiers_max = pl.warm_tiers_max; shape.warm_min_fill_pct = pl.warm_min_fill_pct; shape.warm_min_chunks_per_wave = pl.warm_min_chunks_per_wave;
  shape.hot_pairs = pl.hot_pairs;
  shape.sliced_waves = (int64_t)h->num_cus * kSlicedWaves; shape.pcgs_waves = (int64_t)h->num_cus * pl.lane.per_cu;
  const CorpusLists L = build_corpus_lists(shape, D, doc_ptr, tokens);
  if (pcgs) {
    // the lane-per-document kernels keep the counts as int16: a longer document sends the corpus to the wave-per-document kernel
    h->pcgs_wave = pl.wave_forced || L.longest > kPcgsMaxDocLen;
    if (h->pcgs_wave && !pl.wave.fn) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=pcgs: a document of 32768 tokens or more with more than 4096 topics");
    h->pcgs_z = pcgs_entry(pl, h->scheme, h->pcgs_wave);
    h->pcgs_items = (wave_only(h->scheme) || h->pcgs_wave) ? (int64_t)L.order.size() : ((int64_t)L.order.size() + 63) / 64;   // a wave or a lane per entry
    if (const auto corpus_lds = row_of(h->scheme).corpus_lds) {
      // the list of a document's non-zero topics holds at most min(K, its length) entries (adlda: beside den0, alpha and a block of
      // terms); the resident waves by LDS and, but for spalias, by the kernel's registers.  (The doubly sparse walks took
      // min(lds_workgroups_per_cu(lds, 32), by_regs): with Q = what LDS allows and by_regs >= 1, min(max(1, min(32, Q)), by_regs) =
      // max(1, min(by_regs, 32, Q)) whether min(32, Q) is 0 or not, which is resident_waves_per_cu.)
      h->sp_cap = (int32_t)std::max<int64_t>(1, std::min<int64_t>(h->K, L.longest));
      h->pcgs_z.lds = (int)corpus_lds(h->K, h->sp_cap);
      h->pcgs_z.per_cu = h->scheme == Scheme::spalias ? lds_workgroups_per_cu(h->pcgs_z.lds, 32) : resident_waves_per_cu(h->pcgs_z.fn, h->pcgs_z.lds);
      if (const char *e = debug_env("GGS_DEBUG_SPALIAS_WPC")) h->pcgs_z.per_cu = std::max(1, std::min(h->pcgs_z.per_cu, std::atoi(e)));
    }
  }
  h->D = D; h->N = N; h->C = (int64_t)L.cstart.size(); h->S = (int64_t)L.seg_word.size(); h->doc_base = doc_base; h->tok_base = tok_base;
  h->part_doc = L.part_doc; h->part_chunk = L.part_chunk;
  h->pcgs_order_len = (int64_t)L.order.size();
  h->num_hot = (int32_t)L.hot_words.size(); h->HS = (int64_t)L.hseg_word.size();
  h->Cc = L.Cc; h->Cs = L.Cs; h->Cp = L.Cp; h->hp_pairs = h->hp_tokens = 0;
  for (int64_t c = 0; c < L.Cp; ++c) { h->hp_pairs += L.hp_docs[(size_t)(c * kWarmDocSlots + kHotPairCountSlot)]; h->hp_tokens += L.hp_docs[(size_t)(c * kWarmDocSlots + kHotPairTokSlot)]; }
  h->warm_tiers = L.warm_tiers; h->num_warm = L.num_warm; h->Cw = L.Cw; h->warm_chunks_max = L.warm_chunks_max; h->warm_rows_max = L.warm_rows_max;

  // 4. upload (on the null stream), the state of the corpus zeroed
  const size_t theta_elems = (size_t)D * h->K + 2;
  if ((rc = upload(h, &h->d_doc_ptr, doc_ptr, (size_t)D + 1)) || (rc = upload(h, &h->d_tok, tokens, (size_t)N)) ||
      (rc = upload(h, &h->d_perm, L.perm)) || (rc = upload(h, &h->d_inv_perm, L.inv)) ||
      (rc = upload(h, &h->d_seg_word, L.seg_word)) || (rc = upload(h, &h->d_seg_begin, L.seg_begin)))
    return rc;
  if (pcgs && (rc = upload(h, &h->d_order, L.order))) return rc;
  if (pl.sliced() && ((rc = upload(h, &h->d_ct_tok, L.ct_tok)) || (rc = upload(h, &h->d_ct_idx, L.ct_idx)) || (rc = upload(h, &h->d_ct_ip, L.ct_ip)) ||
                      (rc = upload(h, &h->d_c_docs, L.c_docs)) || (rc = upload(h, &h->d_hot_words, L.hot_words)) ||
                      (rc = upload(h, &h->d_ht_pack, L.ht_pack)) || (rc = upload(h, &h->d_h_docs, L.h_docs)) ||
                      (rc = upload(h, &h->d_hseg_word, L.hseg_word)) || (rc = upload(h, &h->d_hseg_begin, L.hseg_begin)) || (rc = upload(h, &h->d_hseg_end, L.hseg_end))))
    return rc;
  if (h->C && ((rc = upload(h, &h->d_chunk_start, L.cstart)) || (rc = upload(h, &h->d_chunk_doc, L.cdoc)) || (rc = upload(h, &h->d_chunk_len, L.clen)) ||
               (pl.two_rows && (rc = upload(h, &h->d_chunk_doc1, L.cdoc1)))))
    return rc;
  if (L.Cp > 0 && ((rc = upload(h, &h->d_hp_pair, L.hp_pair)) || (rc = upload(h, &h->d_hp_docs, L.hp_docs)) || (rc = upload(h, &h->d_hp_tok, L.hp_tok)))) return rc;
  if (L.warm_tiers > 0 && ((rc = upload(h, &h->d_wt_pack, L.wt_pack)) || (rc = upload(h, &h->d_w_docs, L.w_docs)) ||
                           (rc = upload(h, &h->d_warm_words, L.warm_words)) || (rc = upload(h, &h->d_warm_meta, L.warm_meta))))
    return rc;
  const bool with_theta = !counts_only(h->scheme) && !no_theta(h->scheme);   // no theta in its chain and none for a diagnostic (ggs_log_posterior is unsupported); lightpcldaw2: ensure_diag_theta
  if (!with_theta && h->d_theta) { (void)hipFree(h->d_theta); h->d_theta = nullptr; }   // an earlier corpus' diagnostic theta
  if ((rc = dev_alloc(h, &h->d_z, (size_t)N)) || (rc = dev_alloc(h, &h->d_zw, (size_t)N)) ||
      (with_theta && (rc = dev_alloc(h, &h->d_theta, theta_elems))) || (!pcgs && (rc = dev_alloc(h, &h->d_theta_next, theta_elems))))   // theta_next: what the ggs z phase swaps in
    return rc;
  HIP_TRY(h, hipMemset(h->d_z, 0, sizeof(int32_t) * std::max<size_t>((size_t)N, 1)));
  HIP_TRY(h, hipMemset(h->d_zw, 0, sizeof(int32_t) * std::max<size_t>((size_t)N, 1)));
  if (with_theta) HIP_TRY(h, hipMemset(h->d_theta, 0, sizeof(double) * std::max<size_t>((size_t)D * h->K, 1)));
  if (!pcgs) HIP_TRY(h, hipMemset(h->d_theta_next, 0, sizeof(double) * std::max<size_t>((size_t)D * h->K, 1)));
  if (h->d_mh) HIP_TRY(h, hipMemset(h->d_mh, 0, 3 * sizeof(unsigned long long)));
  if (h->d_ps_stats) HIP_TRY(h, hipMemset(h->d_ps_stats, 0, 4 * sizeof(unsigned long long)));
  // the phi mean is the mean over ONE corpus' chain, like the counters above: a sum that ran on into the next corpus' Phi would be neither's
  if (h->d_phi_mean) HIP_TRY(h, hipMemset(h->d_phi_mean, 0, sizeof(double) * (size_t)h->K * h->V));
  h->n_sampled_phi = 0;
  HIP_TRY(h, hipDeviceSynchronize());   // the uploads and memsets above ran on the null stream; the handle's stream may not synchronise with it

  // 5. a new corpus: no Phi, no sweep in progress, the z form to be timed again
  h->have_corpus = true; h->have_z = false; h->have_phi = false; h->in_sweep = false; h->global_tokens = -1; h->lcg_ready = false;
  h->z_split = pl.split; h->z_split_tried = pl.split_forced;
  h->counts_global = h->xg == nullptr; h->cnt_own_valid = false; h->n_k_valid = false;
  return GGS_OK;
}

int ggs_init_z_java_lcg(ggs_handle *h, int32_t seed) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->tok_base != 0) return set_err(h, GGS_ERR_STATE, "java-LCG init is one sequential stream: only valid with tok_base == 0");
  if ((rc = drop_theta_ahead(h))) return rc;
  // One sequential stream, so it runs on the host exactly once at start-up.
  std::vector<int32_t> z((size_t)h->N);
  const uint64_t lcg_state = java_lcg_next_ints(seed, h->K, h->N, z.data());
  if (h->scheme == Scheme::collapsed) {
    // SerialCollapsedLDA owns ONE Randoms(seed) (SerialCollapsedLDA.java:60-65): addInstances draws the initial topics
    // from it (:789) and the sampling loop goes on with the same object (MSLDA:206): the serial sweep continues this stream
    HIP_TRY(h, hipMemcpyAsync(h->d_lcg, &lcg_state, sizeof lcg_state, hipMemcpyHostToDevice, h->stream));
    h->lcg_ready = true;
  }
  if (h->N) HIP_TRY(h, hipMemcpyAsync(h->d_z, z.data(), sizeof(int32_t) * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  if ((rc = launch_permute_z(h))) return rc;
  if ((rc = launch_count_rebuild(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->have_z = true;
  return GGS_OK;
}

int ggs_set_z(ggs_handle *h, const int32_t *z, int32_t redraw_phi) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->N > 0 && !z) return set_err(h, GGS_ERR_BAD_ARG, "z is null");
  for (int64_t i = 0; i < h->N; ++i)
    if (z[i] < 0 || z[i] >= h->K) return set_err(h, GGS_ERR_BAD_ARG, "topic indicator outside [0, num_topics)");
  if ((rc = drop_theta_ahead(h))) return rc;
  h->lcg_ready = false;                                // a restored z is not the state any java.util.Random stream left: the serial chain starts a new Random(java_seed)
  if (h->N) HIP_TRY(h, hipMemcpyAsync(h->d_z, z, sizeof(int32_t) * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  if ((rc = launch_permute_z(h))) return rc;
  if ((rc = launch_count_rebuild(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->have_z = true;
  if (redraw_phi) return ggs_init_phi(h);
  return GGS_OK;
}

int ggs_init_phi(ggs_handle *h) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme)) {   // nothing to draw: corpus-wide counts and tokensPerTopic are the whole model
    if ((rc = launch_magnitude(h))) return rc;
    h->have_phi = true;
    return check_status(h);
  }
  if ((rc = launch_phi(h, true, false))) return rc;   // with an exchange: the start-up count reduce-scatter, the slice, the all-gather
  return check_status(h);
}

int ggs_set_iteration(ggs_handle *h, int32_t it) {     // a theta drawn ahead for another iteration is simply not used
  if (!h) return GGS_ERR_BAD_ARG;
  if (it < 0) return set_err(h, GGS_ERR_BAD_ARG, "the iteration number is 0 ... INT32_MAX");
  h->iteration = it;
  return GGS_OK;
}
int ggs_get_iteration(const ggs_handle *h, int32_t *it) { if (!h || !it) return GGS_ERR_BAD_ARG; *it = h->iteration; return GGS_OK; }

// see theta_main: only where the z step is one launch pair (no parts), theta is drawn at all, no collective is in the chain, and
// the theta draw (D x K gammas) is the longer leg (the Phi chain draws V x K)
bool chain_on_side_ok(const ggs_handle *h) {
  return h->theta_main && h->plan.sliced() && h->side_hot && h->ev_chain_done && !h->xg &&
         (h->D >= (int64_t)h->V || h->theta_main_always);
}

int ggs_sweep_begin(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_begin called twice without ggs_sweep_end");
  if ((rc = iteration_room(h, 1))) return rc;
  h->iteration += 1;                                   // currentIteration = iteration, UPLDA:646
  h->chain_on_side = chain_on_side_ok(h);              // kept until the sweep's end
  if ((rc = z_phase(h))) { h->chain_on_side = false; return rc; }
  h->in_sweep = true;
  return GGS_OK;
}

int ggs_sweep_end(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_end without ggs_sweep_begin");
  h->in_sweep = false;
  rc = finish_sweep(h, true);
  h->chain_on_side = false;
  return rc;
}

int ggs_sweep_end_async(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_end_async without ggs_sweep_begin");
  h->in_sweep = false;
  rc = finish_sweep(h, true, false);
  h->chain_on_side = false;
  return rc;
}

int ggs_sweep(ggs_handle *h, int32_t n_sweeps) {
  if (h && n_sweeps > 0) {                             // all n_sweeps or none
    int rc = require_ready(h, true);
    if (rc || (rc = iteration_room(h, n_sweeps))) return rc;
  }
  for (int32_t i = 0; i < n_sweeps; ++i) {
    if (h) h->whole_sweep = true;
    int rc = ggs_sweep_begin(h);
    if (!rc) {
      h->in_sweep = false;
      rc = finish_sweep(h, true, i == n_sweeps - 1);
    }
    if (h) h->chain_on_side = h->whole_sweep = false;
    if (rc) return rc;
  }
  return GGS_OK;
}

int ggs_collapsed_serial_sweep(ggs_handle *h, int32_t java_seed, int32_t n_sweeps) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->scheme != Scheme::collapsed) return set_err(h, GGS_ERR_STATE, "ggs_collapsed_serial_sweep needs GGS_FLAG_COLLAPSED");
  if (h->xg || h->tok_base != 0) return set_err(h, GGS_ERR_STATE, "the serial chain runs over ONE unsharded corpus");
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  if ((size_t)h->K * 16 > (size_t)kMaxLdsBytes) return set_err(h, GGS_ERR_UNSUPPORTED, "num_topics too large for the serial kernel's LDS");
  if ((rc = iteration_room(h, n_sweeps))) return rc;
  if ((rc = launch_magnitude(h))) return rc;           // tokensPerTopic in step with the counts
  if (!h->lcg_ready) {                                 // new java.util.Random(seed): the scrambled initial state
    const uint64_t st = ((uint64_t)(int64_t)java_seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1);
    HIP_TRY(h, hipMemcpyAsync(h->d_lcg, &st, sizeof st, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->lcg_ready = true;
  }
  CollapsedSerialParams cp{};
  cp.doc_ptr = h->d_doc_ptr; cp.tok = h->d_tok; cp.inv_perm = h->d_inv_perm; cp.z = h->d_z; cp.zw = h->d_zw; cp.n_wk = h->d_n_wk; cp.n_k = h->d_n_k;
  cp.alpha = h->d_alpha; cp.lcg = h->d_lcg; cp.status = h->d_status; cp.num_docs = h->D; cp.beta = h->beta; cp.beta_sum = h->beta_sum; cp.K = h->K;
  for (int32_t i = 0; i < n_sweeps; ++i) {
    h->iteration += 1;
    hipLaunchKernelGGL(collapsed_serial_kernel, dim3(1), dim3(64), (size_t)h->K * 16, h->stream, cp);
  }
  HIP_TRY(h, hipGetLastError());
  h->have_phi = true;
  return check_status(h);
}

int ggs_sample_z_given_phi(ggs_handle *h, int32_t n_sweeps) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  if (count_form(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, scheme=lightcollapsed and scheme=adlda have no Phi to condition on");
  if ((rc = iteration_room(h, n_sweeps))) return rc;
  for (int32_t i = 0; i < n_sweeps; ++i) {
    h->iteration += 1;                                 // UPLDA:980
    h->force_detail = true;
    rc = z_phase(h);
    h->force_detail = false;
    if (rc) return rc;
    if ((rc = finish_sweep(h, false))) return rc;
  }
  // tokensPerTopic follows the rebuilt counts (with an exchange: the counts are merged here, UPLDA:993)
  if ((rc = launch_magnitude(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GGS_OK;
}

int ggs_counts_device_ptr(ggs_handle *h, void **dev_ptr, int64_t *num_elems) {
  if (!h || !dev_ptr || !num_elems) return GGS_ERR_BAD_ARG;
  if (h->xg) return set_err(h, GGS_ERR_STATE, "an exchange is attached: the library merges the counts itself");
  *dev_ptr = h->d_n_wk; *num_elems = (int64_t)h->K * h->V;
  h->n_k_valid = false;          // the caller may sum other shards' counts into the buffer
  return GGS_OK;
}

int ggs_set_global_token_count(ggs_handle *h, int64_t n_tokens) {
  if (!h || n_tokens < 0) return GGS_ERR_BAD_ARG;
  h->global_tokens = n_tokens;
  return GGS_OK;
}

// ---- multi-GPU: the exchange (include/ggs_hip.h) ------------------------------------------------------------------
int ggs_attach_exchange(ggs_handle *h, int32_t rank, int32_t nranks, const ggs_exchange_ops *ops) {
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  if (!ops || (ops->struct_size != (int32_t)sizeof(ggs_exchange_ops) && ops->struct_size != GGS_EXCHANGE_OPS_V3_SIZE) || !ops->reduce_scatter_i32 ||
      !ops->all_gather_f64 || !ops->all_gather_i32)
    return set_err(h, GGS_ERR_BAD_ARG, "ggs_exchange_ops: wrong struct_size or a null callback");
  auto *x = new (std::nothrow) Exchange();
  if (!x) return GGS_ERR_HIP;
  x->rank = rank; x->nranks = nranks;
  std::memcpy(&x->ops, ops, (size_t)ops->struct_size);   // a version-3 table has no all_to_all_v_i32: it stays null, the count exchange dense
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops);
  return setup_exchange(h, x);
}

int ggs_attach_null_exchange(ggs_handle *h, int32_t rank, int32_t nranks) {
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  auto *x = new (std::nothrow) Exchange();
  if (!x) return GGS_ERR_HIP;
  x->rank = rank; x->nranks = nranks; x->is_null = true;
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops); x->ops.ctx = x;
  x->ops.reduce_scatter_i32 = xops::null_reduce_scatter_i32;
  x->ops.all_gather_f64 = xops::null_all_gather<double>;
  x->ops.all_gather_i32 = xops::null_all_gather<int32_t>;
  x->ops.all_to_all_v_i32 = xops::null_all_to_all_v_i32;
  return setup_exchange(h, x);
}

int ggs_rccl_unique_id(void *out_id) {
  if (!out_id) return GGS_ERR_BAD_ARG;
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) return GGS_ERR_UNSUPPORTED;
  static_assert(sizeof(ncclUniqueId) == GGS_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return GGS_ERR_HIP;
  std::memcpy(out_id, &id, sizeof id);
  return GGS_OK;
}

int ggs_attach_rccl(ggs_handle *h, int32_t rank, int32_t nranks, const void *unique_id) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!unique_id) return set_err(h, GGS_ERR_BAD_ARG, "null unique id");
  int rc = exchange_precheck(h, rank, nranks);       // before the blocking collective below: a rejected call must not have joined it
  if (rc) return rc;
  Exchange *x = new_rccl_exchange(h, rank, nranks, &rc);
  if (!x) return rc;
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof id);
  const ncclResult_t r = x->api->CommInitRank(&x->comm, nranks, id, rank);      // collective: every rank of the job is in here
  if (r != ncclSuccess) {
    const std::string msg = std::string("ncclCommInitRank: ") + x->api->GetErrorString(r);
    delete x;
    return set_err(h, GGS_ERR_HIP, msg);
  }
  x->own_comm = true;
  return setup_exchange(h, x);
}

int ggs_attach_rccl_comm(ggs_handle *h, int32_t rank, int32_t nranks, void *nccl_comm) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!nccl_comm) return set_err(h, GGS_ERR_BAD_ARG, "null communicator");
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  Exchange *x = new_rccl_exchange(h, rank, nranks, &rc);
  if (!x) return rc;
  x->comm = static_cast<ncclComm_t>(nccl_comm);
  return setup_exchange(h, x);
}

int ggs_get_exchange_info(const ggs_handle *h, int32_t *rank, int32_t *nranks, int32_t *k_begin, int32_t *k_end) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (rank) *rank = h->xg ? h->xg->rank : 0;
  if (nranks) *nranks = h->xg ? h->xg->nranks : 1;
  if (k_begin) *k_begin = h->k0;
  if (k_end) *k_end = h->k0 + h->Ks;
  return GGS_OK;
}

int ggs_set_count_exchange(ggs_handle *h, int32_t mode) {
  if (!h || mode < 0 || mode > 2) return GGS_ERR_BAD_ARG;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  h->count_mode = mode;
  return GGS_OK;
}
int ggs_get_count_exchange(const ggs_handle *h, int32_t *sparse, int64_t *pairs_last, int64_t *cells) {
  if (!h || !sparse) return GGS_ERR_BAD_ARG;
  *sparse = use_sparse(h) ? 1 : 0;
  if (pairs_last) *pairs_last = h->sp_pairs_last;
  if (cells) *cells = h->xg ? (int64_t)h->V * h->Ksm * h->xg->nranks : (int64_t)h->V * h->K;
  return GGS_OK;
}

int ggs_get_exchange_provider(const ggs_handle *h, int32_t *provider, int32_t *comm_nranks, int32_t *comm_rank) {
  if (!h) return GGS_ERR_BAD_ARG;
  const Exchange *x = h->xg;
  if (provider) *provider = !x ? 0 : x->api ? 1 : x->is_null ? 3 : 2;
  int n = x ? x->nranks : 1, r = x ? x->rank : 0;
  if (x && x->api && x->comm) {                         // what the communicator itself reports, not what the caller passed in
    if (x->api->CommCount && x->api->CommCount(x->comm, &n) != ncclSuccess) n = -1;
    if (x->api->CommUserRank && x->api->CommUserRank(x->comm, &r) != ncclSuccess) r = -1;
  }
  if (comm_nranks) *comm_nranks = n;
  if (comm_rank) *comm_rank = r;
  return GGS_OK;
}

int ggs_group_gather_counts(ggs_handle **hs, int32_t n) {
  if (!is_group(hs, n)) return GGS_ERR_BAD_ARG;
  return group_gather_counts(hs, n);
}

int ggs_group_create(const ggs_config *cfg, int32_t n, const int32_t *device_ids, ggs_handle **out) {
  if (!cfg || n < 1 || !device_ids || !out) return GGS_ERR_BAD_ARG;
  for (int32_t i = 0; i < n; ++i) out[i] = nullptr;
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) return GGS_ERR_UNSUPPORTED;
  int rc = GGS_OK;
  for (int32_t i = 0; i < n && !rc; ++i) {
    ggs_config c = *cfg;
    c.device_id = device_ids[i];
    rc = ggs_create(&c, &out[i]);
  }
  std::vector<ncclComm_t> comms((size_t)n, nullptr);
  if (!rc && api->CommInitAll(comms.data(), n, device_ids) != ncclSuccess) rc = GGS_ERR_HIP;
  for (int32_t i = 0; i < n && !rc; ++i) {
    Exchange *x = new_rccl_exchange(out[i], i, n, &rc);
    if (!x) break;
    x->comm = comms[(size_t)i]; x->own_comm = true; comms[(size_t)i] = nullptr;
    rc = setup_exchange(out[i], x);
  }
  if (rc) {
    for (ncclComm_t c : comms) if (c) (void)api->CommDestroy(c);
    for (int32_t i = 0; i < n; ++i) { ggs_destroy(out[i]); out[i] = nullptr; }
    return rc;
  }
  out[0]->group.assign(out, out + n);
  for (int32_t i = 0; i < n; ++i) out[i]->in_group = true;
  return GGS_OK;
}

int ggs_group_adopt(ggs_handle **hs, int32_t n) {
  if (!hs || n < 1) return GGS_ERR_BAD_ARG;
  for (int32_t i = 0; i < n; ++i) {
    if (!hs[i]) return GGS_ERR_BAD_ARG;
    if (!hs[i]->xg || hs[i]->xg->api) return set_err(hs[i], GGS_ERR_STATE, "ggs_group_adopt takes handles with a caller-supplied exchange (ggs_attach_exchange)");
    if (hs[i]->xg->rank != i || hs[i]->xg->nranks != n) return set_err(hs[i], GGS_ERR_BAD_ARG, "ggs_group_adopt: handle i must be rank i of n");
  }
  hs[0]->group.assign(hs, hs + n);
  for (int32_t i = 0; i < n; ++i) hs[i]->in_group = true;
  return GGS_OK;
}

void ggs_group_destroy(ggs_handle **handles, int32_t n) {
  if (!handles) return;
  for (int32_t i = 0; i < n; ++i) { ggs_destroy(handles[i]); handles[i] = nullptr; }
}

int ggs_group_set_z(ggs_handle **hs, int32_t n, const int32_t *const *z, int32_t redraw_phi) {
  if (!is_group(hs, n) || !z) return GGS_ERR_BAD_ARG;
  int rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = ggs_set_z(hs[i], z[i], 0))) return rc;          // this shard's counts
  if (!redraw_phi) return GGS_OK;
  if (count_form(hs[0]->scheme)) {                                                 // no Phi: the merged counts and tokensPerTopic are the model
    if ((rc = group_gather_counts(hs, n))) return rc;
    for (int32_t i = 0; i < n; ++i) {
      if ((rc = bind_device(hs[i])) || (rc = launch_magnitude(hs[i]))) return rc;
      hs[i]->have_phi = true;
    }
  } else if ((rc = group_phi(hs, n, true, false))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = bind_device(hs[i])) || (rc = check_status(hs[i]))) return rc;
  return GGS_OK;
}

int ggs_group_sweep(ggs_handle **hs, int32_t n, int32_t n_sweeps) {
  if (!is_group(hs, n)) return GGS_ERR_BAD_ARG;
  int rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = iteration_room(hs[i], n_sweeps))) return rc;
  for (int32_t s = 0; s < n_sweeps; ++s) {
    if ((count_form(hs[0]->scheme) || count_tables(hs[0]->scheme)) && (rc = group_gather_counts(hs, n))) return rc;   // the z step conditions on the corpus-wide sweep-start counts
    for (int32_t i = 0; i < n; ++i) {
      ggs_handle *h = hs[i];
      if ((rc = require_ready(h, true))) return rc;
      if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
      h->iteration += 1;
      if ((rc = z_phase(h))) return rc;
    }
    if (count_form(hs[0]->scheme)) {                                               // the AD-LDA merge: gathered counts, then tokensPerTopic; no Phi
      if ((rc = group_gather_counts(hs, n))) return rc;
      for (int32_t i = 0; i < n; ++i) {
        ggs_handle *h = hs[i];
        if ((rc = bind_device(h))) return rc;
        Events &E = h->evs[h->ev_head];
        E.exchanged = false; E.e4_is_e3 = false;
        HIP_TRY(h, hipEventRecord(E.e[4], h->stream));
        if ((rc = launch_magnitude(h))) return rc;
        HIP_TRY(h, hipEventRecord(E.e[5], h->stream));
        h->ev_pending += 1;
      }
    } else if ((rc = group_phi(hs, n, false, true))) return rc;
    if (s == n_sweeps - 1 || (hs[0]->flags & GGS_FLAG_PARANOID))
      for (int32_t i = 0; i < n; ++i)
        if ((rc = bind_device(hs[i])) || (rc = check_status(hs[i])) || (rc = settle_sweeps(hs[i]))) return rc;
  }
  return GGS_OK;
}

int ggs_synchronize(ggs_handle *h) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  return check_status(h);
}

int ggs_get_z(ggs_handle *h, int32_t *z) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->N > 0 && !z) return GGS_ERR_BAD_ARG;
  return copy_out(h, z, h->d_z, sizeof(int32_t) * (size_t)h->N);
}
int ggs_get_type_topic_counts(ggs_handle *h, int32_t *n_wk) {
  if (!h || !n_wk) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  return copy_out(h, n_wk, h->d_n_wk, sizeof(int32_t) * (size_t)h->K * h->V);
}
int ggs_get_topic_totals(ggs_handle *h, int32_t *n_k) {
  if (!h || !n_k) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  // valid whatever came last: a sweep, ggs_set_z(redraw=0), an external all-reduce on ggs_counts_device_ptr
  h->n_k_valid = h->n_k_valid && h->xg != nullptr;
  if ((rc = launch_magnitude(h))) return rc;
  return copy_out(h, n_k, h->d_n_k, sizeof(int32_t) * (size_t)h->K);
}

int ggs_get_phi(ggs_handle *h, double *phi) {
  if (!h || !phi) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (count_form(h->scheme)) {   // the point estimate from the current counts
    if (!h->d_phiT && (rc = dev_alloc(h, &h->d_phiT, (size_t)h->V * h->Kp + kPhiTailPadBytes / 8))) return rc;   // lightcollapsed: only now
    if ((rc = launch_magnitude(h))) return rc;
    hipLaunchKernelGGL(psi_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_n_wk, h->d_n_k, h->beta, h->beta_sum,
                       h->d_phiT, h->K, h->Kp, h->V);
    HIP_TRY(h, hipGetLastError());
  }
  return phi_out(h, h->d_phiT, h->Kp, phi, 1.0);
}
int ggs_set_phi(ggs_handle *h, const double *phi) {
  if (!h || !phi) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (counts_only(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightcollapsed and scheme=adlda have no Phi to set");
  const size_t kv = (size_t)h->K * h->V;
  if (h->have_priors) {   // the z step leaves the prior factor out because Phi is exactly zero wherever the prior is (ggs_hip.h)
    for (int32_t v = 0; v < h->V; ++v)
      for (int32_t j = 0; j < h->pr_pitch; ++j)
        for (uint32_t bits = h->pr_mask[(size_t)v * h->pr_pitch + j]; bits; bits &= bits - 1)
          if (phi[(size_t)(j * 32 + __builtin_ctz(bits)) * h->V + v] != 0.0)
            return set_err(h, GGS_ERR_BAD_ARG, "ggs_set_phi: phi is not zero in a cell the topic priors zero");
  }
  if ((rc = ensure_scratch(h, kv * sizeof(double)))) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->d_scratch, phi, kv * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(phi_to_phiT_kernel, dim3(grid_for((int64_t)kv, 256)), dim3(256), 0, h->stream, static_cast<const double *>(h->d_scratch),
                     h->d_phiT, h->K, h->Kp, h->V, h->d_phiT32, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  // UPLDA:1897-1902: `if (savePhiMeans()) phiMean = new double[numTopics][numTypes]` -- the running sum restarts, noSampledPhi keeps counting
  if (h->d_phi_mean) HIP_TRY(h, hipMemsetAsync(h->d_phi_mean, 0, kv * sizeof(double), h->stream));
  h->alias_stale = true;
  h->vs_lists = ggs_handle::VsLists::nonzero;          // nzvsspalias: the lists of a Phi that was set are its non-zero cells (ours)
  h->vs_drawn = false;                                 // ... and no draw stands behind it: ggs_get_vs_stats reports none
  if ((rc = launch_alias_build(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->have_phi = true;
  return GGS_OK;
}

int ggs_set_topic_priors(ggs_handle *h, int64_t n_zero, const int32_t *topic, const int32_t *word) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::spalias) return set_err(h, GGS_ERR_STATE, "ggs_set_topic_priors needs GGS_FLAG_SPALIAS");
  if (h->have_phi) return set_err(h, GGS_ERR_STATE, "ggs_set_topic_priors: the handle already has a Phi");
  if (n_zero < 0 || (n_zero > 0 && (!topic || !word))) return set_err(h, GGS_ERR_BAD_ARG, "bad topic prior arguments");
  // 1. validate into a mask of its own: a refused call leaves the handle as it was
  const int32_t pitch = (h->K + 31) / 32;
  std::vector<uint32_t> mask((size_t)h->V * pitch, 0u);
  std::vector<int32_t> per_topic((size_t)h->K, 0), per_word((size_t)h->V, 0);
  for (int64_t i = 0; i < n_zero; ++i) {
    const int32_t k = topic[i], v = word[i];
    if (k < 0 || k >= h->K || v < 0 || v >= h->V) return set_err(h, GGS_ERR_BAD_ARG, "topic prior cell outside [0, num_topics) x [0, num_types)");
    uint32_t &m = mask[(size_t)v * pitch + (k >> 5)];
    if (m & (1u << (k & 31))) continue;                // duplicates are allowed
    m |= 1u << (k & 31);
    per_topic[(size_t)k] += 1; per_word[(size_t)v] += 1;
  }
  // ensureConsistentPriors, SpaliasUncollapsedParallelWithPriors.java:102-121
  for (int32_t k = 0; k < h->K; ++k)
    if (per_topic[(size_t)k] == h->V) return set_err(h, GGS_ERR_BAD_ARG, "Inconsistent prior spec, one topic has all Zero priors!");
  for (int32_t v = 0; v < h->V; ++v)
    if (per_word[(size_t)v] == h->K) return set_err(h, GGS_ERR_BAD_ARG, "Inconsistent prior spec, word " + std::to_string(v) + " has all Zero priors!");
  // 2. what the conditional Phi phase needs
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = upload(h, &h->d_pr_mask, mask)) || (rc = dev_alloc(h, &h->d_pr_sum_phi, (size_t)h->K))) return rc;
  if (h->exact_sum && ((rc = dev_alloc(h, &h->d_pr_pref, ((size_t)h->sum_nseg + 1) * h->K)) || (rc = dev_alloc(h, &h->d_pr_fn, (size_t)h->sum_nseg * h->K * 4))))
    return rc;
  h->pr_mask.swap(mask);
  h->pr_pitch = pitch;
  h->have_priors = true;
  return GGS_OK;
}

int ggs_get_topic_priors(ggs_handle *h, double *priors) {
  if (!h || !priors) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::spalias) return set_err(h, GGS_ERR_STATE, "ggs_get_topic_priors needs GGS_FLAG_SPALIAS");
  std::fill(priors, priors + (size_t)h->K * h->V, 1.0);
  if (!h->have_priors) return GGS_OK;
  std::vector<uint32_t> mask((size_t)h->V * h->pr_pitch);       // the mask the kernels read
  if ((rc = copy_out(h, mask.data(), h->d_pr_mask, mask.size() * sizeof(uint32_t)))) return rc;
  for (int32_t v = 0; v < h->V; ++v)
    for (int32_t j = 0; j < h->pr_pitch; ++j)
      for (uint32_t bits = mask[(size_t)v * h->pr_pitch + j]; bits; bits &= bits - 1)
        priors[(size_t)(j * 32 + __builtin_ctz(bits)) * h->V + v] = 0.0;
  return GGS_OK;
}

int ggs_get_alias_tables(ggs_handle *h, double *ps, int32_t *a, double *type_norm) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_tables(h->scheme))                          // adlda: lightcollapsed's sibling has them; promised GGS_ERR_UNSUPPORTED in ggs_hip.h
    return counts_only(h->scheme) ? set_err(h, GGS_ERR_UNSUPPORTED, "scheme=adlda builds no alias tables") : set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_alias_tables", kHasTables));
  if ((rc = refresh_tables(h))) return rc;
  const size_t kv = (size_t)h->K * h->V;
  std::vector<int32_t> n(count_tables(h->scheme) ? (size_t)h->V : 0);   // lightcollapsed, lightpcldaw2: the kernel writes a row's first nw[w] entries
  if (!n.empty()) HIP_TRY(h, hipMemcpyAsync(n.data(), h->d_nw, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (ps) HIP_TRY(h, hipMemcpyAsync(ps, h->d_alias_ps, kv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (a) HIP_TRY(h, hipMemcpyAsync(a, h->d_alias_a, kv * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (type_norm) HIP_TRY(h, hipMemcpyAsync(type_norm, h->d_alias_tn, (size_t)h->V * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t w = 0; w < n.size(); ++w)                // ... behind them ps = 1.0, a = the index
    for (int32_t i = n[w]; i < h->K; ++i) {
      if (ps) ps[w * h->K + i] = 1.0;
      if (a) a[w * h->K + i] = i;
    }
  return GGS_OK;
}
int ggs_get_mh_stats(ggs_handle *h, int64_t out[3]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_mh(h->scheme))                              // adlda: as in ggs_get_alias_tables
    return counts_only(h->scheme) ? set_err(h, GGS_ERR_UNSUPPORTED, "scheme=adlda has no Metropolis-Hastings step") : set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_mh_stats", kHasMh));
  unsigned long long v[3];
  HIP_TRY(h, hipMemcpyAsync(v, h->d_mh, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 3; ++i) out[i] = (int64_t)v[i];
  return GGS_OK;
}
int ggs_get_word_topic_lists(ggs_handle *h, int32_t *nw, int32_t *topics) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_word_lists(h->scheme)) return set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_word_topic_lists", kHasWordLists));
  if ((rc = refresh_tables(h))) return rc;
  const size_t kv = (size_t)h->K * h->V;
  std::vector<int32_t> n((size_t)h->V);
  std::vector<uint16_t> l(topics ? kv : 0);
  HIP_TRY(h, hipMemcpyAsync(n.data(), h->d_nw, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (topics) HIP_TRY(h, hipMemcpyAsync(l.data(), h->d_nzw, kv * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (nw) std::copy(n.begin(), n.end(), nw);
  if (topics)
    for (int32_t w = 0; w < h->V; ++w)
      for (int32_t i = 0; i < h->K; ++i) topics[(size_t)w * h->K + i] = i < n[(size_t)w] ? (int32_t)l[(size_t)w * h->K + i] : -1;
  return GGS_OK;
}
int ggs_get_sparse_stats(ggs_handle *h, int64_t out[4]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_sparse_stats(h->scheme)) return set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_sparse_stats", kSparseStats));
  unsigned long long v[4];
  HIP_TRY(h, hipMemcpyAsync(v, h->d_ps_stats, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; ++i) out[i] = (int64_t)v[i];
  return GGS_OK;
}
int ggs_set_variable_selection_prior(ggs_handle *h, double pi) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (h->scheme != Scheme::nzvsspalias) return set_err(h, GGS_ERR_STATE, "ggs_set_variable_selection_prior needs GGS_FLAG_NZVSSPALIAS");
  if (h->have_phi) return set_err(h, GGS_ERR_STATE, "ggs_set_variable_selection_prior: the handle already has a Phi");
  if (!(pi > 0.0 && pi < 1.0)) return set_err(h, GGS_ERR_BAD_ARG, "the variable-selection prior must lie in (0, 1)");
  h->vs_pi = pi;
  return GGS_OK;
}
int ggs_get_vs_stats(ggs_handle *h, int64_t out[3]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::nzvsspalias) return set_err(h, GGS_ERR_STATE, "ggs_get_vs_stats needs GGS_FLAG_NZVSSPALIAS");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi yet: call ggs_init_phi or ggs_set_phi first");
  out[0] = out[1] = out[2] = 0;
  HIP_TRY(h, hipMemsetAsync(h->d_vs_zero, 0, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(vs_zero_cells_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 4)), dim3(256), 0, h->stream, h->d_phiT, h->K, h->Kp, h->V, h->d_vs_zero);
  HIP_TRY(h, hipGetLastError());
  unsigned long long zero = 0;
  if ((rc = copy_out(h, &zero, h->d_vs_zero, sizeof zero))) return rc;
  out[1] = (int64_t)zero;
  if (!h->vs_drawn) return GGS_OK;                     // no variable-selection draw yet: nothing undrawn, no rounds
  std::vector<uint32_t> und((size_t)h->V * h->vs_pitch);    // the by-word mask: every topic's cells, with an exchange too
  std::vector<int32_t> rounds((size_t)h->Ks);               // the chains this handle ran: its own topics
  if ((rc = copy_out(h, und.data(), h->d_vs_mask, und.size() * sizeof(uint32_t))) || (rc = copy_out(h, rounds.data(), h->d_vs_rounds, rounds.size() * sizeof(int32_t))))
    return rc;
  for (uint32_t w : und) out[0] += __builtin_popcount(w);
  for (int32_t r : rounds) out[2] = std::max<int64_t>(out[2], r);
  return GGS_OK;
}
int ggs_get_phi_mean(ggs_handle *h, double *phi_mean, int32_t *n_sampled) {
  if (!h || !n_sampled) return GGS_ERR_BAD_ARG;
  *n_sampled = h->n_sampled_phi;
  if (h->n_sampled_phi == 0 || !h->d_phi_mean) return GGS_OK;   // Java returns null (UPLDA:1955-1958)
  if (!phi_mean) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  return phi_out(h, h->d_phi_mean, h->K, phi_mean, (double)h->n_sampled_phi);
}
int ggs_get_theta(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *theta) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (doc_begin < 0 || doc_end > h->D || doc_begin > doc_end || (!theta && doc_end > doc_begin)) return set_err(h, GGS_ERR_BAD_ARG, "bad document range");
  if (counts_only(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightcollapsed and scheme=adlda keep no theta");
  if (no_theta(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightpcldaw2 keeps no theta");
  return copy_out(h, theta, h->d_theta + (size_t)doc_begin * h->K, sizeof(double) * (size_t)(doc_end - doc_begin) * h->K);
}
int ggs_get_doc_topic_counts(ggs_handle *h, int64_t doc_begin, int64_t doc_end, int32_t *n_dk) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (doc_begin < 0 || doc_end > h->D || doc_begin > doc_end || (!n_dk && doc_end > doc_begin)) return set_err(h, GGS_ERR_BAD_ARG, "bad document range");
  const int64_t nd = doc_end - doc_begin;
  if (nd == 0) return GGS_OK;
  const size_t bytes = (size_t)nd * h->K * sizeof(int32_t);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  hipLaunchKernelGGL(doc_topic_kernel, dim3((unsigned)nd), dim3(64), 0, h->stream, h->d_doc_ptr, h->d_z, doc_begin, h->K, static_cast<int32_t *>(h->d_scratch));
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, n_dk, h->d_scratch, bytes);
}
int ggs_doc_topic_histogram(ggs_handle *h, int32_t symmetric, int64_t n_bins, int32_t *hist, int32_t *doc_lengths) {
  return doc_topic_histogram(h, symmetric, n_bins, hist, doc_lengths);
}
int ggs_type_topic_count_histogram(ggs_handle *h, int64_t n_bins, int32_t *hist) { return type_topic_count_histogram(h, n_bins, hist); }
int ggs_set_hyperparameters(ggs_handle *h, const double *alpha, double beta, double beta_sum) { return set_hyperparameters(h, alpha, beta, beta_sum); }
int ggs_get_hyperparameters(const ggs_handle *h, double *alpha, double *beta, double *beta_sum) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (alpha) std::copy(h->alpha.begin(), h->alpha.end(), alpha);
  if (beta) *beta = h->beta;
  if (beta_sum) *beta_sum = h->beta_sum;
  return GGS_OK;
}
int ggs_learn_symmetric_concentration(const int32_t *count_hist, int64_t n_hist, const int32_t *obs_lengths, int64_t n_len, int32_t num_dimensions,
                                      double current, double *out) {
  if (!count_hist || n_hist < 1 || !obs_lengths || n_len < 1 || num_dimensions < 1 || !out) return GGS_ERR_BAD_ARG;
  *out = mallet_learn_symmetric_concentration(count_hist, n_hist, obs_lengths, n_len, num_dimensions, current);
  return GGS_OK;
}
int ggs_learn_parameters(double *params, int32_t K, const int32_t *obs, int64_t n_bins, const int32_t *obs_lengths, int64_t n_len, double shape, double scale,
                         int32_t iterations, double *sum_out) {
  if (!params || K < 1 || !obs || n_bins < 1 || !obs_lengths || n_len < 1 || iterations < 0 || !sum_out) return GGS_ERR_BAD_ARG;
  *sum_out = mallet_learn_parameters(params, K, obs, n_bins, obs_lengths, n_len, shape, scale, iterations);
  return GGS_OK;
}
int ggs_model_log_likelihood(ggs_handle *h, double *doc_side, double *topic_side) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!doc_side || !topic_side) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = launch_magnitude(h))) return rc;       // corpus-wide counts gathered, tokensPerTopic in step with them
  const int K = h->K;
  if ((rc = ll_check_topics(h))) return rc;
  const int64_t doc_blocks = (h->D + kLLBlock / 64 - 1) / (kLLBlock / 64), type_blocks = 1024;
  const size_t bytes = 32 + sizeof(double) * (size_t)(doc_blocks + type_blocks);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_out = static_cast<double *>(h->d_scratch);                       // [0] document side, [1] topic side
  auto *d_nz = reinterpret_cast<unsigned long long *>(d_out + 2);
  double *d_doc = d_out + 4, *d_type = d_doc + doc_blocks;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, 32, h->stream));
  const double alpha_sum = h->alpha_sum;               // the k-order sum
  if (doc_blocks)
    hipLaunchKernelGGL(ll_docs_kernel, dim3((unsigned)doc_blocks), dim3(kLLBlock), ll_docs_lds_bytes(K), h->stream, h->d_doc_ptr,
                       h->d_z, h->d_alpha, alpha_sum, h->D, K, d_doc);
  hipLaunchKernelGGL(ll_types_kernel, dim3((unsigned)type_blocks), dim3(kLLBlock), 0, h->stream, h->d_n_wk, (int64_t)K * h->V, h->beta, d_type, d_nz);
  hipLaunchKernelGGL(ll_finish_kernel, dim3(1), dim3(kLLBlock), 0, h->stream, d_doc, doc_blocks, d_type, type_blocks, h->d_n_k, K, h->beta_sum,
                     alpha_sum, h->beta, h->D, d_nz, d_out);
  HIP_TRY(h, hipGetLastError());
  double out[2];
  if ((rc = copy_out(h, out, d_out, sizeof out))) return rc;
  *doc_side = out[0]; *topic_side = out[1];
  return GGS_OK;
}
int ggs_log_posterior(ggs_handle *h, double *doc_side, double *topic_side) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!doc_side || !topic_side) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if (count_form(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed and scheme=lightcollapsed have no Phi: the log posterior of UPLDA:1573-1634 does not apply");
  if ((rc = ll_check_topics(h))) return rc;
  if (pcgs_family(h->scheme)) {
    // UPLDA:710-714: every scheme but ggs draws theta_d ~ Dir(n_d. + alpha) afresh for the diagnostics
    // (LDAUtils.drawDirichlets); here: the theta draw of GGS:57-72 under the stream GGS_PURPOSE_THETA at the current iteration
    if ((rc = drop_theta_ahead(h)) || (rc = ensure_diag_theta(h)) || (rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  const int K = h->K;
  const int64_t doc_blocks = (h->D + kLLBlock / 64 - 1) / (kLLBlock / 64), phi_blocks = 1024;
  const size_t bytes = 32 + sizeof(double) * (size_t)(doc_blocks + phi_blocks);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_out = static_cast<double *>(h->d_scratch);
  double *d_doc = d_out + 4, *d_phi = d_doc + doc_blocks;
  if (doc_blocks)
    hipLaunchKernelGGL(lp_docs_kernel, dim3((unsigned)doc_blocks), dim3(kLLBlock), ll_docs_lds_bytes(K), h->stream, h->d_doc_ptr,
                       h->d_tok, h->d_z, h->d_alpha, h->d_theta, h->d_phiT, h->D, K, h->Kp, d_doc);
  hipLaunchKernelGGL(lp_phi_kernel, dim3((unsigned)phi_blocks), dim3(kLLBlock), 0, h->stream, h->d_phiT, (int64_t)h->V, K, h->Kp, d_phi);
  hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(kLLBlock), 0, h->stream, d_doc, doc_blocks, d_phi, phi_blocks, h->beta, d_out);
  HIP_TRY(h, hipGetLastError());
  double out[2];
  if ((rc = copy_out(h, out, d_out, sizeof out))) return rc;
  *doc_side = out[0]; *topic_side = out[1];
  return GGS_OK;
}
int ggs_min_doc_distances(ggs_handle *h, const double *other, int64_t n_other, double *min_dist) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme))
    return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, lightcollapsed and adlda draw no theta: the document distances of UPLDA:723-753 do not apply");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  const int64_t D = h->D, K = h->K;
  if (n_other < 0 || (!other && n_other != 0) || (!min_dist && D > 0)) return set_err(h, GGS_ERR_BAD_ARG, "null output or negative size");
  if (D == 0) return GGS_OK;
  if (pcgs_family(h->scheme)) {
    // UPLDA:710-714: one fresh theta per diagnostic iteration for the distances and the log posterior together; here both
    // calls redraw the same bits (the stream GGS_PURPOSE_THETA at the current iteration), as ggs_log_posterior does
    if ((rc = drop_theta_ahead(h)) || (rc = ensure_diag_theta(h)) || (rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  const int64_t piece_rows = other ? std::max<int64_t>(1, std::min<int64_t>(n_other, (int64_t)(dist_piece_bytes() / (sizeof(double) * (size_t)K)))) : 0;
  const size_t head = sizeof(double) * 2 * (size_t)D;     // [D] minimal sums as bit patterns, [D] distances
  if ((rc = ensure_scratch(h, head + sizeof(double) * (size_t)piece_rows * (size_t)K))) return rc;
  auto *d_bits = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_out = reinterpret_cast<double *>(d_bits + D);
  double *d_piece = d_out + D;
  const int grid = grid_for(D, 256);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid), dim3(256), 0, h->stream, d_bits, D);
  if (!other) launch_min_row_dist(h->stream, h->d_theta, D, h->d_theta, D, K, true, d_bits);
  for (int64_t r0 = 0; other && r0 < n_other; r0 += piece_rows) {
    const int64_t rows = std::min(piece_rows, n_other - r0);
    HIP_TRY(h, hipMemcpyAsync(d_piece, other + r0 * K, sizeof(double) * (size_t)rows * (size_t)K, hipMemcpyHostToDevice, h->stream));
    launch_min_row_dist(h->stream, h->d_theta, D, d_piece, rows, K, false, d_bits);
    if (r0 + piece_rows < n_other) HIP_TRY(h, hipStreamSynchronize(h->stream));   // the piece is overwritten next
  }
  hipLaunchKernelGGL(min_dist_finish_kernel, dim3(grid), dim3(256), 0, h->stream, d_bits, D, d_out, static_cast<double *>(nullptr));
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, min_dist, d_out, sizeof(double) * (size_t)D);
}

int ggs_min_topic_distance(ggs_handle *h, double *min_dist) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme))
    return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, lightcollapsed and adlda draw no Phi: the topic distances of UPLDA:778-806 do not apply");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  if (!min_dist) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  const int64_t K = h->K;
  if ((rc = ensure_scratch(h, sizeof(double) * ((size_t)K + 1)))) return rc;
  auto *d_bits = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_out = reinterpret_cast<double *>(d_bits + K);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid_for(K, 256)), dim3(256), 0, h->stream, d_bits, K);
  launch_min_topic_dist(h->stream, h->d_phiT, K, h->Kp, h->V, d_bits);
  hipLaunchKernelGGL(min_dist_reduce_kernel, dim3(1), dim3(kDistBlock), 0, h->stream, d_bits, K, d_out);
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, min_dist, d_out, sizeof(double));
}
int ggs_get_theta_estimate(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *out) { return sim_get_doc_rows(h, doc_begin, doc_end, false, out); }
int ggs_get_zbar(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *out) { return sim_get_doc_rows(h, doc_begin, doc_end, true, out); }
int ggs_nearest_documents(ggs_handle *h, int32_t metric, const double *query, const int64_t *query_len, int64_t Q, int32_t n_nearest, int64_t *idx, double *dist) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (n_nearest < 1 || n_nearest > kSimMaxNearest) return set_err(h, GGS_ERR_BAD_ARG, "n_nearest must be in [1, GGS_NEAREST_MAX]");
  return sim_handle_distances(h, metric, query, query_len, Q, n_nearest, idx, dist);
}
int ggs_document_distances(ggs_handle *h, int32_t metric, const double *query, const int64_t *query_len, int64_t Q, double *dist) {
  return sim_handle_distances(h, metric, query, query_len, Q, 0, nullptr, dist);
}
int ggs_row_distances(int32_t device_id, int32_t metric, const double *a, const double *b, int64_t n, int64_t m, int64_t len, double *out) {
  return sim_row_distances(device_id, metric, a, b, n, m, len, out);
}
int ggs_top_words(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t *idx, double *score) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if ((rc = ts_check_args(h, h->V, h->K, h->beta, kind, n_words, lambda, idx))) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  const TsPlan q(h->V, h->K, n_words);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  ts_launch(h->stream, h->exact_sum, h->d_n_wk, h->beta, lambda, kind, q, work, false, nullptr);
  HIP_TRY(h, hipGetLastError());
  if ((rc = copy_out(h, idx, work + q.idx, sizeof(int32_t) * (size_t)h->K * n_words))) return rc;
  return score ? copy_out(h, score, work + q.score, sizeof(double) * (size_t)h->K * n_words) : GGS_OK;
}
int ggs_debug_top_words_phases(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t element_chain, double *ms) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  int32_t dummy = 0;
  if (!ms) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = ts_check_args(h, h->V, h->K, h->beta, kind, n_words, lambda, &dummy))) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  const TsPlan q(h->V, h->K, n_words);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  ScopedEvents<5> ev;
  while (ev.n < 5)
    if (!ev.make()) return set_err(h, GGS_ERR_HIP, "hipEventCreate");
  ts_launch(h->stream, element_chain ? false : h->exact_sum, h->d_n_wk, h->beta, lambda, kind, q, static_cast<char *>(h->d_scratch), false, nullptr, ev.ev);
  HIP_TRY(h, hipGetLastError());
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; ++i) { float f = 0; HIP_TRY(h, hipEventElapsedTime(&f, ev.ev[i], ev.ev[i + 1])); ms[i] = f; }
  return GGS_OK;
}
int ggs_topic_doc_statistics(ggs_handle *h, int32_t n_words, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats, double *clogc_out) {
  return td_doc_statistics(h, n_words, idx, clogc_in, codoc, doc_stats, clogc_out, nullptr);
}
int ggs_topic_scores(ggs_handle *h, int32_t n_words, const int32_t *idx, const int32_t *codoc, const int32_t *doc_stats, const double *clogc, double *topic_scores,
                     double *word_scores) {
  return td_scores(h, n_words, idx, codoc, doc_stats, clogc, topic_scores, word_scores, nullptr);
}
int ggs_debug_topic_diagnostics_phases(ggs_handle *h, int32_t n_words, double *ms) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!ms) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = td_check_args(h, h->V, h->K, n_words, nullptr))) return rc;
  const size_t K = (size_t)h->K, n = (size_t)n_words;
  std::vector<int32_t> idx(K * n), codoc(K * n * n), stats(K * kTdStats);
  std::vector<double> clogc(K), ts(kTdScoreRows * K);
  if ((rc = ggs_top_words(h, GGS_TOP_WORDS, n_words, 0.0, idx.data(), nullptr))) return rc;
  for (int i = 0; i < kTdPhases; ++i) ms[i] = 0;
  {
    TdTimer tm{h->stream, {}};
    if ((rc = td_doc_statistics(h, n_words, idx.data(), nullptr, codoc.data(), stats.data(), clogc.data(), &tm))) return rc;
    if (!tm.collect(ms)) return set_err(h, GGS_ERR_UNSUPPORTED, "the phase timer holds 1024 marks: too many pieces of documents for it");
  }
  TdTimer tm{h->stream, {}};
  if ((rc = td_scores(h, n_words, idx.data(), codoc.data(), stats.data(), clogc.data(), ts.data(), nullptr, &tm))) return rc;
  return tm.collect(ms) ? GGS_OK : set_err(h, GGS_ERR_HIP, "the phase timer could not create an event");
}
int ggs_set_test_corpus(ggs_handle *h, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, int64_t doc_base) {
  if (!h || D < 0 || !doc_ptr || doc_base < 0) return set_err(h, GGS_ERR_BAD_ARG, "bad test corpus arguments");
  if (doc_ptr[0] != 0) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr[0] must be 0");
  for (int64_t d = 0; d < D; ++d) {
    if (doc_ptr[d + 1] < doc_ptr[d]) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr must be non-decreasing");
    if (doc_ptr[d + 1] - doc_ptr[d] > ((int64_t)1 << 25))
      return set_err(h, GGS_ERR_UNSUPPORTED, "a test document has more than 2^25 tokens (one Philox stream per particle: 2^24 blocks of two uniforms)");
  }
  const int64_t N = doc_ptr[D];
  if (N > 0 && !tokens) return set_err(h, GGS_ERR_BAD_ARG, "tokens is null");
  for (int64_t i = 0; i < N; ++i)
    if (tokens[i] < 0) return set_err(h, GGS_ERR_BAD_ARG, "negative token id");    // ids >= num_types are out of vocabulary (MPE:341-345)
  int rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = dev_alloc(h, &h->d_test_ptr, (size_t)D + 1)) || (rc = dev_alloc(h, &h->d_test_tok, (size_t)N)) || (rc = dev_alloc(h, &h->d_test_ll, (size_t)D))) return rc;
  HIP_TRY(h, hipMemcpy(h->d_test_ptr, doc_ptr, sizeof(int64_t) * (size_t)(D + 1), hipMemcpyHostToDevice));
  if (N) HIP_TRY(h, hipMemcpy(h->d_test_tok, tokens, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice));
  h->test_ptr.assign(doc_ptr, doc_ptr + D + 1);
  // by the width a particle's per-topic counts need: one byte (documents of at most 255 tokens), two (65 535), four
  h->test_short.clear(); h->test_long.clear(); h->test_huge.clear();
  for (int64_t d = 0; d < D; ++d) {
    const int64_t len = doc_ptr[d + 1] - doc_ptr[d];
    (len <= 255 ? h->test_short : len <= 65535 ? h->test_long : h->test_huge).push_back((int32_t)d);
  }
  if ((rc = dev_alloc(h, &h->d_test_docs, (size_t)D))) return rc;
  {
    size_t at = 0;
    for (const std::vector<int32_t> *ids : {&h->test_short, &h->test_long, &h->test_huge}) {
      if (!ids->empty()) HIP_TRY(h, hipMemcpy(h->d_test_docs + at, ids->data(), sizeof(int32_t) * ids->size(), hipMemcpyHostToDevice));
      at += ids->size();
    }
  }
  h->test_doc_base = doc_base;
  h->have_test = true;
  return GGS_OK;
}

int ggs_heldout_log_likelihood(ggs_handle *h, int32_t num_particles, double *doc_ll, double *total) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!h->have_test) return set_err(h, GGS_ERR_STATE, "no test set: call ggs_set_test_corpus first");
  if (num_particles < 1 || !total) return set_err(h, GGS_ERR_BAD_ARG, "num_particles < 1 or null output");
  return heldout_evaluate(h, num_particles, doc_ll, total);
}

int ggs_get_timings(ggs_handle *h, ggs_timings *out) { if (!h || !out) return GGS_ERR_BAD_ARG; *out = h->tm; return GGS_OK; }
int ggs_reset_timings(ggs_handle *h) { if (!h) return GGS_ERR_BAD_ARG; h->tm = ggs_timings{}; return GGS_OK; }

int ggs_check_invariants(ggs_handle *h) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  const int K = h->K;
  const size_t bytes = 16 + sizeof(int32_t) * (size_t)K;
  if ((rc = ensure_global_counts(h))) return rc;
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_total = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_flags = reinterpret_cast<uint32_t *>(static_cast<char *>(h->d_scratch) + 8);
  auto *d_col = reinterpret_cast<int32_t *>(static_cast<char *>(h->d_scratch) + 16);
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  const int64_t kv = (int64_t)K * h->V;
  hipLaunchKernelGGL(invariants_kernel, dim3(grid_for(kv, 256)), dim3(256), 0, h->stream, h->d_n_wk, kv, K, d_total, d_col, d_flags);
  HIP_TRY(h, hipGetLastError());
  if ((rc = launch_magnitude(h))) return rc;
  std::vector<unsigned char> host(bytes);
  std::vector<int32_t> nk((size_t)K);
  if ((rc = copy_out(h, host.data(), h->d_scratch, bytes))) return rc;
  if ((rc = copy_out(h, nk.data(), h->d_n_k, sizeof(int32_t) * (size_t)K))) return rc;
  unsigned long long total; uint32_t fl;
  std::memcpy(&total, host.data(), 8); std::memcpy(&fl, host.data() + 8, 4);
  const int32_t *col = reinterpret_cast<const int32_t *>(host.data() + 16);
  if (fl & 1u) return set_err(h, GGS_ERR_INVARIANT, "negative type-topic count");
  if ((int64_t)total != (h->global_tokens >= 0 ? h->global_tokens : h->N)) return set_err(h, GGS_ERR_INVARIANT, "type-topic counts do not sum to the corpus size");
  for (int k = 0; k < K; ++k)
    if (col[k] != nk[(size_t)k]) return set_err(h, GGS_ERR_INVARIANT, "column sum differs from tokensPerTopic");
  return GGS_OK;
}

int ggs_get_launch_info(ggs_handle *h, int64_t *num_chunks, int32_t *lds_bytes_z, int32_t *docs_per_block_theta) {
  if (!h) return GGS_ERR_BAD_ARG;
  const LaunchPlan &pl = h->plan;
  const bool pcgs = pcgs_family(h->scheme);            // what launch_pcgs_z launches, over what
  if (num_chunks) *num_chunks = pcgs ? h->pcgs_items : pl.sliced() ? h->Cs + h->Cw : h->C;
  if (lds_bytes_z) *lds_bytes_z = pcgs ? h->pcgs_z.lds : pl.sliced() ? sliced_fused_lds(h->K, pl.hot_cap) : pl.z.lds;
  if (docs_per_block_theta) *docs_per_block_theta = h->cfg->theta_docs;
  return GGS_OK;
}

int ggs_get_num_hot_words(ggs_handle *h, int32_t *num_hot) {
  if (!h || !num_hot) return GGS_ERR_BAD_ARG;
  *num_hot = h->plan.sliced() ? h->num_hot + h->num_warm : 0;
  return GGS_OK;
}

int ggs_get_z_parts(ggs_handle *h, int32_t *parts) {
  if (!h || !parts) return GGS_ERR_BAD_ARG;
  const int32_t P = (int32_t)h->part_doc.size() - 1;
  *parts = (h->plan.stream() && h->overlap_theta && P > 1) ? P : 1;
  return GGS_OK;
}

int ggs_get_warm_tiers(ggs_handle *h, int32_t *tiers, int32_t *warm_words, int32_t *docs_per_chunk) {
  if (!h) return GGS_ERR_BAD_ARG;
  const bool on = h->have_corpus && h->plan.sliced();
  if (tiers) *tiers = on ? h->warm_tiers : 0;
  if (warm_words) *warm_words = on ? h->num_warm : 0;
  if (docs_per_chunk) *docs_per_chunk = on && h->warm_tiers ? h->plan.warm_docs : 0;
  return GGS_OK;
}

int ggs_get_hot_pairs(ggs_handle *h, int32_t *enabled, int64_t *pair_chunks, int64_t *pairs, int64_t *tokens) {
  if (!h) return GGS_ERR_BAD_ARG;
  const bool built = h->have_corpus && h->plan.sliced() && h->plan.hot_pairs;
  if (enabled) *enabled = (built && h->Cp > 0 && h->z_split && h->Cs > h->Cc && h->Cc > 0) ? 1 : 0;
  if (pair_chunks) *pair_chunks = built ? h->Cp : 0;
  if (pairs) *pairs = built ? h->hp_pairs : 0;
  if (tokens) *tokens = built ? h->hp_tokens : 0;
  return GGS_OK;
}

int ggs_get_z_form(ggs_handle *h, int32_t *kernel, int32_t *form, int32_t *calibrated) {
  if (!h) return GGS_ERR_BAD_ARG;
  const bool splittable = h->plan.sliced() && h->Cs > h->Cc && h->Cc > 0;
  const int32_t own = row_of(h->scheme).z_kernel;
  if (kernel) *kernel = own ? own : pcgs_family(h->scheme) ? (h->pcgs_wave ? 5 : 4) : h->plan.kernel;
  if (form) *form = h->plan.sliced() ? (splittable && h->z_split ? 1 : 2) : 0;
  if (calibrated) *calibrated = (splittable && h->z_split_tried && !h->plan.split_forced && h->plan.split) ? 1 : 0;
  return GGS_OK;
}

int ggs_java_lcg_next_ints(int32_t seed, int32_t bound, int64_t n, int32_t *out) {
  if (bound <= 0 || n < 0 || (n > 0 && !out)) return GGS_ERR_BAD_ARG;
  java_lcg_next_ints(seed, bound, n, out);
  return GGS_OK;
}

// ---- primitives for the parity tests ---------------------------------------------
int ggs_debug_philox(int32_t device_id, int64_t n, const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  if (n <= 0 || !ctr || !key || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *dc = static_cast<uint32_t *>(t.get(n * 16)); auto *dk = static_cast<uint32_t *>(t.get(n * 8)); auto *dou = static_cast<uint32_t *>(t.get(n * 16));
  if (!dc || !dk || !dou) return GGS_ERR_HIP;
  if (hipMemcpy(dc, ctr, n * 16, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dk, key, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, n, dc, dk, dou);
  if (hipMemcpy(out, dou, n * 16, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_math(int32_t device_id, int32_t op, int64_t n, const double *x, const double *y, double *out) {
  if (n <= 0 || !x || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *dx = static_cast<double *>(t.get(n * 8)); auto *dy = static_cast<double *>(t.get(n * 8)); auto *dou = static_cast<double *>(t.get(n * 8));
  if (!dx || !dy || !dou) return GGS_ERR_HIP;
  if (hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemcpy(dy, y ? y : x, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, n, dx, dy, dou);
  if (hipMemcpy(out, dou, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_draw(int32_t device_id, int32_t kind, uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0, int64_t n,
                   const double *shape, double *out, int32_t *status) {
  if (n <= 0 || !out || (kind == 2 && !shape) || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *ds = static_cast<double *>(t.get(n * 8)); auto *dou = static_cast<double *>(t.get(n * 8)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!ds || !dou || !dst) return GGS_ERR_HIP;
  if (shape && hipMemcpy(ds, shape, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemset(dst, 0, 16) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_draw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, seed, iteration, purpose, elem0, n, ds, dou, dst);
  uint32_t st = 0;
  if (hipMemcpy(out, dou, n * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  if (status) *status = (int32_t)st;
  return GGS_OK;
}

int ggs_debug_poisson(int32_t device_id, double beta, int32_t threshold, uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0, int64_t n,
                      const int32_t *counts, int32_t *out) {
  const int32_t L = threshold == 0 ? 100 : threshold;
  if (n <= 0 || !counts || !out || !(beta > 0) || L < 1 || L > kPoissonMaxThreshold || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  for (int64_t i = 0; i < n; ++i)
    if (counts[i] < 0) return GGS_ERR_BAD_ARG;
  std::vector<double> T;
  build_poisson_table(beta, L, T);
  TmpDev t;
  auto *dt = static_cast<double *>(t.get(T.size() * 8)); auto *dc = static_cast<int32_t *>(t.get(n * 4));
  auto *dou = static_cast<int32_t *>(t.get(n * 4)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!dt || !dc || !dou || !dst) return GGS_ERR_HIP;
  if (hipMemcpy(dt, T.data(), T.size() * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dc, counts, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dst, 0, 16) != hipSuccess)
    return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_poisson_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, seed, iteration, purpose, elem0, n, dc, L, beta, dt, T[0],
                     dou, dst);
  uint32_t st = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpy(out, dou, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return st ? GGS_ERR_RNG_EXHAUSTED : GGS_OK;
}

int ggs_debug_alias(int32_t device_id, int32_t V, int32_t K, const double *phi, const double *alpha, double *ps, int32_t *a, double *type_norm) {
  if (V <= 0 || K <= 0 || K > kPcgsWaveMaxTopics || !phi || !alpha || !ps || !a || !type_norm || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  const size_t kv = (size_t)K * V;
  std::vector<double> phiT(kv);                         // [V][K], as the handle keeps it (pitch K here)
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) phiT[(size_t)v * K + k] = phi[(size_t)k * V + v];
  TmpDev t;
  auto *dphi = static_cast<double *>(t.get(kv * 8)); auto *dal = static_cast<double *>(t.get((size_t)K * 8));
  auto *dps = static_cast<double *>(t.get(kv * 8)); auto *da = static_cast<int32_t *>(t.get(kv * 4)); auto *dtn = static_cast<double *>(t.get((size_t)V * 8));
  if (!dphi || !dal || !dps || !da || !dtn) return GGS_ERR_HIP;
  if (hipMemcpy(dphi, phiT.data(), kv * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dal, alpha, (size_t)K * 8, hipMemcpyHostToDevice) != hipSuccess)
    return GGS_ERR_HIP;
  AliasParams ap{};
  ap.phiT = dphi; ap.alpha = dal; ap.ps = dps; ap.a = da; ap.type_norm = dtn; ap.V = V; ap.K = K; ap.Kp = K; ap.wpb = alias_words_per_block(K);
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(alias_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(alias_build_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)V + ap.wpb - 1) / ap.wpb, 4096)), dim3(64), alias_lds_bytes(K, ap.wpb), nullptr, ap);
  if (hipGetLastError() != hipSuccess || hipMemcpy(ps, dps, kv * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(a, da, kv * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(type_norm, dtn, (size_t)V * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_vs_indicators(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, const double *prev_phi, double beta, double pi, uint64_t seed,
                            uint32_t iteration, const double *u, uint8_t *drawn_out, int32_t *s_end, int32_t *rounds) {
  if (V <= 0 || K <= 0 || !counts || !prev_phi || !drawn_out || !s_end || !rounds || !(beta > 0) || !(pi > 0.0 && pi < 1.0) || hipSetDevice(device_id) != hipSuccess)
    return GGS_ERR_BAD_ARG;
  const Knobs kn;
  const bool global = V > kVsLdsMaxV || (kn.vs_global.set && kn.vs_global.v != 0);
  const size_t kv = (size_t)K * V;
  const int32_t W = (V + 31) / 32;
  const size_t kw = (size_t)K * W;
  std::vector<int32_t> cntT(kv), n_k((size_t)K, 0);     // [V][K], as the handle keeps them
  std::vector<double> phiT(kv);
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) {
      const int32_t c = counts[(size_t)k * V + v];
      if (c < 0) return GGS_ERR_BAD_ARG;
      cntT[(size_t)v * K + k] = c; n_k[(size_t)k] += c;
      phiT[(size_t)v * K + k] = prev_phi[(size_t)k * V + v];
    }
  TmpDev t;
  auto *dc = static_cast<int32_t *>(t.get(kv * 4)); auto *dphi = static_cast<double *>(t.get(kv * 8)); auto *dnk = static_cast<int32_t *>(t.get((size_t)K * 4));
  auto *dcz = static_cast<uint32_t *>(t.get(kw * 4)); auto *dpz = static_cast<uint32_t *>(t.get(kw * 4)); auto *dun = static_cast<uint32_t *>(t.get(kw * 4));
  auto *dwork = static_cast<int32_t *>(t.get(global ? 2 * kw * 4 : 16)); auto *du = static_cast<double *>(t.get(u ? kv * 8 : 16));
  auto *dse = static_cast<int32_t *>(t.get((size_t)K * 4)); auto *dro = static_cast<int32_t *>(t.get((size_t)K * 4)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!dc || !dphi || !dnk || !dcz || !dpz || !dun || !dwork || !du || !dse || !dro || !dst) return GGS_ERR_HIP;
  if (hipMemcpy(dc, cntT.data(), kv * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dphi, phiT.data(), kv * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dnk, n_k.data(), (size_t)K * 4, hipMemcpyHostToDevice) != hipSuccess || (u && hipMemcpy(du, u, kv * 8, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemset(dst, 0, 16) != hipSuccess)
    return GGS_ERR_HIP;
  VsBitsParams bp{};
  bp.cnt = dc; bp.phiT = dphi; bp.cz = dcz; bp.pz = dpz; bp.cnt_pitch = K; bp.Kp = K; bp.k0 = 0; bp.Ks = K; bp.V = V; bp.W = W;
  hipLaunchKernelGGL(vs_bits_kernel, dim3((unsigned)std::min<int64_t>((int64_t)W * ((K + 63) / 64), 4096)), dim3(64), 0, nullptr, bp);
  VsChainParams cp{};
  cp.cz = dcz; cp.pz = dpz; cp.und = dun; cp.work = dwork; cp.n_k = dnk; cp.u = u ? du : nullptr; cp.s_end = dse; cp.rounds = dro; cp.status = dst;
  cp.seed = seed; cp.iteration = iteration; cp.Ks = K; cp.k0 = 0; cp.V = V; cp.W = W; cp.beta = beta; cp.odds = pi / (1 - pi);
  if (global) hipLaunchKernelGGL(vs_chain_kernel<true>, dim3((unsigned)K), dim3(kVsBlock), 0, nullptr, cp);
  else hipLaunchKernelGGL(vs_chain_kernel<false>, dim3((unsigned)K), dim3(kVsBlock), vs_chain_lds_bytes(W), nullptr, cp);
  std::vector<uint32_t> und(kw);
  uint32_t st = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpy(und.data(), dun, kw * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(s_end, dse, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rounds, dro, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) drawn_out[(size_t)k * V + v] = (uint8_t)(((und[(size_t)k * W + (v >> 5)] >> (v & 31)) & 1u) ^ 1u);
  return (st & ST_INVARIANT) ? GGS_ERR_INVARIANT : GGS_OK;
}

int ggs_debug_column_sum_guided(int32_t device_id, int32_t V, int32_t K, const double *x, const int32_t *counts, double beta, const double *guess,
                                double *out, double *pref_out, int32_t *n_k_out) {
  if (V <= 0 || K <= 0 || (!x == !counts) || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const size_t kv = (size_t)V * K;
  SumCtx tmp{nullptr, V, beta, true, (V + kSumSegRows - 1) / kSumSegRows, nullptr, nullptr};   // what launch_column_sum reads
  const size_t pref_bytes = ((size_t)tmp.sum_nseg + 1) * K * 8;
  tmp.pref = static_cast<double *>(t.get(pref_bytes));
  tmp.fn = static_cast<double *>(t.get((size_t)tmp.sum_nseg * K * 32));
  void *dsrc = t.get(kv * (x ? 8 : 4));
  auto *dou = static_cast<double *>(t.get((size_t)K * 8));
  auto *dnk = static_cast<int32_t *>(t.get((size_t)K * 4));
  int rc = GGS_OK;
  if (!tmp.pref || !tmp.fn || !dsrc || !dou || !dnk) rc = GGS_ERR_HIP;
  else if (hipMemcpy(dsrc, x ? (const void *)x : (const void *)counts, kv * (x ? 8 : 4), hipMemcpyHostToDevice) != hipSuccess) rc = GGS_ERR_HIP;
  else if (guess && hipMemcpy(tmp.pref, guess, pref_bytes, hipMemcpyHostToDevice) != hipSuccess) rc = GGS_ERR_HIP;
  else {
    if (x) launch_column_sum<double, false>(tmp, static_cast<const double *>(dsrc), K, K, dou, nullptr, guess != nullptr, true);
    else launch_column_sum<int32_t, true>(tmp, static_cast<const int32_t *>(dsrc), K, K, dou, dnk, guess != nullptr, true);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out, dou, (size_t)K * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
    else if (pref_out && hipMemcpy(pref_out, tmp.pref, pref_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
    else if (n_k_out && counts && hipMemcpy(n_k_out, dnk, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
  }
  return rc;
}

int ggs_debug_column_sum(int32_t device_id, int32_t V, int32_t K, const double *x, const int32_t *counts, double beta, double *out) {
  return ggs_debug_column_sum_guided(device_id, V, K, x, counts, beta, nullptr, out, nullptr, nullptr);
}

int ggs_debug_min_distances(int32_t device_id, const double *a, int64_t n, const double *b, int64_t m, int64_t len, int32_t element_major, double *min_dist,
                            double *min_sq) {
  if (!a || !min_dist || n <= 0 || len <= 0 || (b && m <= 0) || (element_major && b) || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *da = static_cast<double *>(t.get(sizeof(double) * (size_t)n * (size_t)len));
  auto *db = b ? static_cast<double *>(t.get(sizeof(double) * (size_t)m * (size_t)len)) : da;
  auto *dbits = static_cast<unsigned long long *>(t.get(sizeof(double) * (size_t)n));
  auto *dout = static_cast<double *>(t.get(sizeof(double) * (size_t)n)), *dsq = static_cast<double *>(t.get(sizeof(double) * (size_t)n));
  if (!da || !db || !dbits || !dout || !dsq) return GGS_ERR_HIP;
  if (hipMemcpy(da, a, sizeof(double) * (size_t)n * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (b && hipMemcpy(db, b, sizeof(double) * (size_t)m * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid), dim3(256), 0, nullptr, dbits, n);
  if (element_major) launch_min_topic_dist(nullptr, da, n, n, len, dbits);
  else launch_min_row_dist(nullptr, da, n, db, b ? m : n, len, b == nullptr, dbits);
  hipLaunchKernelGGL(min_dist_finish_kernel, dim3(grid), dim3(256), 0, nullptr, dbits, n, dout, dsq);
  if (hipGetLastError() != hipSuccess || hipMemcpy(min_dist, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  if (min_sq && hipMemcpy(min_sq, dsq, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_summaries(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, double beta, double lambda, int32_t kind, int32_t n_words,
                              int32_t *idx, double *score, double *mass_k, double *rowsum_w, double *total, double *all_scores) {
  if (V <= 0 || K <= 0 || !counts || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  int rc = ts_check_args(nullptr, V, K, beta, kind, n_words, lambda, idx);
  if (rc) return rc;
  TmpDev t;
  const TsPlan q(V, K, n_words);
  const size_t kv = (size_t)V * K;
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dcnt = static_cast<int32_t *>(t.get(kv * 4));
  double *dall = all_scores ? static_cast<double *>(t.get(kv * 8)) : nullptr;
  if (!work || !dcnt || (all_scores && !dall)) return GGS_ERR_HIP;
  if (hipMemcpy(dcnt, counts, kv * 4, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  // GGS_DEBUG_CHAIN=1: both column sums walked element by element
  ts_launch(nullptr, !Knob("GGS_DEBUG_CHAIN").is(1), dcnt, beta, lambda, kind, q, work, true, dall);
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  if (hipGetLastError() != hipSuccess || !fetch(idx, work + q.idx, 4 * (size_t)K * n_words) || !fetch(score, work + q.score, 8 * (size_t)K * n_words) ||
      !fetch(mass_k, work + q.mass, 8 * (size_t)K) || !fetch(rowsum_w, work + q.rowsum, 8 * (size_t)V) || !fetch(total, work + q.total, 8) ||
      !fetch(all_scores, dall, kv * 8))
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_doc_statistics(int32_t device_id, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, const int32_t *z, int32_t V, int32_t K,
                                   const double *alpha, int32_t n_words, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats,
                                   double *clogc_out) {
  if (D < 0 || V <= 0 || K <= 0 || !doc_ptr || !alpha || !idx || !codoc || !doc_stats || !clogc_out || doc_ptr[0] != 0) return GGS_ERR_BAD_ARG;
  for (int64_t d = 0; d < D; ++d)
    if (doc_ptr[d + 1] < doc_ptr[d]) return GGS_ERR_BAD_ARG;
  const int64_t N = doc_ptr[D];
  if (N > 0 && (!tokens || !z)) return GGS_ERR_BAD_ARG;
  for (int64_t t = 0; t < N; ++t)
    if (tokens[t] < 0 || tokens[t] >= V || z[t] < 0 || z[t] >= K) return GGS_ERR_BAD_ARG;
  int rc = td_check_args(nullptr, V, K, n_words, idx);
  if (rc || (rc = td_check_topics(nullptr, K))) return rc;
  if (hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const TdDocPlan q(D, V, K, n_words);
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dptr = static_cast<int64_t *>(t.get(8 * ((size_t)D + 1)));
  auto *dtok = static_cast<int32_t *>(t.get(4 * (size_t)N)), *dz = static_cast<int32_t *>(t.get(4 * (size_t)N));
  auto *dalpha = static_cast<double *>(t.get(8 * (size_t)K));
  if (!work || !dptr || !dtok || !dz || !dalpha) return GGS_ERR_HIP;
  if (hipMemcpy(dptr, doc_ptr, 8 * ((size_t)D + 1), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dalpha, alpha, 8 * (size_t)K, hipMemcpyHostToDevice) != hipSuccess ||
      (N > 0 && (hipMemcpy(dtok, tokens, 4 * (size_t)N, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dz, z, 4 * (size_t)N, hipMemcpyHostToDevice) != hipSuccess)))
    return GGS_ERR_HIP;
  if (td_doc_launch(nullptr, q, work, dptr, dtok, dz, dalpha, td_alpha_sum(alpha, K), idx, clogc_in, nullptr) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemcpy(codoc, work + q.codoc, 4 * (size_t)K * n_words * n_words, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(doc_stats, work + q.stats, 4 * (size_t)K * kTdStats, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(clogc_out, work + q.clogc, 8 * (size_t)K, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_scores(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, double beta, int32_t n_words, const int32_t *idx, const int32_t *codoc,
                           const int32_t *doc_stats, const double *clogc, double *topic_scores, double *word_scores, int32_t *sorted_ids) {
  if (V <= 0 || K <= 0 || !counts || !idx || !codoc || !doc_stats || !clogc || !topic_scores) return GGS_ERR_BAD_ARG;
  int rc = td_check_args(nullptr, V, K, n_words, idx);
  if (rc) return rc;
  if ((int64_t)V * K > ((int64_t)1 << 31) - 256) return GGS_ERR_UNSUPPORTED;
  for (size_t i = 0; i < (size_t)V * K; ++i)
    if (counts[i] < 0) return GGS_ERR_BAD_ARG;
  if (hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const TdScorePlan q(V, K, n_words);
  const size_t kv = (size_t)V * K;
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dcnt = static_cast<int32_t *>(t.get(kv * 4));
  if (!work || !dcnt) return GGS_ERR_HIP;
  if (hipMemcpy(dcnt, counts, kv * 4, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (td_score_launch(nullptr, q, work, dcnt, K, beta, idx, codoc, doc_stats, clogc, word_scores != nullptr, nullptr) != hipSuccess) return GGS_ERR_HIP;
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  if (!fetch(topic_scores, work + q.ts, 8 * (size_t)kTdScoreRows * K) || !fetch(word_scores, work + q.ws, 8 * (size_t)kTdWordRows * K * n_words) ||
      !fetch(sorted_ids, work + q.head, 4 * (size_t)K * n_words))
    return GGS_ERR_HIP;
  return GGS_OK;
}

}  // extern "C"
