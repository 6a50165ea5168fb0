// ggs_host_exchange.hpp -- attaching an exchange (its buffers, column map, streams and events: setup_exchange) and the one-process
// group: a collective step for every handle (group_collective), the grouped Phi phase and the grouped gather of the counts.
#pragma once
#include "ggs_host_sweep.hpp"

namespace {
// An Exchange that never got attached: its communicator goes with it when the library created it.
void exchange_free(Exchange *x) {
  if (!x) return;
  if (x->own_comm && x->comm && x->api) (void)x->api->CommDestroy(x->comm);
  delete x;
}
// what every attach call checks BEFORE it creates anything (ncclCommInitRank is a blocking collective)
int exchange_precheck(ggs_handle *h, int32_t rank, int32_t nranks) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (h->xg) return set_err(h, GGS_ERR_STATE, "an exchange is already attached");
  if (h->have_corpus) return set_err(h, GGS_ERR_STATE, "attach the exchange before ggs_set_corpus");
  if (nranks < 1 || rank < 0 || rank >= nranks) return set_err(h, GGS_ERR_BAD_ARG, "rank outside [0, nranks)");
  return bind_device(h);
}

// Buffers and the column map of an attached exchange; the handle moves to a stream of its own.  Takes ownership of x.
int setup_exchange(ggs_handle *h, Exchange *x) {
  int rc = exchange_precheck(h, x->rank, x->nranks);
  if (rc) { exchange_free(x); return rc; }
  const std::vector<int32_t> sl = topic_slices(h->K, x->nranks);
  h->xg = x;
  h->k0 = sl[(size_t)x->rank]; h->Ks = sl[(size_t)x->rank + 1] - h->k0; h->Ksm = (h->K + x->nranks - 1) / x->nranks;
  {
    auto magic = [](uint32_t d) { return d > 1 ? (uint32_t)((0x100000000ull + d - 1) / d) : 0u; };   // udiv_magic (ggs_kernels.hpp)
    h->smap.size = h->K / x->nranks; h->smap.rem = h->K % x->nranks; h->smap.ksm = h->Ksm;
    h->smap.m_size = magic((uint32_t)std::max(h->smap.size, 1)); h->smap.m_size1 = magic((uint32_t)h->smap.size + 1);
    h->smap.rank_stride = (int64_t)h->V * h->Ksm;
    if (const char *e = debug_env("GGS_DEBUG_ZCOUNTS")) { h->z_counts = std::atoi(e) != 0; h->z_counts_forced = std::atoi(e) == 2; }
    if (const char *e = debug_env("GGS_DEBUG_TIMING_EVERY")) h->detail_every = std::max(1, std::atoi(e));
    if (const char *e = debug_env("GGS_DEBUG_COUNT_EXCHANGE")) h->count_mode = std::max(0, std::min(2, std::atoi(e)));
  }
  std::vector<int64_t> koff((size_t)h->K);
  for (int32_t r = 0; r < x->nranks; ++r)
    for (int32_t k = sl[(size_t)r]; k < sl[(size_t)r + 1]; ++k) koff[(size_t)k] = (int64_t)r * h->V * h->Ksm + (k - sl[(size_t)r]);
  std::vector<int32_t> krank((size_t)h->K), kcol((size_t)h->K);
  for (int32_t r = 0; r < x->nranks; ++r)
    for (int32_t k = sl[(size_t)r]; k < sl[(size_t)r + 1]; ++k) { krank[(size_t)k] = r; kcol[(size_t)k] = k - sl[(size_t)r]; }
  // the all-gather of the gammas in two halves of the vocabulary (whole 64-row segments: the draw's tiles); a short
  // vocabulary goes in one
  h->seg_split = h->sum_nseg >= 16 ? h->sum_nseg / 2 : 0;
  if (const char *e = debug_env("GGS_DEBUG_AGSPLIT")) h->seg_split = std::max(0, std::min(h->sum_nseg - 1, std::atoi(e)));
  h->v_split = h->seg_split * kSumSegRows;
  const size_t slice = (size_t)h->V * h->Ksm, all = slice * (size_t)x->nranks;
  auto fail = [&](int code) {                        // a half-built exchange must not stay attached
    void *bufs[] = {h->d_koff, h->d_krank, h->d_kcol, h->d_cnt_send, h->d_cnt_own, h->d_phi_own, h->d_phi_all0, h->d_phi_all1, h->d_mag_own, h->d_n_k_own};
    for (void *b : bufs) if (b) (void)hipFree(b);
    h->d_koff = nullptr; h->d_krank = h->d_kcol = nullptr; h->d_cnt_send = h->d_cnt_own = nullptr; h->d_phi_own = h->d_phi_all0 = h->d_phi_all1 = nullptr;
    h->d_mag_own = nullptr; h->d_n_k_own = nullptr;
    h->xg = nullptr; h->Ks = h->Ksm = h->K; h->k0 = 0;
    exchange_free(x);
    return code;
  };
  if ((rc = upload(h, &h->d_koff, koff)) || (rc = upload(h, &h->d_krank, krank)) || (rc = upload(h, &h->d_kcol, kcol)) ||
      (rc = dev_alloc_zeroed(h, &h->d_cnt_send, all)) || (rc = dev_alloc_zeroed(h, &h->d_cnt_own, slice)) || (rc = dev_alloc_zeroed(h, &h->d_phi_own, slice + (size_t)h->Ksm)) ||
      (rc = dev_alloc_zeroed(h, &h->d_phi_all0, std::max<size_t>(half0_elems(h) * (size_t)x->nranks, 1))) ||
      (rc = dev_alloc_zeroed(h, &h->d_phi_all1, half1_elems(h) * (size_t)x->nranks)) ||
      (rc = dev_alloc(h, &h->d_mag_own, (size_t)h->Ksm)) || (rc = dev_alloc(h, &h->d_n_k_own, (size_t)h->Ksm)))
    return fail(rc);
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  if (make_stream(h, &h->comm_stream, hi) || make_event(h, &h->ev_half_drawn, hipEventDisableTiming) || make_event(h, &h->ev_half_gathered, hipEventDisableTiming))
    return fail(set_err(h, GGS_ERR_HIP, "exchange: communication stream / events"));
  if (!h->stream) {
    // Collectives are ordered by THIS stream alone: not the legacy default stream, whose implicit synchronisation with
    // other libraries' blocking streams is exactly the convention not to rely on.  HIGH priority: measured with RCCL
    // and a torch process group in the process, a normal-priority stream shares its hardware queue with theirs and the
    // sweep's phases stretch (one rank: 2.59 ms per sweep against 1.93 on a high-priority stream or the null stream).
    if (!(debug_env("GGS_DEBUG_OWN_STREAM") && std::atoi(debug_env("GGS_DEBUG_OWN_STREAM")) == 0)) {   // 0: experiments
      if (make_stream(h, &h->own_stream, hi)) return GGS_ERR_HIP;
      h->stream = h->own_stream;
    }
  }
  HIP_TRY(h, hipDeviceSynchronize());
  h->counts_global = false; h->cnt_own_valid = false; h->n_k_valid = false;
  h->cnt_send_zeroed = true;                           // the memset above
  return GGS_OK;
}

Exchange *new_rccl_exchange(ggs_handle *h, int32_t rank, int32_t nranks, int *rc) {
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) { *rc = set_err(h, GGS_ERR_UNSUPPORTED, err); return nullptr; }
  auto *x = new (std::nothrow) Exchange();
  if (!x) { *rc = GGS_ERR_HIP; return nullptr; }
  x->rank = rank; x->nranks = nranks; x->api = api;
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops); x->ops.ctx = x;
  x->ops.reduce_scatter_i32 = xops::rccl_reduce_scatter_i32;
  x->ops.all_gather_f64 = xops::rccl_all_gather_f64;
  x->ops.all_gather_i32 = xops::rccl_all_gather_i32;
  x->ops.all_to_all_v_i32 = (api->Send && api->Recv) ? xops::rccl_all_to_all_v_i32 : nullptr;
  *rc = GGS_OK;
  return x;
}

// a collective step for every handle of the group: inside ncclGroupStart/End for RCCL; an adopted group (the caller's
// transport) simply gets the calls one after the other, rank 0 first
template <typename Step>
int group_collective(ggs_handle **hs, int32_t n, Step step) {
  RcclApi *api = hs[0]->xg->api;
  int r = GGS_OK;
  if (api) api->GroupStart();
  for (int32_t i = 0; i < n && !r; ++i)
    if (!(r = bind_device(hs[i]))) r = step(hs[i]);
  if (api && api->GroupEnd() != ncclSuccess && !r) r = set_err(hs[0], GGS_ERR_HIP, "ncclGroupEnd failed");
  return r;
}

bool is_group(ggs_handle **hs, int32_t n) {
  if (!hs || n < 1 || !hs[0] || (int32_t)hs[0]->group.size() != n) return false;
  for (int32_t i = 0; i < n; ++i)
    if (hs[i] != hs[0]->group[(size_t)i] || !hs[i]->xg || hs[i]->xg->api != hs[0]->xg->api) return false;   // all RCCL, or all the caller's transport
  return true;
}

// the Phi phase for every handle of the group: each collective step for all devices inside ncclGroupStart/End
int group_phi(ggs_handle **hs, int32_t n, bool initial, bool in_sweep) {
  std::vector<char> acc((size_t)n, 0);
  int rc = GGS_OK;
  for (int32_t i = 0; i < n && !rc; ++i) {
    ggs_handle *h = hs[i];
    if ((rc = bind_device(h))) break;
    if (in_sweep) {
      Events &E = h->evs[h->ev_head];
      if (!E.light && hipEventRecord(E.e[4], h->stream) != hipSuccess) { rc = set_err(h, GGS_ERR_HIP, "hipEventRecord"); break; }
      E.exchanged = true; E.e4_is_e3 = false;
      acc[(size_t)i] = (h->flags & GGS_FLAG_SAVE_PHI_MEAN) && sample_phi_this_iteration(h);
    }
  }
  if (rc) return rc;
  auto timed = [&](ggs_handle *h) -> Events * { return (in_sweep && !h->evs[h->ev_head].light) ? &h->evs[h->ev_head] : nullptr; };   // a light sweep records no phase events
  auto grouped = [&](auto step) { return group_collective(hs, n, [&](ggs_handle *h) { return step(h, timed(h)); }); };
  // a step for every handle; events are recorded AFTER a grouped step: inside ncclGroupStart/End the collectives are
  // only collected, and an event recorded there would land on the stream before them
  auto each = [&](auto step) {
    int r = GGS_OK;
    for (int32_t i = 0; i < n && !r; ++i)
      if (!(r = bind_device(hs[i]))) r = step(hs[i], timed(hs[i]));
    return r;
  };
  auto record = [](ggs_handle *h, hipEvent_t ev) { return hipEventRecord(ev, h->stream) == hipSuccess ? GGS_OK : set_err(h, GGS_ERR_HIP, "hipEventRecord"); };
  if ((rc = grouped([](ggs_handle *h, Events *) { return phi_step_a(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { int r = phi_step_a_clear(h); if (!r && E) r = record(h, E->x[0]); return r ? r : phi_step_b1(h, initial); })) ||
      (rc = grouped([](ggs_handle *h, Events *) { return phi_step_g0(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { int r = phi_step_b2(h, initial); if (!r && E) r = record(h, E->x[1]); return r ? r : phi_join_halves(h); })) ||
      (rc = grouped([](ggs_handle *h, Events *) { return phi_step_g1(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { return E ? record(h, E->x[2]) : GGS_OK; })))
    return rc;
  for (int32_t i = 0; i < n; ++i) {
    ggs_handle *h = hs[i];
    if ((rc = bind_device(h)) || (rc = phi_step_c(h, initial, acc[(size_t)i] != 0)) || (rc = launch_alias_build(h))) return rc;
    if (in_sweep) {
      HIP_TRY(h, hipEventRecord(h->evs[h->ev_head].e[5], h->stream));
      if (acc[(size_t)i]) h->n_sampled_phi++;
      h->ev_pending += 1;
    }
  }
  return GGS_OK;
}

// corpus-wide counts on every handle of the group: the two collectives of ensure_global_counts, each grouped
int group_gather_counts(ggs_handle **hs, int32_t n) {
  int rc;
  if ((rc = group_collective(hs, n, [](ggs_handle *h) { return h->counts_global ? GGS_OK : exchange_reduce_scatter(h); }))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = bind_device(hs[i])) || (rc = clear_send_buffer_if_dead(hs[i], hs[i]->stream))) return rc;
  if ((rc = group_collective(hs, n, [](ggs_handle *h) { return h->counts_global ? GGS_OK : gather_counts_step_gather(h); }))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if (!hs[i]->counts_global && ((rc = bind_device(hs[i])) || (rc = gather_counts_step_unslice(hs[i])))) return rc;
  return GGS_OK;
}
}  // namespace
