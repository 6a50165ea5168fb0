// ggs_host_phi.hpp -- the Phi chain: the Poisson table, the variable-selection chain, the slice draws (phi_slice_*), the steps of
// the Phi phase with an exchange (phi_step_*), the alias build, the count-form sweep heads and launch_phi.
#pragma once
#include "ggs_host_counts.hpp"

namespace {
// scheme=polyaurn: the inverse-CDF tables of the Poisson draws with c < L (ggs_phi_poisson.hpp), row c for lambda = beta + c:
// p_0 = exp(-lambda), p_j = p_{j-1} * lambda / j for j < 2L (PoissonFixedCoeffSampler.java:31-50 keeps the same 2L terms),
// S_j = p_0 + ... + p_j left to right, T_c[j] = S_j / S_{2L-1} and T_c[2L-1] = 1.  fp64, in this order: the tests restate it.
void build_poisson_table(double beta, int32_t L, std::vector<double> &T) {
  const int n = 2 * L;
  T.assign((size_t)L * n, 0.0);
  std::vector<double> S((size_t)n);
  for (int32_t c = 0; c < L; ++c) {
    const double lambda = beta + (double)c;
    double pj = std::exp(-lambda), acc = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j > 0) pj = pj * lambda / (double)j;
      acc += pj;
      S[(size_t)j] = acc;
    }
    for (int j = 0; j < n - 1; ++j) T[(size_t)c * n + j] = S[(size_t)j] / S[(size_t)n - 1];
    T[(size_t)c * n + n - 1] = 1.0;
  }
}

// Topic priors (ggs_set_topic_priors).  The sweep draw is then the CONDITIONAL one (conditional_phi): the masked gamma draw, and
// (g / sum_gamma) * sum_phi in place of the division and its clamp.  sum_phi[k], the index-order sum of the OLD phi row (masked
// cells are +0.0 and leave the running sum as it is), is an exact column sum of phiT over all K topics -- every rank of an exchange
// holds the whole old phiT and sums it for itself -- taken before anything overwrites phiT, unguided, in work space of its own.
// The initial draw runs to its end as ever and is then multiplied by the priors (phi_apply_priors).
bool conditional_phi(const ggs_handle *h, bool initial) { return h->have_priors && !initial; }
// scheme=nzvsspalias: the sweep draw is the variable-selection one (ggs_phi_vs.hpp); the initial draw is pcgs's
bool vs_phi(const ggs_handle *h, bool initial) { return h->scheme == Scheme::nzvsspalias && !initial; }
// ... and what a draw leaves the words' lists to be built from: nothing (the initial Phi), or its drawn cells
void vs_note_draw(ggs_handle *h, bool initial) {
  if (h->scheme == Scheme::nzvsspalias) { h->vs_lists = initial ? ggs_handle::VsLists::empty : ggs_handle::VsLists::drawn; if (initial) h->vs_drawn = false; }
}
// The indicator chain of the topics [k0, k0 + Ks) from their counts cnt [V][cnt_pitch] (tokensPerTopic in n_k) and the Phi now
// in d_phiT: the undrawn cells into d_vs_und (by topic) and d_vs_mask (by word).  Before anything overwrites phiT.
int launch_vs_chain(ggs_handle *h, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, const int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  VsBitsParams bp{};
  bp.cnt = cnt; bp.phiT = h->d_phiT; bp.cz = h->d_vs_cz; bp.pz = h->d_vs_pz;
  bp.cnt_pitch = cnt_pitch; bp.Kp = h->Kp; bp.k0 = k0; bp.Ks = Ks; bp.V = h->V; bp.W = h->vs_W;
  void *bargs[] = {&bp};
  HIP_TRY(h, launch(h, h->plan.vsbits, (int64_t)h->vs_W * ((Ks + 63) / 64), bargs, h->stream));
  VsChainParams cp{};
  cp.cz = h->d_vs_cz; cp.pz = h->d_vs_pz; cp.und = h->d_vs_und; cp.work = h->d_vs_work; cp.n_k = n_k; cp.u = nullptr;
  cp.s_end = h->d_vs_s_end; cp.rounds = h->d_vs_rounds; cp.status = h->d_status; cp.seed = h->seed; cp.iteration = (uint32_t)h->iteration;
  cp.Ks = Ks; cp.k0 = k0; cp.V = h->V; cp.W = h->vs_W; cp.beta = h->beta; cp.odds = h->vs_pi / (1 - h->vs_pi);
  void *cargs[] = {&cp};
  HIP_TRY(h, hipLaunchKernel(h->plan.vschain.fn, dim3((unsigned)Ks), dim3(kVsBlock), cargs, (size_t)h->plan.vschain.lds, h->stream));   // a workgroup per topic
  hipLaunchKernelGGL(vs_mask_kernel, dim3(grid_for((int64_t)h->V * h->vs_pitch, 256)), dim3(256), 0, h->stream, h->d_vs_und, h->vs_W, k0, Ks, h->V, h->vs_pitch,
                     h->d_vs_mask);
  HIP_TRY(h, hipGetLastError());
  h->vs_drawn = true;
  return GGS_OK;
}
int launch_sum_phi(ggs_handle *h) {
  SumCtx c = sum_ctx(h);
  c.pref = h->d_pr_pref; c.fn = h->d_pr_fn;
  launch_column_sum<double, false>(c, h->d_phiT, h->Kp, h->K, h->d_pr_sum_phi, nullptr, false, false);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_apply_priors(ggs_handle *h) {
  hipLaunchKernelGGL(phi_apply_priors_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_phiT, h->d_pr_mask, h->pr_pitch, h->K,
                     h->Kp, h->V, h->d_phiT32, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  h->alias_stale = true;
  return GGS_OK;
}

// Phi draw: initial (K8) or per sweep (K6) for the topics [k0, k0 + Ks) from their corpus-wide counts
// cnt [V][cnt_pitch]; rows into out [V][out_pitch].  In steps, so that the exchange can slot its collectives in:
//   phi_slice_magnitude   the Dirichlet magnitudes (and tokensPerTopic)
//   phi_slice_gamma       the gamma draws of the segments [seg0, seg1) + the segment functions of their column sums
//   phi_slice_total       the walk of those: tot[k] = sum_v gamma, in index order
//   phi_slice_normalise   one GPU: divide in place (with an exchange the division is done by the repack kernel)
int phi_slice_gamma(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                    const double *mag, int32_t seg0, int32_t seg1) {
  if (Ks <= 0 || seg1 <= seg0) return GGS_OK;
  PhiGammaParams gp{};
  gp.n_wk = cnt; gp.mag = mag; gp.phiT = out; gp.status = h->d_status;
  gp.seed = h->seed; gp.iteration = (uint32_t)h->iteration;
  gp.purpose = initial ? GGS_PURPOSE_INIT_PHI : GGS_PURPOSE_PHI;
  gp.K = Ks; gp.Kp = out_pitch; gp.V = h->V; gp.cnt_pitch = cnt_pitch; gp.k0 = k0; gp.beta = h->beta;
  // Dirichlet(int size, double beta): magnitude = V*beta, partition = 1.0/V
  gp.prior_pm = (1.0 / (double)h->V) * ((double)h->V * h->beta);
  gp.initial = initial ? 1 : 0;
  // tiles of one 64-row segment x kc <= kPhiCols topics, the column groups as equal as they come.  A single wave per
  // tile issues an instruction every ~8 cycles, so what makes the draw fast is waves per SIMD: a narrow slice (one rank
  // in eight draws 13 topics) is cut into narrower tiles until there are ~4 waves for each of the chip's SIMDs; the price
  // is a thinner leftover queue per tile (the general rejection loops then run with fewer lanes in use).
  const int64_t want_tiles = (int64_t)h->num_cus * 4 * 4;
  int kc_cap = (int)std::min<int64_t>(kPhiCols, std::max<int64_t>(2, (int64_t)Ks * (seg1 - seg0) / want_tiles));
  if (const char *e = debug_env("GGS_DEBUG_PHICOLS")) kc_cap = std::max(1, std::min(kPhiCols, std::atoi(e)));
  gp.ncg = (Ks + kc_cap - 1) / kc_cap;
  gp.kc = (Ks + gp.ncg - 1) / gp.ncg;
  gp.ncg = (Ks + gp.kc - 1) / gp.kc;
  gp.seg_begin = seg0; gp.seg_end = seg1;
  gp.queue_cap = std::min(kPhiQueue, h->gamma_queue_cap);
  gp.prio = h->xg ? 1 : 0;
  gp.guess = h->exact_sum ? h->d_sum_pref : nullptr; gp.fn = h->d_sum_fn;
  const int64_t tiles = (int64_t)(seg1 - seg0) * gp.ncg;
  // single-wave workgroups; a grid of at most 32 per CU, the rest by striding
  const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)h->num_cus * 32));
  if (conditional_phi(h, initial)) {                   // the masked draw; its sums' guess is still the magnitudes' (any guess will do)
    gp.zero_mask = h->d_pr_mask; gp.mask_pitch = h->pr_pitch;
    hipLaunchKernelGGL(phi_gamma_kernel<true>, grid, dim3(64), 0, h->stream, gp);
  } else if (vs_phi(h, initial)) {                     // the cells the indicator chain left undrawn are masked; shape = beta + n
    gp.zero_mask = h->d_vs_mask; gp.mask_pitch = h->vs_pitch;
    gp.undrawn_negative = h->xg ? 1 : 0;               // the drawn set travels in the gathered gammas' signs of zero (phi_step_c)
    hipLaunchKernelGGL(phi_gamma_vs_kernel, grid, dim3(64), 0, h->stream, gp);
  } else {
    hipLaunchKernelGGL(phi_gamma_kernel<false>, grid, dim3(64), 0, h->stream, gp);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_slice_total(ggs_handle *h, const double *out, int32_t out_pitch, int32_t Ks, double *tot) {
  if (Ks <= 0) return GGS_OK;
  if (h->exact_sum) {
    SumParams sp{};
    sp.src = out; sp.guess = h->d_sum_pref; sp.fn = h->d_sum_fn; sp.out = tot; sp.beta = h->beta; sp.n_k = nullptr;
    sp.pitch = out_pitch; sp.K = Ks; sp.V = h->V; sp.nseg = h->sum_nseg; sp.write_pref = 0;   // the guess stays the magnitudes' running sums
    hipLaunchKernelGGL((sum_walk_kernel<double, false>), dim3((unsigned)Ks), dim3(64), 0, h->stream, sp);
  } else {
    launch_column_sum<double, false>(sum_ctx(h), out, out_pitch, Ks, tot, nullptr, false, false);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
// scheme=polyaurn: the Poisson draws of the rows [seg0, seg1) * 64 (ggs_phi_poisson.hpp) into out, their integer totals
// into d_pa_acc -- zeroed first by the draw's first launch (`first`), so the two halves of an exchange's draw add up
int phi_slice_poisson(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                      int32_t seg0, int32_t seg1, bool first) {
  if (Ks <= 0) return GGS_OK;
  if (first) HIP_TRY(h, hipMemsetAsync(h->d_pa_acc, 0, sizeof(unsigned long long) * kPoissonAccStride * (size_t)Ks, h->stream));
  if (seg1 <= seg0) return GGS_OK;
  PhiPoissonParams pp{};
  pp.cnt = cnt; pp.out = out; pp.table = h->d_pa_table; pp.acc = h->d_pa_acc; pp.status = h->d_status;
  pp.seed = h->seed; pp.iteration = (uint32_t)h->iteration; pp.purpose = initial ? GGS_PURPOSE_INIT_PHI : GGS_PURPOSE_PHI;
  pp.Ks = Ks; pp.out_pitch = out_pitch; pp.cnt_pitch = cnt_pitch; pp.k0 = k0; pp.V = h->V;
  pp.row_begin = seg0 * kSumSegRows; pp.row_end = std::min(h->V, seg1 * kSumSegRows);
  pp.L = h->pa_L; pp.beta = h->beta; pp.t00 = h->pa_t00;
  // tiles sized by the launch's work, as phi_slice_gamma sizes its own: about eight per CU, at least one cell per thread (a
  // narrow slice -- one rank in eight draws 13 topics -- gets many short tiles); two workgroups per CU take them by grid
  // stride, so the totals cost 2 * Ks atomics per workgroup whatever the tile count
  const int64_t rows = pp.row_end - pp.row_begin, cells = rows * Ks;
  const int64_t want = std::max<int64_t>(kPoissonThreads, cells / ((int64_t)h->num_cus * 8));
  pp.rows_per_tile = (int32_t)std::max<int64_t>(1, std::min<int64_t>(rows, (want + Ks - 1) / Ks));
  const int64_t tiles = (rows + pp.rows_per_tile - 1) / pp.rows_per_tile;
  hipLaunchKernelGGL(phi_poisson_kernel, dim3((unsigned)std::min<int64_t>(tiles, (int64_t)h->num_cus * 2)), dim3(kPoissonThreads), (size_t)Ks * 12, h->stream, pp);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_slice_poisson_totals(ggs_handle *h, int32_t Ks, double *tot, int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  hipLaunchKernelGGL(phi_poisson_totals_kernel, dim3((unsigned)((Ks + 255) / 256)), dim3(256), 0, h->stream, h->d_pa_acc, Ks, tot, n_k);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int launch_phi_slice(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                     double *mag, double *tot, int32_t *n_k, double *phi_mean) {
  if (Ks <= 0) return GGS_OK;
  int rc;
  if (poisson_phi(h->scheme)) {   // no magnitudes, no gammas, no exact-sum walk: the totals are integers
    if ((rc = phi_slice_poisson(h, initial, cnt, cnt_pitch, Ks, k0, out, out_pitch, 0, h->sum_nseg, true)) || (rc = phi_slice_poisson_totals(h, Ks, tot, n_k)))
      return rc;
    hipLaunchKernelGGL(phi_normalise_polyaurn_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V,
                       phi_mean, out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
    HIP_TRY(h, hipGetLastError());
    return GGS_OK;
  }
  // (nzvsspalias: the magnitudes are not the draw's, but their pass leaves tokensPerTopic for the chain and a guess for the sums)
  if ((rc = launch_magnitude_on(h, cnt, cnt_pitch, Ks, mag, n_k)) || (vs_phi(h, initial) && (rc = launch_vs_chain(h, cnt, cnt_pitch, Ks, k0, n_k))) ||
      (rc = phi_slice_gamma(h, initial, cnt, cnt_pitch, Ks, k0, out, out_pitch, mag, 0, h->sum_nseg)) || (rc = phi_slice_total(h, out, out_pitch, Ks, tot)))
    return rc;
  if (vs_phi(h, initial))                              // x / sum, a row of sum 0 all +0.0; the reference's loopOverTopics override never adds to the phi mean
    hipLaunchKernelGGL(phi_normalise_polyaurn_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V,
                       static_cast<double *>(nullptr), out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  else if (conditional_phi(h, initial))                     // one GPU: the slice is the whole matrix, sum_phi's columns are its columns
    hipLaunchKernelGGL(phi_normalise_conditional_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, h->d_pr_sum_phi, Ks,
                       out_pitch, h->V, phi_mean, out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  else
    hipLaunchKernelGGL(phi_normalise_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V, phi_mean,
                       out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// The steps of the Phi phase with an exchange attached (ggs_group_sweep issues each for all handles of a one-process
// group, the collective ones inside ncclGroupStart/End; one handle per process runs them back to back):
//   A     reduce-scatter of the counts by topic slice
//   B1    this rank's slice: magnitudes, the gammas of the first half of the vocabulary
//   G0    all-gather of that half on the communication stream -- it runs UNDER step B2
//   B2    the gammas of the second half, then the walk of the column sums (it needs every gamma of the slice)
//   G1    all-gather of the second half with the Ksm column sums behind it, on the main stream, issued behind G0
//   C     repack [nranks][..] -> phiT [V][Kp], dividing by the owner's column sum on the way (the same IEEE division
//         the one-GPU normalise kernel does: bit-identical) (+ the running phi mean)
// What travels is therefore the UNNORMALISED gammas: the division does not have to wait for the slice to be complete
// before the first bytes go out.  Events are recorded by the callers AFTER a grouped step (inside
// ncclGroupStart/End the collectives are only collected, not enqueued).
size_t half0_elems(const ggs_handle *h) { return (size_t)h->v_split * h->Ksm; }
size_t half1_elems(const ggs_handle *h) { return (size_t)(h->V - h->v_split) * h->Ksm + (size_t)h->Ksm; }
int phi_step_a(ggs_handle *h) { return exchange_reduce_scatter(h); }
// behind step A, outside any ncclGroupStart/End: a short vocabulary has no communication-stream step to hide the fill under
int phi_step_a_clear(ggs_handle *h) { return h->seg_split > 0 ? GGS_OK : clear_send_buffer_if_dead(h, h->stream); }
int phi_step_b1(ggs_handle *h, bool initial) {
  int rc;
  if (conditional_phi(h, initial) && (rc = launch_sum_phi(h))) return rc;   // phiT is the old Phi until step C
  if (poisson_phi(h->scheme)) {   // the Poisson draws of the first half (and the totals' zero fill)
    if ((rc = phi_slice_poisson(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, 0, h->seg_split, true))) return rc;
  } else if ((rc = launch_magnitude_on(h, h->d_cnt_own, h->Ksm, h->Ks, h->d_mag_own, h->d_n_k_own))) {
    return rc;
  }
  // nzvsspalias: the indicator chain of the rank's own topics, from their corpus-wide counts and the old Phi (phiT until step C);
  // d_vs_mask then holds the slice's undrawn cells for the two halves' draws
  if (vs_phi(h, initial) && (rc = launch_vs_chain(h, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_n_k_own))) return rc;
  if (h->seg_split > 0) {
    if (!poisson_phi(h->scheme) && (rc = phi_slice_gamma(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->d_mag_own, 0, h->seg_split))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_half_drawn, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, h->ev_half_drawn, 0));
  }
  return GGS_OK;
}
int phi_step_g0(ggs_handle *h) {
  if (h->seg_split <= 0) return GGS_OK;
  return xcall(h, h->xg->ops.all_gather_f64(h->xg->ops.ctx, h->d_phi_own, h->d_phi_all0, (int64_t)half0_elems(h), h->comm_stream), "all_gather_f64");
}
int phi_step_b2(ggs_handle *h, bool initial) {
  int rc;
  if (h->seg_split > 0) {
    // behind the first all-gather on the communication stream (which waited for the slice's first half, hence for the
    // reduce-scatter before it): the send buffer's zero fill, deferred by phi_step_a
    if ((rc = clear_send_buffer_if_dead(h, h->comm_stream))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_half_gathered, h->comm_stream));
  }
  if (poisson_phi(h->scheme)) {   // the second half, then the integer totals into the slot behind the slice
    if ((rc = phi_slice_poisson(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->seg_split, h->sum_nseg, false))) return rc;
    return phi_slice_poisson_totals(h, h->Ks, h->d_phi_own + (size_t)h->V * h->Ksm, h->d_n_k_own);
  }
  if ((rc = phi_slice_gamma(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->d_mag_own, h->seg_split, h->sum_nseg))) return rc;
  return phi_slice_total(h, h->d_phi_own, h->Ksm, h->Ks, h->d_phi_own + (size_t)h->V * h->Ksm);
}
int phi_step_g1(ggs_handle *h) {
  return xcall(h, h->xg->ops.all_gather_f64(h->xg->ops.ctx, h->d_phi_own + half0_elems(h), h->d_phi_all1, (int64_t)half1_elems(h), h->stream), "all_gather_f64");
}
int phi_join_halves(ggs_handle *h) {                   // the main stream goes on only when the first half has arrived too
  if (h->seg_split > 0) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_half_gathered, 0));
  return GGS_OK;
}
int phi_step_c(ggs_handle *h, bool initial, bool accumulate_mean) {
  PhiRepackParams rp{};
  rp.all0 = h->d_phi_all0; rp.all1 = h->d_phi_all1; rp.krank = h->d_krank; rp.kcol = h->d_kcol; rp.phiT = h->d_phiT;
  rp.phi_mean = accumulate_mean ? h->d_phi_mean : nullptr;
  rp.c0 = (int64_t)half0_elems(h); rp.c1 = (int64_t)half1_elems(h); rp.K = h->K; rp.Kp = h->Kp; rp.V = h->V; rp.Ksm = h->Ksm; rp.v_split = h->v_split;
  rp.phiT32 = h->d_phiT32; rp.Kp32 = h->plan.Kp32; rp.sum_phi = h->d_pr_sum_phi;
  if (vs_phi(h, initial)) {                            // every topic's undrawn cells from the signs of zero, then the repack that clears them
    rp.phi_mean = nullptr;                             // the reference's loopOverTopics override never adds to the phi mean
    hipLaunchKernelGGL(vs_mask_gathered_kernel, dim3(grid_for((int64_t)h->V * h->vs_pitch, 256)), dim3(256), 0, h->stream, rp, h->d_vs_mask, h->vs_pitch);
    hipLaunchKernelGGL(phi_repack_vs_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  } else if (poisson_phi(h->scheme)) hipLaunchKernelGGL(phi_repack_polyaurn_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  else if (conditional_phi(h, initial)) hipLaunchKernelGGL(phi_repack_conditional_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  else hipLaunchKernelGGL(phi_repack_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  HIP_TRY(h, hipGetLastError());
  h->have_phi = true;
  h->alias_stale = true;
  vs_note_draw(h, initial);
  if (h->have_priors && initial) return phi_apply_priors(h);
  return GGS_OK;
}

// scheme=spalias: the alias tables of the Phi now in d_phiT (ggs_alias.hpp), on the handle's stream.  Called wherever Phi
// changes (the draws below, ggs_set_phi), inside the span ggs_get_timings counts as phi_ms.  With an exchange every rank
// holds the whole Phi after the all-gather and builds all V words for itself: what a rank's shard contains changes
// with the corpus, the tables' layout does not.
int launch_alias_build(ggs_handle *h) {
  if (!has_alias(h->scheme)) return GGS_OK;
  AliasParams ap{};
  ap.phiT = h->d_phiT; ap.alpha = h->d_alpha; ap.ps = h->d_alias_ps; ap.a = h->d_alias_a; ap.type_norm = h->d_alias_tn;
  ap.V = h->V; ap.K = h->K; ap.Kp = h->Kp; ap.wpb = h->plan.alias_wpb;
  void *args[] = {&ap};
  HIP_TRY(h, launch(h, h->plan.alias, ((int64_t)h->V + ap.wpb - 1) / ap.wpb, args, h->stream));
  if (h->scheme == Scheme::nzvsspalias && h->vs_lists == ggs_handle::VsLists::empty) {   // the reference fills no list before its first samplePhi
    HIP_TRY(h, hipMemsetAsync(h->d_nw, 0, (size_t)h->V * sizeof(int32_t), h->stream));
  } else if (doubly_sparse(h->scheme)) {               // the words' lists of non-zero topics, of the same Phi (nzvsspalias after a sweep: of its drawn cells)
    const bool from_mask = h->vs_lists == ggs_handle::VsLists::drawn;   // nzvsspalias alone has them (vs_note_draw)
    WordListParams wp{};
    wp.phiT = h->d_phiT; wp.nzw = h->d_nzw; wp.nw = h->d_nw; wp.V = h->V; wp.K = h->K; wp.Kp = h->Kp;
    wp.zero_mask = h->d_vs_mask; wp.mask_pitch = h->vs_pitch;
    void *wargs[] = {&wp};
    HIP_TRY(h, launch(h, from_mask ? h->plan.wordmask : h->plan.wordlist, h->V, wargs, h->stream));
  }
  h->alias_stale = false;
  return GGS_OK;
}

// The head of a count-form scheme's z step (launch_sweep_head), on the handle's stream: what the step conditions on, of the
// corpus-wide counts now in d_n_wk / d_n_k; also run for the getters.  With an exchange every rank holds the gathered counts and
// builds all for itself.  scheme=lightcollapsed: the words' lists and tables (count_alias_build_kernel)
int launch_count_alias_build(ggs_handle *h) {
  CountAliasParams cp{};
  cp.n_wk = h->d_n_wk; cp.n_k = h->d_n_k; cp.ps = h->d_alias_ps; cp.a = h->d_alias_a; cp.type_norm = h->d_alias_tn;
  cp.nzw = h->d_nzw; cp.nw = h->d_nw; cp.tpt = h->d_tpt; cp.beta_sum = h->beta_sum;
  cp.V = h->V; cp.K = h->K; cp.wpb = h->plan.alias_wpb;
  void *args[] = {&cp};
  HIP_TRY(h, launch(h, h->plan.countalias, ((int64_t)h->V + cp.wpb - 1) / cp.wpb, args, h->stream));
  return GGS_OK;
}

// scheme=adlda: den0, S0 and the words' lists
int launch_adlda_head(ggs_handle *h) {
  AdldaHeadParams hp{};
  hp.n_k = h->d_n_k; hp.alpha = h->d_alpha; hp.den0 = h->d_ad_den0; hp.s0 = h->d_ad_s0; hp.beta = h->beta; hp.beta_sum = h->beta_sum; hp.K = h->K;
  void *hargs[] = {&hp};
  HIP_TRY(h, launch(h, h->plan.adhead, 1, hargs, h->stream));
  WordListParams wp{};
  wp.counts = h->d_n_wk; wp.nzw = h->d_nzw; wp.nw = h->d_nw; wp.V = h->V; wp.K = h->K; wp.Kp = h->Kp;
  void *wargs[] = {&wp};
  HIP_TRY(h, launch(h, h->plan.adlists, h->V, wargs, h->stream));
  return GGS_OK;
}

int launch_sweep_head(ggs_handle *h) {
  const int rc = launch_magnitude(h);                  // the counts gathered, tokensPerTopic in step with them
  if (rc) return rc;
  if (count_tables(h->scheme)) return launch_count_alias_build(h);   // lightpcldaw2 too: Phi is not touched
  if (h->scheme == Scheme::adlda) return launch_adlda_head(h);
  // collapsed: the ratios (beta + n_wk)/(betaSum + n_k) into phiT, for the pcgs loop over them
  hipLaunchKernelGGL(psi_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_n_wk, h->d_n_k, h->beta, h->beta_sum, h->d_phiT,
                     h->K, h->Kp, h->V);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// Phi draw: initial (K8) or per sweep (K6).  One GPU: the whole matrix in place (and tokensPerTopic refreshed);
// with an exchange: steps A, B, C above.
int launch_phi(ggs_handle *h, bool initial, bool accumulate_mean, Events *E = nullptr) {
  int rc;
  if (h->xg) {
    if ((rc = phi_step_a(h)) || (rc = phi_step_a_clear(h))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[0], h->stream));
    if ((rc = phi_step_b1(h, initial)) || (rc = phi_step_g0(h)) || (rc = phi_step_b2(h, initial))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[1], h->stream));
    // the second all-gather is issued only behind the first: no two collectives of one communicator are ever in flight
    // on different streams at once (they could not share the links anyway), whatever the transport does about that itself
    if ((rc = phi_join_halves(h)) || (rc = phi_step_g1(h))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[2], h->stream));
    if ((rc = phi_step_c(h, initial, accumulate_mean))) return rc;
    return launch_alias_build(h);
  }
  if (conditional_phi(h, initial) && (rc = launch_sum_phi(h))) return rc;   // before the draw overwrites phiT
  if ((rc = launch_phi_slice(h, initial, h->d_n_wk, h->K, h->K, 0, h->d_phiT, h->Kp, h->d_mag, h->d_tot, h->d_n_k, accumulate_mean ? h->d_phi_mean : nullptr)))
    return rc;
  h->n_k_valid = true;
  h->have_phi = true;
  vs_note_draw(h, initial);
  if (h->have_priors && initial && (rc = phi_apply_priors(h))) return rc;
  return launch_alias_build(h);
}
}  // namespace
