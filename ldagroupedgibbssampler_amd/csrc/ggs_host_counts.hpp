// ggs_host_counts.hpp -- the count chain: the (word, z) histogram and its sparse form, the exact column sums and the magnitudes,
// the count exchange (reduce-scatter, the send buffer's clears, the gather of the slices) and ensure_global_counts.
#pragma once
#include "ggs_host_state.hpp"

namespace {
// after a host upload of z (document order): refresh the word-sorted copy the count kernel reads
int launch_permute_z(ggs_handle *h) {
  if (h->N > 0)
    hipLaunchKernelGGL(permute_z_kernel, dim3(grid_for(h->N, 256)), dim3(256), 0, h->stream, h->d_perm, h->d_z, h->d_zw, h->N);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// Does the next count exchange of this handle ship (cell, count) pairs?  Every input of the rule is the same on every rank.
bool use_sparse(const ggs_handle *h) {
  if (!h->xg || h->in_group || !h->xg->ops.all_to_all_v_i32 || h->xg->nranks > kSparseMaxRanks) return false;
  if ((int64_t)h->V * h->Ksm >= ((int64_t)1 << 31)) return false;       // a cell index is an int32
  if (h->count_mode == 1) return false;
  if (h->count_mode == 2) return true;
  if (h->global_tokens < 0) return false;              // the rule needs a figure all ranks share
  const int64_t cells = (int64_t)h->V * h->K;
  return cells >= ((int64_t)1 << 26) && h->global_tokens / h->xg->nranks < cells / 2;
}
SparseCountParams sparse_params(const ggs_handle *h) {
  SparseCountParams sp{};
  sp.zw = h->d_zw; sp.seg_word = h->d_seg_word; sp.seg_begin = h->d_seg_begin; sp.K = h->K; sp.num_segs = (int32_t)h->S; sp.nranks = h->xg->nranks;
  sp.ksm = h->Ksm; sp.rem = h->smap.rem; sp.size = h->smap.size; sp.m_size = h->smap.m_size; sp.m_size1 = h->smap.m_size1;
  return sp;
}
// pass A of the sparse form: how many pairs this rank has for every destination
int launch_sparse_count(ggs_handle *h) {
  const int n = h->xg->nranks;
  int rc;
  if (!h->d_sp_count && ((rc = dev_alloc(h, &h->d_sp_count, (size_t)n)) || (rc = dev_alloc(h, &h->d_sp_cnt32, (size_t)n)) || (rc = dev_alloc(h, &h->d_sp_all, (size_t)n * n)))) return rc;
  const int64_t wgs = (h->S + kSparseSegsPerBlock - 1) / kSparseSegsPerBlock;
  if (wgs != h->sp_wgs || !h->d_sp_wg_count) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((rc = dev_alloc(h, &h->d_sp_wg_count, (size_t)wgs * n)) || (rc = dev_alloc(h, &h->d_sp_wg_off, (size_t)wgs * n))) return rc;
    h->sp_wgs = wgs;
  }
  if (wgs > 0) {
    SparseCountParams sp = sparse_params(h);
    sp.wg_count = h->d_sp_wg_count;
    hipLaunchKernelGGL(sparse_count_kernel<false>, dim3((unsigned)wgs), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, sp);
    hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)n), dim3(256), 0, h->stream, h->d_sp_wg_count, (int32_t)wgs, n, h->d_sp_wg_off, h->d_sp_count);
    HIP_TRY(h, hipGetLastError());
  } else {
    HIP_TRY(h, hipMemsetAsync(h->d_sp_count, 0, sizeof(int64_t) * (size_t)n, h->stream));
  }
  h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false;
  h->counted_sparse = true;
  return GGS_OK;
}

// n_wk = histogram of (word, z) over this handle's tokens (UPLDA:471-474 summed over the corpus).  With an exchange the
// histogram goes straight into the slice-major send buffer of the count reduce-scatter.
int launch_count_rebuild(ggs_handle *h) {
  if (use_sparse(h)) return launch_sparse_count(h);     // no dense buffer: the pairs are emitted inside the exchange step, once their number is known
  h->counted_sparse = false;
  const size_t cells = h->xg ? (size_t)h->xg->nranks * h->V * h->Ksm : (size_t)h->K * h->V;
  int32_t *dst = h->xg ? h->d_cnt_send : h->d_n_wk;
  if (!(h->xg && h->cnt_send_zeroed)) HIP_TRY(h, hipMemsetAsync(dst, 0, cells * sizeof(int32_t), h->stream));
  h->cnt_send_zeroed = false;
  if (h->S > 0) {
    CountParams cp{};
    cp.zw = h->d_zw; cp.seg_word = h->d_seg_word; cp.seg_begin = h->d_seg_begin; cp.n_wk = dst; cp.K = h->K; cp.num_segs = (int32_t)h->S;
    cp.koff = h->xg ? h->d_koff : nullptr; cp.row_stride = h->xg ? h->Ksm : h->K;
    cp.seg_end = nullptr; cp.segs_per_block = kCountSegsPerBlock;
    hipLaunchKernelGGL(count_sorted_kernel, dim3((unsigned)((h->S + kCountSegsPerBlock - 1) / kCountSegsPerBlock)), dim3(256), (size_t)h->K * sizeof(int32_t),
                       h->stream, cp);
  }
  HIP_TRY(h, hipGetLastError());
  h->n_k_valid = false;
  if (h->xg) { h->counts_global = false; h->cnt_own_valid = false; }
  return GGS_OK;
}
// The hot words' share of the send buffer, behind a z step whose kernels counted the cold tokens themselves.
int launch_count_hot(ggs_handle *h) {
  if (h->HS > 0) {
    CountParams cp{};
    cp.zw = h->d_zw; cp.seg_word = h->d_hseg_word; cp.seg_begin = h->d_hseg_begin; cp.seg_end = h->d_hseg_end; cp.n_wk = h->d_cnt_send; cp.K = h->K;
    cp.num_segs = (int32_t)h->HS; cp.koff = h->d_koff; cp.row_stride = h->Ksm; cp.segs_per_block = 1;
    hipLaunchKernelGGL(count_sorted_kernel, dim3((unsigned)h->HS), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, cp);
    HIP_TRY(h, hipGetLastError());
  }
  h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false;
  return GGS_OK;
}

// out[k] = sum over v, in index order, of src[v][k] (MAGNITUDE: of beta + src[v][k]) for the Ks columns of a topic
// slice -- the exact parallel formulation of ggs_exact_sum.hpp, or the element-by-element chain it replaces.
// `guided`: c.pref already holds a guess of the running sums for these columns (the exact values of the last
// magnitude sum over the same buffer); otherwise two extra launches make one.  The walk leaves the exact running
// sums there (write_pref): the next sweep's guess, and this sweep's guess for the sum of the gammas.
// What it reads: sum_ctx(h) for a handle (a caller with work space of its own replaces pref / fn), or filled by hand where there is none.
struct SumCtx { hipStream_t stream; int32_t V; double beta; bool exact_sum; int32_t sum_nseg; double *pref, *fn; };
SumCtx sum_ctx(const ggs_handle *h) { return {h->stream, h->V, h->beta, h->exact_sum, h->sum_nseg, h->d_sum_pref, h->d_sum_fn}; }
template <typename T, bool MAGNITUDE>
void launch_column_sum(const SumCtx &c, const T *src, int32_t pitch, int32_t Ks, double *out, int32_t *n_k, bool guided, bool write_pref) {
  if (Ks <= 0) return;
  if (!c.exact_sum) {
    hipLaunchKernelGGL((column_chain_kernel<T, MAGNITUDE>), dim3((Ks + 7) / 8), dim3(256), 0, c.stream, src, pitch, Ks, c.V, c.beta, out);
    return;
  }
  SumParams sp{};
  sp.src = src; sp.guess = c.pref; sp.fn = c.fn; sp.out = out; sp.beta = c.beta; sp.n_k = n_k;
  sp.pitch = pitch; sp.K = Ks; sp.V = c.V; sp.nseg = c.sum_nseg; sp.write_pref = write_pref ? 1 : 0;
  const dim3 rows((unsigned)c.sum_nseg, (unsigned)((Ks + kSumBlock - 1) / kSumBlock));
  if (!guided) {
    hipLaunchKernelGGL((sum_seg_kernel<T, MAGNITUDE>), rows, dim3(kSumBlock), 0, c.stream, sp);
    hipLaunchKernelGGL(sum_prefix_kernel, dim3((unsigned)Ks), dim3(64), 0, c.stream, sp);
  }
  hipLaunchKernelGGL((sum_segfn_kernel<T, MAGNITUDE>), dim3((unsigned)c.sum_nseg, (unsigned)((Ks + kSegFnCols - 1) / kSegFnCols)), dim3(256), 0, c.stream, sp);
  hipLaunchKernelGGL((sum_walk_kernel<T, MAGNITUDE>), dim3((unsigned)Ks), dim3(64), 0, c.stream, sp);
}

// magnitude_k = sum_v (beta + n_kv) and tokensPerTopic for the Ks columns of `cnt`
int launch_magnitude_on(ggs_handle *h, const int32_t *cnt, int32_t pitch, int32_t Ks, double *mag, int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  if (h->exact_sum) {
    // the guess of the guided form is only a guess for the SAME columns of the SAME buffer
    const bool guided = h->sum_guided && h->guess_src == cnt && h->guess_cols == Ks;
    launch_column_sum<int32_t, true>(sum_ctx(h), cnt, pitch, Ks, mag, n_k, guided, true);   // tokensPerTopic falls out of the segment pass
    h->guess_src = cnt; h->guess_cols = Ks;
  } else {
    HIP_TRY(h, hipMemsetAsync(n_k, 0, sizeof(int32_t) * (size_t)Ks, h->stream));
    launch_column_sum<int32_t, true>(sum_ctx(h), cnt, pitch, Ks, mag, nullptr, false, false);
    hipLaunchKernelGGL(topic_totals_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 16)), dim3(256), (size_t)Ks * sizeof(int32_t), h->stream, cnt,
                       Ks, pitch, h->V, n_k);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// One collective of the attached exchange, on the handle's stream.
int xcall(ggs_handle *h, int rc, const char *what) {
  if (!rc) return GGS_OK;
  return set_err(h, GGS_ERR_HIP, std::string("exchange ") + what + " failed" + (h->xg->err.empty() ? "" : ": " + h->xg->err));
}
// Behind the reduce-scatter the send buffer is dead until the next z step fills it again (the z kernels add their cells
// into it, or count_sorted_kernel does): it is cleared right here, off the z step's critical path -- on the communication
// stream when the Phi phase is about to use it anyway (`defer_clear`: phi_step_b2 enqueues the fill behind the first
// all-gather, and the event the main stream waits for before the second one covers it), otherwise on the handle's stream.
int clear_send_buffer(ggs_handle *h, hipStream_t on) {
  HIP_TRY(h, hipMemsetAsync(h->d_cnt_send, 0, (size_t)h->xg->nranks * h->V * h->Ksm * sizeof(int32_t), on));
  h->cnt_send_zeroed = true;
  return GGS_OK;
}
// NOT cleared in here: inside ncclGroupStart/End a collective is only collected, and a fill enqueued beside it would land
// on the stream BEFORE it.  The callers clear once the collective is really enqueued (clear_send_buffer_if_dead); a
// buffer nobody cleared is cleared by the next z step itself.
// The sparse form of the count exchange: pair counts to the host, all-gathered; the pairs emitted at their offsets;
// all-to-all of the variable blocks; scatter-add into the zeroed slice.  Two host round trips (the sizes of what travels
// are only known on the device) -- this form is for exchanges whose dense buffer is hundreds of megabytes.
int sparse_exchange(ggs_handle *h) {
  const int n = h->xg->nranks, me = h->xg->rank;
  std::vector<int64_t> mine((size_t)n), soff((size_t)n), scnt((size_t)n), roff((size_t)n), rcnt((size_t)n);
  std::vector<int32_t> mine32((size_t)n), all((size_t)n * n);
  HIP_TRY(h, hipMemcpyAsync(mine.data(), h->d_sp_count, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  int64_t total = 0;
  for (int r = 0; r < n; ++r) {
    if (mine[(size_t)r] > INT32_MAX / 2) return set_err(h, GGS_ERR_UNSUPPORTED, "sparse count exchange: more than 2^30 pairs for one destination");
    mine32[(size_t)r] = (int32_t)mine[(size_t)r];
    soff[(size_t)r] = 2 * total; scnt[(size_t)r] = 2 * mine[(size_t)r];
    total += mine[(size_t)r];
  }
  h->sp_pairs_last = total;
  HIP_TRY(h, hipMemcpyAsync(h->d_sp_cnt32, mine32.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  int rc = xcall(h, h->xg->ops.all_gather_i32(h->xg->ops.ctx, h->d_sp_cnt32, h->d_sp_all, n, h->stream), "all_gather_i32 (pair counts)");
  if (rc) return rc;
  HIP_TRY(h, hipMemcpyAsync(all.data(), h->d_sp_all, sizeof(int32_t) * (size_t)n * n, hipMemcpyDeviceToHost, h->stream));
  // the pairs, at their destinations' offsets
  if ((size_t)(2 * total) > h->sp_send_cap) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((rc = dev_alloc(h, &h->d_sp_send, (size_t)(2 * total) + (size_t)(2 * total) / 8 + 64))) return rc;
    h->sp_send_cap = (size_t)(2 * total) + (size_t)(2 * total) / 8 + 64;
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_sp_count, soff.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));   // the destinations' blocks
  if (h->sp_wgs > 0) {
    SparseCountParams sp = sparse_params(h);
    sp.wg_off = h->d_sp_wg_off; sp.dest_base = h->d_sp_count; sp.pairs = h->d_sp_send;
    hipLaunchKernelGGL(sparse_count_kernel<true>, dim3((unsigned)h->sp_wgs), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, sp);
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));        // `all` has arrived (and soff / mine32 may go out of scope)
  int64_t rtotal = 0;
  for (int s2 = 0; s2 < n; ++s2) {
    rcnt[(size_t)s2] = 2 * (int64_t)all[(size_t)s2 * n + me];
    roff[(size_t)s2] = rtotal;
    rtotal += rcnt[(size_t)s2];
  }
  if ((size_t)rtotal > h->sp_recv_cap) {
    if ((rc = dev_alloc(h, &h->d_sp_recv, (size_t)rtotal + (size_t)rtotal / 8 + 64))) return rc;
    h->sp_recv_cap = (size_t)rtotal + (size_t)rtotal / 8 + 64;
  }
  if ((rc = xcall(h, h->xg->ops.all_to_all_v_i32(h->xg->ops.ctx, h->d_sp_send, soff.data(), scnt.data(), h->d_sp_recv, roff.data(), rcnt.data(), h->stream), "all_to_all_v_i32")))
    return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_cnt_own, 0, sizeof(int32_t) * (size_t)h->V * h->Ksm, h->stream));
  if (rtotal > 0) {
    hipLaunchKernelGGL(scatter_add_pairs_kernel, dim3(grid_for(rtotal / 2, 256)), dim3(256), 0, h->stream, h->d_sp_recv, rtotal / 2, h->d_cnt_own);
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));        // the host arrays handed to the transport stay alive until it has used them
  h->cnt_own_valid = true;
  return GGS_OK;
}
int exchange_reduce_scatter(ggs_handle *h) {
  if (h->cnt_own_valid) return GGS_OK;
  if (use_sparse(h) != h->counted_sparse) {            // the form was switched between the count and its exchange: count again in the form that travels
    int rc = launch_count_rebuild(h);
    if (rc) return rc;
  }
  if (use_sparse(h)) return sparse_exchange(h);
  int rc = xcall(h, h->xg->ops.reduce_scatter_i32(h->xg->ops.ctx, h->d_cnt_send, h->d_cnt_own, (int64_t)h->V * h->Ksm, h->stream), "reduce_scatter_i32");
  if (rc) return rc;
  h->cnt_own_valid = true;
  h->cnt_send_zeroed = false;
  return GGS_OK;
}
// the send buffer's contents have been through the reduce-scatter (cnt_own is their sum): dead, clear them on `on`
int clear_send_buffer_if_dead(ggs_handle *h, hipStream_t on) {
  if (!h->xg || h->cnt_send_zeroed || !h->cnt_own_valid || use_sparse(h)) return GGS_OK;
  return clear_send_buffer(h, on);
}

// Corpus-wide counts in d_n_wk: with an exchange, gathered from the ranks' slices on demand (a COLLECTIVE call).  In
// steps, so that a one-process group can issue each collective for all of its devices inside ncclGroupStart/End.
int gather_counts_step_gather(ggs_handle *h) {
  const size_t cells = (size_t)h->xg->nranks * h->V * h->Ksm;
  int rc;
  if (!h->d_cnt_all && (rc = dev_alloc(h, &h->d_cnt_all, cells))) return rc;
  return xcall(h, h->xg->ops.all_gather_i32(h->xg->ops.ctx, h->d_cnt_own, h->d_cnt_all, (int64_t)h->V * h->Ksm, h->stream), "all_gather_i32");
}
int gather_counts_step_unslice(ggs_handle *h) {
  hipLaunchKernelGGL(counts_unslice_kernel, dim3(grid_for((int64_t)h->K * h->V, 256)), dim3(256), 0, h->stream, h->d_cnt_all, h->d_koff, h->Ksm, h->d_n_wk,
                     h->K, h->V);
  HIP_TRY(h, hipGetLastError());
  h->counts_global = true; h->n_k_valid = false;
  return GGS_OK;
}
int ensure_global_counts(ggs_handle *h) {
  if (!h->xg || h->counts_global) return GGS_OK;
  int rc;
  if ((rc = exchange_reduce_scatter(h)) || (rc = clear_send_buffer_if_dead(h, h->stream)) || (rc = gather_counts_step_gather(h))) return rc;
  return gather_counts_step_unslice(h);
}

// tokensPerTopic (and the Dirichlet magnitudes) of the corpus-wide counts
int launch_magnitude(ggs_handle *h) {
  int rc = ensure_global_counts(h);
  if (rc) return rc;
  if (h->n_k_valid) return GGS_OK;
  if ((rc = launch_magnitude_on(h, h->d_n_wk, h->K, h->K, h->d_mag, h->d_n_k))) return rc;
  h->n_k_valid = true;
  return GGS_OK;
}
}  // namespace
