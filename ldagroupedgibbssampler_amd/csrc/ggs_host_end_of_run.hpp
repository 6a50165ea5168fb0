// ggs_host_end_of_run.hpp -- what the end-of-run entry points and the getters share: Phi out, the tables' refresh, the diagnostics'
// theta, the min distances' launches, the topic summaries (TsPlan, ts_*), the topic diagnostics (Td*Plan, td_*), the held-out estimator.
#pragma once
#include "ggs_host_sweep.hpp"

namespace {
int phi_out(ggs_handle *h, const double *src_T, int32_t pitch, double *dst, double scale) {
  const size_t kv = (size_t)h->K * h->V;
  int rc = ensure_scratch(h, kv * sizeof(double));
  if (rc) return rc;
  hipLaunchKernelGGL(phiT_to_phi_kernel, dim3(grid_for((int64_t)kv, 256)), dim3(256), 0, h->stream, src_T, static_cast<double *>(h->d_scratch),
                     h->K, pitch, h->V, scale);
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, dst, h->d_scratch, kv * sizeof(double));
}
// What ggs_get_alias_tables and ggs_get_word_topic_lists read, brought up to date: of the current counts (a count-form scheme: what
// the next sweep builds at its head), or of the current Phi
int refresh_tables(ggs_handle *h) {
  int rc;
  if (count_form(h->scheme) || count_tables(h->scheme)) return (rc = require_ready(h, false)) ? rc : launch_sweep_head(h);
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi yet: call ggs_init_phi or ggs_set_phi first");
  return h->alias_stale ? launch_alias_build(h) : GGS_OK;
}
// the diagnostics' theta of a scheme that keeps none (lightpcldaw2): allocated when the log posterior or the document distances first draw one
int ensure_diag_theta(ggs_handle *h) {
  if (h->d_theta) return GGS_OK;
  const int rc = dev_alloc(h, &h->d_theta, (size_t)h->D * h->K + 2);
  if (rc) return rc;
  HIP_TRY(h, hipMemset(h->d_theta, 0, sizeof(double) * ((size_t)h->D * h->K + 2)));
  return GGS_OK;
}
// ll_docs_kernel and lp_docs_kernel keep four K-long histograms per block in LDS (ggs_loglik.hpp)
int ll_check_topics(ggs_handle *h) {
  if (h->K > kLLMaxTopics)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the model log likelihood and the log posterior keep four documents' topic counts in LDS: at most " +
                                               std::to_string(kLLMaxTopics) + " topics fit its 160 KiB, this model has " + std::to_string(h->K));
  return GGS_OK;
}

// ---- min document / topic distances (csrc/ggs_distances.hpp) ---------------------------------------------------------------
// One launch covers at most 2^30 tiles (GGS_DEBUG_DIST_BAND_TILES: fewer): bands of whole tile rows.
constexpr int64_t kDistBandTiles = (int64_t)1 << 30;
int64_t dist_band_rows(int64_t tiles_b) {
  return std::max<int64_t>(1, debug_shrunk("GGS_DEBUG_DIST_BAND_TILES", kDistBandTiles) / std::max<int64_t>(tiles_b, 1));
}
// min_bits[n] (preset by the caller) <- the minimal sums of the rows of A [n][len] over the rows of B [m][len]; B == A with diag
void launch_min_row_dist(hipStream_t st, const double *A, int64_t n, const double *B, int64_t m, int64_t len, bool diag, unsigned long long *min_bits) {
  if (n <= 0 || m <= 0) return;
  constexpr int T = dist_tile_edge(kDistRowR);
  const int64_t ta = (n + T - 1) / T, tb = (m + T - 1) / T, band = dist_band_rows(tb);
  for (int64_t t0 = 0; t0 < ta; t0 += band)
    hipLaunchKernelGGL(min_row_dist_kernel, dim3((unsigned)(std::min(band, ta - t0) * tb)), dim3(kDistBlock), 0, st, A, n, B, m, len, diag ? 1 : 0, t0 * tb, tb, min_bits);
}
// the same for the columns of A [len][pitch] against each other
void launch_min_topic_dist(hipStream_t st, const double *A, int64_t n, int64_t pitch, int64_t len, unsigned long long *min_bits) {
  if (n <= 1) return;
  constexpr int T = dist_tile_edge(kDistTopR);
  const int64_t ta = (n + T - 1) / T, band = dist_band_rows(ta);
  for (int64_t t0 = 0; t0 < ta; t0 += band)
    hipLaunchKernelGGL(min_topic_dist_kernel, dim3((unsigned)(std::min(band, ta - t0) * ta)), dim3(kDistBlock), 0, st, A, n, pitch, len, t0 * ta, ta, min_bits);
}
constexpr size_t kDistPieceBytes = (size_t)64 << 20;   // a foreign block travels to scratch in pieces of at most this
size_t dist_piece_bytes() { return (size_t)debug_shrunk("GGS_DEBUG_DIST_PIECE_BYTES", (int64_t)kDistPieceBytes); }   // tests: several pieces

// ---- top words per topic (csrc/ggs_topic_summaries.hpp) --------------------------------------------------------------------
// the device work space of one call, carved from one allocation
struct TsPlan {
  int32_t V = 0, K = 0, n = 0, nseg = 0, sum_nseg = 0, tot_nseg = 0;
  size_t mass = 0, total = 0, rowsum = 0, k1mass = 0, pw = 0, logpw = 0, guess = 0, fn = 0, tguess = 0, tfn = 0, cand_s = 0, cand_i = 0, idx = 0, score = 0, bytes = 0;
  TsPlan(int32_t V, int32_t K, int32_t n);
};
TsPlan::TsPlan(int32_t V, int32_t K, int32_t n) {
  TsPlan &q = *this;
  q.V = V; q.K = K; q.n = n;
  q.nseg = (V + kTsSegWords - 1) / kTsSegWords;
  q.sum_nseg = (V + kSumSegRows - 1) / kSumSegRows;
  q.tot_nseg = (int32_t)(((int64_t)V * K + kSumSegRows - 1) / kSumSegRows);
  size_t at = 0;
  auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
  q.mass = take(8 * (size_t)K); q.total = take(8);
  q.rowsum = take(8 * (size_t)V); q.k1mass = take(8 * (size_t)V); q.pw = take(8 * (size_t)V); q.logpw = take(8 * (size_t)V);
  q.guess = take(8 * ((size_t)q.sum_nseg + 1) * K); q.fn = take(32 * (size_t)q.sum_nseg * K);
  q.tguess = take(8 * ((size_t)q.tot_nseg + 1)); q.tfn = take(32 * (size_t)q.tot_nseg);
  q.cand_s = take(8 * (size_t)q.nseg * n * K); q.cand_i = take(4 * (size_t)q.nseg * n * K);
  q.idx = take(4 * (size_t)K * n); q.score = take(8 * (size_t)K * n);
  q.bytes = at;
}
int ts_check_args(ggs_handle *h, int32_t V, int32_t K, double beta, int32_t kind, int32_t n, double lambda, const int32_t *idx) {
  if (!idx) return set_err(h, GGS_ERR_BAD_ARG, "null idx");
  if (kind < 0 || kind >= kTsKinds) return set_err(h, GGS_ERR_BAD_ARG, "unknown kind: 0 top, 1 relevance, 2 distinctive, 3 salient, 4 k1");
  if (n < 1 || n > V) return set_err(h, GGS_ERR_BAD_ARG, "Asked for more words (" + std::to_string(n) + ") than there are types (unique words = noTypes = " + std::to_string(V) + ").");
  if (!std::isfinite(lambda)) return set_err(h, GGS_ERR_BAD_ARG, "lambda must be finite");
  if (kind != kTsTop && !(beta > 0.0)) return set_err(h, GGS_ERR_BAD_ARG, "beta must be positive for the probability rankings (the scores of empty cells are NaN otherwise)");
  if (n > kTsMaxWords) return set_err(h, GGS_ERR_UNSUPPORTED, "at most " + std::to_string(kTsMaxWords) + " words per topic");
  if ((int64_t)V * K > ((int64_t)1 << 31) - 256 || (V + kTsSegWords - 1) / kTsSegWords > 16000)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the topic summaries index the V * K cells with 32 bits and keep V / 256 list heads in LDS");
  return GGS_OK;
}
// cnt [V][K] on the device -> idx / score in the work space; norms: the normalisers and the words' statistics whatever the kind
// ev (or NULL): five events recorded around mass_k | total | the words' statistics | selection and merge
void ts_launch(hipStream_t st, bool exact_sum, const int32_t *cnt, double beta, double lambda, int32_t kind, const TsPlan &q, char *work, bool norms, double *all_scores,
               hipEvent_t *ev = nullptr) {
  auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], st); };
  auto D = [&](size_t o) { return reinterpret_cast<double *>(work + o); };
  TsParams p{};
  p.cnt = cnt; p.mass = D(q.mass); p.total = D(q.total); p.rowsum = D(q.rowsum); p.k1mass = D(q.k1mass); p.pw = D(q.pw); p.logpw = D(q.logpw);
  p.cand_score = D(q.cand_s); p.cand_id = reinterpret_cast<int32_t *>(work + q.cand_i); p.idx = reinterpret_cast<int32_t *>(work + q.idx); p.score = D(q.score);
  p.all_scores = all_scores; p.beta = beta; p.lambda = lambda; p.one_minus_lambda = 1 - lambda;
  p.pitch = q.K; p.V = q.V; p.K = q.K; p.kind = kind; p.n = q.n; p.nseg = q.nseg;
  if (norms || kind != kTsTop) {
    // mass_k: the Dirichlet magnitude sum; total: the same sum over the one column of the V * K cells flattened.  Unguided, in
    // work space of their own: the handle's running sums (the Phi phase's guess) are neither read nor written.
    mark(0);
    launch_column_sum<int32_t, true>({st, q.V, beta, exact_sum, q.sum_nseg, D(q.guess), D(q.fn)}, cnt, q.K, q.K, D(q.mass), nullptr, false, false);
    mark(1);
    launch_column_sum<int32_t, true>({st, (int32_t)((int64_t)q.V * q.K), beta, exact_sum, q.tot_nseg, D(q.tguess), D(q.tfn)}, cnt, 1, 1, D(q.total), nullptr, false, false);
    mark(2);
    hipLaunchKernelGGL(ts_words_kernel, dim3((unsigned)((q.V + 63) / 64)), dim3(64), 0, st, p);
  } else {
    mark(0); mark(1); mark(2);
  }
  mark(3);
  if (all_scores) hipLaunchKernelGGL(ts_scores_kernel, dim3((unsigned)((q.K + 255) / 256), (unsigned)std::min(q.V, 4096)), dim3(256), 0, st, p);
  const dim3 grid((unsigned)q.nseg, (unsigned)((q.K + kTsTopics - 1) / kTsTopics));
  if (q.n <= kTsLdsWords) hipLaunchKernelGGL(ts_select_kernel<true>, grid, dim3(64), (size_t)q.n * 64 * 12, st, p);
  else hipLaunchKernelGGL(ts_select_kernel<false>, grid, dim3(64), 0, st, p);
  hipLaunchKernelGGL(ts_merge_kernel, dim3((unsigned)q.K), dim3(64), sizeof(int32_t) * (size_t)q.nseg, st, p);
  mark(4);
}

// ---- topic diagnostics (csrc/ggs_topic_diagnostics.hpp) ---------------------------------------------------------------------
constexpr size_t kTdPieceBytes = (size_t)64 << 20;     // the dense rows of a piece of documents / the sort buffers of a group of topics
// what both planners below size by, wherever they are constructed (a handle's call or its ggs_debug_* twin)
size_t td_piece_bytes() { return (size_t)debug_shrunk("GGS_DEBUG_TD_PIECE_BYTES", (int64_t)kTdPieceBytes); }   // tests: several pieces / groups
// events between the phases of a call (ggs_debug_topic_diagnostics_phases); without it, nothing is recorded
struct TdTimer {
  hipStream_t st;
  ScopedEvents<1024> marks;                            // three per piece of documents: small pieces of a large corpus pass that ...
  signed char phase_of[1024];                          // the phase that ends at a mark, or -1 for a start
  bool lost = false;                                   // ... and a mark that could not be made is reported by collect()
  void mark(int phase) {
    hipEvent_t e = marks.make();
    if (!e) { lost = true; return; }
    (void)hipEventRecord(e, st);
    phase_of[marks.n - 1] = (signed char)phase;
  }
  // after a synchronize: adds every span to ms[phase]; false: a mark was lost, the spans are not the whole call
  bool collect(double *ms) {
    for (int i = 1; i < marks.n; ++i) {
      float f = 0;
      if (phase_of[i] >= 0 && hipEventElapsedTime(&f, marks.ev[i - 1], marks.ev[i]) == hipSuccess) ms[phase_of[i]] += f;
    }
    return !lost;
  }
};
inline void td_mark(TdTimer *t, int phase) { if (t) t->mark(phase); }
enum { kTdPhMembership = 0, kTdPhDocs = 1, kTdPhColumns = 2, kTdPhChain = 3, kTdPhTotals = 4, kTdPhSorted = 5, kTdPhSmall = 6, kTdPhases = 7 };

int td_check_args(ggs_handle *h, int32_t V, int32_t K, int32_t n, const int32_t *idx) {
  if (n < 1 || n > V) return set_err(h, GGS_ERR_BAD_ARG, "Asked for more words (" + std::to_string(n) + ") than there are types (unique words = noTypes = " + std::to_string(V) + ").");
  if (n > kTdMaxWords) return set_err(h, GGS_ERR_UNSUPPORTED, "at most " + std::to_string(kTdMaxWords) + " words per topic");
  if (idx)
    for (size_t i = 0; i < (size_t)K * n; ++i)
      if (idx[i] < 0 || idx[i] >= V) return set_err(h, GGS_ERR_BAD_ARG, "idx holds a word id outside [0, V)");
  return GGS_OK;
}
int td_check_topics(ggs_handle *h, int32_t K) {
  if (K > kTdMaxTopics)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the topic diagnostics keep a document's topic counts and top-word masks in LDS (20 bytes per topic): at most " +
                                               std::to_string(kTdMaxTopics) + " topics fit 60 KiB, this model has " + std::to_string(K));
  return GGS_OK;
}

// the device work space of ggs_topic_doc_statistics
struct TdDocPlan {
  int64_t D = 0, piece = 0;
  int32_t V = 0, K = 0, n = 0;
  size_t mem_ptr = 0, mem = 0, codoc = 0, stats = 0, clogc = 0, maxtopic = 0, crow = 0, addend = 0, bytes = 0;
  TdDocPlan(int64_t D_, int32_t V_, int32_t K_, int32_t n_) : D(D_), V(V_), K(K_), n(n_) {
    // a piece's dense rows (4 + 8 bytes per cell) stay within kTdPieceBytes, but hold at least one wave's 256 documents
    piece = (int64_t)(td_piece_bytes() / (12 * (size_t)K)) / kTdSegDocs * kTdSegDocs;
    piece = std::max<int64_t>(piece, kTdSegDocs);
    piece = std::min<int64_t>(piece, std::max<int64_t>(D, 1));
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
    mem_ptr = take(4 * ((size_t)V + 1)); mem = take(4 * (size_t)K * n); codoc = take(4 * (size_t)K * n * n); stats = take(4 * (size_t)K * kTdStats);
    clogc = take(8 * (size_t)K); maxtopic = take(4 * (size_t)piece); crow = take(4 * (size_t)piece * K); addend = take(8 * (size_t)piece * K);
    bytes = at;
  }
};
// idx [K][n] (host) -> the CSR by word of the (topic, position) pairs
void td_membership(const int32_t *idx, int32_t V, int32_t K, int32_t n, std::vector<int32_t> &ptr, std::vector<int32_t> &mem) {
  ptr.assign((size_t)V + 1, 0);
  mem.assign((size_t)K * n, 0);
  for (size_t i = 0; i < (size_t)K * n; ++i) ptr[(size_t)idx[i] + 1] += 1;
  for (int32_t w = 0; w < V; ++w) ptr[(size_t)w + 1] += ptr[w];
  std::vector<int32_t> cur(ptr.begin(), ptr.end() - 1);
  for (int32_t k = 0; k < K; ++k)
    for (int32_t r = 0; r < n; ++r) mem[(size_t)cur[idx[(size_t)k * n + r]]++] = k * 128 + r;
}
// Enqueues the whole document pass; the results are left in work (q.codoc, q.stats, q.clogc).  The uploads are synchronous.
hipError_t td_doc_launch(hipStream_t st, const TdDocPlan &q, char *work, const int64_t *d_doc_ptr, const int32_t *d_tok, const int32_t *d_z, const double *d_alpha,
                         double alpha_sum, const int32_t *idx, const double *clogc_in, TdTimer *tm) {
  td_mark(tm, -1);
  std::vector<int32_t> ptr, mem;
  td_membership(idx, q.V, q.K, q.n, ptr, mem);
  hipError_t e;
  if ((e = hipMemcpyAsync(work + q.mem_ptr, ptr.data(), 4 * ptr.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.mem, mem.data(), 4 * mem.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(work + q.codoc, 0, q.stats + 4 * (size_t)q.K * kTdStats - q.codoc, st)) != hipSuccess) return e;
  if (clogc_in) e = hipMemcpyAsync(work + q.clogc, clogc_in, 8 * (size_t)q.K, hipMemcpyHostToDevice, st);
  else e = hipMemsetAsync(work + q.clogc, 0, 8 * (size_t)q.K, st);
  if (e != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;           // ptr / mem / clogc_in are pageable host memory
  td_mark(tm, kTdPhMembership);
  TdDocParams p{};
  p.doc_ptr = d_doc_ptr; p.tok = d_tok; p.z = d_z;
  p.mem_ptr = reinterpret_cast<int32_t *>(work + q.mem_ptr); p.mem = reinterpret_cast<int32_t *>(work + q.mem);
  p.crow = reinterpret_cast<int32_t *>(work + q.crow); p.maxtopic = reinterpret_cast<int32_t *>(work + q.maxtopic);
  p.codoc = reinterpret_cast<int32_t *>(work + q.codoc); p.alpha = d_alpha; p.alpha_sum = alpha_sum;
  p.addend = reinterpret_cast<double *>(work + q.addend); p.doc_stats = reinterpret_cast<int32_t *>(work + q.stats);
  p.K = q.K; p.n = q.n;
  double *clogc = reinterpret_cast<double *>(work + q.clogc);
  const unsigned kblocks = (unsigned)((q.K + 63) / 64);
  for (int64_t d0 = 0; d0 < q.D; d0 += q.piece) {
    p.d0 = d0; p.nd = std::min<int64_t>(q.piece, q.D - d0);
    hipLaunchKernelGGL(td_docs_kernel, dim3((unsigned)std::min<int64_t>(p.nd, 4096)), dim3(64), (size_t)kTdLdsPerTopic * q.K, st, p);
    td_mark(tm, kTdPhDocs);
    hipLaunchKernelGGL(td_columns_kernel, dim3(kblocks, (unsigned)((p.nd + kTdSegDocs - 1) / kTdSegDocs)), dim3(64), 0, st, p);
    td_mark(tm, kTdPhColumns);
    hipLaunchKernelGGL(td_clogc_kernel, dim3(kblocks), dim3(64), 0, st, p.addend, p.nd, q.K, clogc);
    td_mark(tm, kTdPhChain);
  }
  hipLaunchKernelGGL(td_mirror_kernel, dim3((unsigned)grid_for((int64_t)q.K * q.n * q.n, 256)), dim3(256), 0, st, p.codoc, q.K, q.n);
  td_mark(tm, kTdPhDocs);
  return hipGetLastError();
}

// the device work space of ggs_topic_scores
struct TdScorePlan {
  int32_t V = 0, K = 0, n = 0, group = 0;
  size_t n_k = 0, wtc = 0, idx = 0, codoc = 0, stats = 0, clogc = 0, head = 0, ts = 0, ws = 0, key_a = 0, id_a = 0, key_b = 0, id_b = 0, bytes = 0;
  TdScorePlan(int32_t V_, int32_t K_, int32_t n_) : V(V_), K(K_), n(n_) {
    group = (int32_t)std::min<size_t>((size_t)K, std::max<size_t>(1, td_piece_bytes() / (16 * (size_t)V)));   // the sort's four [group][V] buffers within kTdPieceBytes
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
    n_k = take(4 * (size_t)K); wtc = take(4 * (size_t)V); idx = take(4 * (size_t)K * n); codoc = take(4 * (size_t)K * n * n); stats = take(4 * (size_t)K * kTdStats);
    clogc = take(8 * (size_t)K); head = take(4 * (size_t)K * n); ts = take(8 * (size_t)kTdScoreRows * K); ws = take(8 * (size_t)kTdWordRows * K * n);
    const size_t buf = 4 * (size_t)group * V;
    key_a = take(buf); id_a = take(buf); key_b = take(buf); id_b = take(buf);
    bytes = at;
  }
};
hipError_t td_score_launch(hipStream_t st, const TdScorePlan &q, char *work, const int32_t *d_cnt, int32_t pitch, double beta, const int32_t *idx, const int32_t *codoc,
                           const int32_t *doc_stats, const double *clogc, bool words, TdTimer *tm) {
  hipError_t e;
  td_mark(tm, -1);
  if ((e = hipMemcpyAsync(work + q.idx, idx, 4 * (size_t)q.K * q.n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.codoc, codoc, 4 * (size_t)q.K * q.n * q.n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.stats, doc_stats, 4 * (size_t)q.K * kTdStats, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.clogc, clogc, 8 * (size_t)q.K, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(work + q.n_k, 0, 4 * (size_t)q.K, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  td_mark(tm, -1);
  auto I = [&](size_t o) { return reinterpret_cast<int32_t *>(work + o); };
  TdScoreParams p{};
  p.cnt = d_cnt; p.n_k = I(q.n_k); p.wtc = I(q.wtc); p.idx = I(q.idx); p.codoc = I(q.codoc); p.doc_stats = I(q.stats);
  p.clogc = reinterpret_cast<double *>(work + q.clogc); p.key_a = I(q.key_a); p.id_a = I(q.id_a); p.key_b = I(q.key_b); p.id_b = I(q.id_b);
  p.sorted_head = I(q.head); p.topic_scores = reinterpret_cast<double *>(work + q.ts); p.word_scores = words ? reinterpret_cast<double *>(work + q.ws) : nullptr;
  p.beta = beta; p.pitch = pitch; p.V = q.V; p.K = q.K; p.n = q.n;
  hipLaunchKernelGGL(td_nk_kernel, dim3((unsigned)((q.K + 63) / 64), (unsigned)std::min(q.V, 256)), dim3(64), 0, st, p);
  hipLaunchKernelGGL(td_wtc_kernel, dim3((unsigned)std::min(q.V, 8192)), dim3(64), 0, st, p);
  td_mark(tm, kTdPhTotals);
  for (int32_t k0 = 0; k0 < q.K; k0 += q.group) {
    p.k0 = k0;
    hipLaunchKernelGGL(td_sorted_kernel, dim3((unsigned)std::min(q.group, q.K - k0)), dim3(64), 0, st, p);
  }
  td_mark(tm, kTdPhSorted);
  hipLaunchKernelGGL(td_small_kernel, dim3((unsigned)q.K), dim3(64), 0, st, p);
  td_mark(tm, kTdPhSmall);
  return hipGetLastError();
}
double td_alpha_sum(const double *alpha, int32_t K) {
  double s = 0;
  for (int32_t k = 0; k < K; ++k) s += alpha[k];
  return s;
}
// idx, or the handle's own top words into own
int td_resolve_idx(ggs_handle *h, int32_t n, const int32_t *&idx, std::vector<int32_t> &own) {
  int rc = td_check_args(h, h->V, h->K, n, idx);
  if (rc || idx) return rc;
  own.resize((size_t)h->K * n);
  if ((rc = ggs_top_words(h, GGS_TOP_WORDS, n, 0.0, own.data(), nullptr))) return rc;
  idx = own.data();
  return GGS_OK;
}
int td_doc_statistics(ggs_handle *h, int32_t n, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats, double *clogc_out, TdTimer *tm) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!codoc || !doc_stats || !clogc_out) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  std::vector<int32_t> own;
  if ((rc = td_resolve_idx(h, n, idx, own)) || (rc = td_check_topics(h, h->K))) return rc;
  const TdDocPlan q(h->D, h->V, h->K, n);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  HIP_TRY(h, td_doc_launch(h->stream, q, work, h->d_doc_ptr, h->d_tok, h->d_z, h->d_alpha, td_alpha_sum(h->alpha.data(), h->K), idx, clogc_in, tm));
  if ((rc = copy_out(h, codoc, work + q.codoc, 4 * (size_t)h->K * n * n)) || (rc = copy_out(h, doc_stats, work + q.stats, 4 * (size_t)h->K * kTdStats))) return rc;
  return copy_out(h, clogc_out, work + q.clogc, 8 * (size_t)h->K);
}
int td_scores(ggs_handle *h, int32_t n, const int32_t *idx, const int32_t *codoc, const int32_t *doc_stats, const double *clogc, double *topic_scores,
              double *word_scores, TdTimer *tm) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!codoc || !doc_stats || !clogc || !topic_scores) return set_err(h, GGS_ERR_BAD_ARG, "null argument");
  std::vector<int32_t> own;
  if ((rc = td_resolve_idx(h, n, idx, own)) || (rc = ensure_global_counts(h))) return rc;
  const TdScorePlan q(h->V, h->K, n);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  HIP_TRY(h, td_score_launch(h->stream, q, work, h->d_n_wk, h->K, h->beta, idx, codoc, doc_stats, clogc, word_scores != nullptr, tm));
  if ((rc = copy_out(h, topic_scores, work + q.ts, 8 * (size_t)kTdScoreRows * h->K))) return rc;
  return word_scores ? copy_out(h, word_scores, work + q.ws, 8 * (size_t)kTdWordRows * h->K * n) : GGS_OK;
}

// ---- the held-out estimator (csrc/ggs_heldout.hpp): ggs_heldout_log_likelihood behind its argument checks ----------------------
int heldout_evaluate(ggs_handle *h, int32_t num_particles, double *doc_ll, double *total) {
  int rc;
  if ((rc = launch_magnitude(h))) return rc;       // corpus-wide counts gathered, tokensPerTopic in step with them
  const int K = h->K;
  const int64_t D = (int64_t)h->test_ptr.size() - 1;
  // LDS: alpha, the denominators and the coefficient table once per block; per wave the word's cell list and 1 or 2 bytes
  // per (particle, topic).  The block shape that puts most waves on a CU wins (the kernel is issue-bound).
  const size_t Kpad = (size_t)(K + 63) / 64 * 64;
  auto lds_of = [&](int w, int cnt_bytes, int cap) { return (size_t)(16 + 8 * cap) * K + (size_t)w * (Kpad * 8 + (size_t)K * 64 * cnt_bytes); };
  struct Shape { int waves = 0, per_cu = 0, cap = 0; };
  auto shape_for = [&](int cnt_bytes, int cap) {
    Shape s; s.cap = cap;
    for (int w = kHeldoutMaxWaves; w >= 1; w >>= 1) {
      const size_t alloc = (lds_of(w, cnt_bytes, cap) + 2047) / 2048 * 2048;   // LDS is handed out in 2 KiB granules
      const int per_cu = alloc <= (size_t)160 * 1024 ? std::min((int)((size_t)160 * 1024 / alloc) * w, 32) : 0;
      if (per_cu && per_cu >= s.per_cu) { s.per_cu = per_cu; s.waves = w; }       // ties: the smaller block (documents differ in length)
    }
    return s;
  };
  // the deepest coefficient table that costs no wave (measured at K=100: 16 -> 31 ms, 32 -> 26, 48 -> 24.6 per evaluation)
  auto best_shape = [&](int cnt_bytes) {
    const int n_caps = (int)(sizeof(kHeldoutCoefCaps) / sizeof(kHeldoutCoefCaps[0]));
    const Shape floor = shape_for(cnt_bytes, kHeldoutCoefCaps[n_caps - 1]);
    for (int i = 0; i < n_caps; ++i) {
      const Shape s = shape_for(cnt_bytes, kHeldoutCoefCaps[i]);
      if (s.per_cu && s.per_cu >= floor.per_cu) return s;
    }
    return floor;
  };
  // a class of documents whose per-particle counts do not fit LDS (more than 1704 topics with one-byte counts, 1024 with
  // two; four-byte counts always) keeps them in global memory: the LDS then holds the tables and the cell lists only
  const Shape shape8 = best_shape(1), shape16 = best_shape(2), shape_spill = best_shape(0);
  const bool spill8 = !h->test_short.empty() && !shape8.waves, spill16 = !h->test_long.empty() && !shape16.waves, spill32 = !h->test_huge.empty();
  if ((spill8 || spill16 || spill32) && !shape_spill.waves)
    return set_err(h, GGS_ERR_UNSUPPORTED, "num_topics too large for the held-out estimator's tables in LDS (about 6000 topics)");
  const int64_t spill_blocks = (int64_t)h->num_cus * std::max(1, shape_spill.waves ? shape_spill.per_cu / shape_spill.waves : 1);   // a persistent grid: what is resident
  if (spill8 || spill16 || spill32) {
    const size_t need = (size_t)spill_blocks * shape_spill.waves * (size_t)K * 64 * (spill32 ? 4 : spill16 ? 2 : 1);
    if (h->heldout_spill_bytes < need) {
      if (h->d_heldout_spill) (void)hipFree(h->d_heldout_spill);
      h->d_heldout_spill = nullptr; h->heldout_spill_bytes = 0;
      HIP_TRY(h, hipMalloc(&h->d_heldout_spill, need));
      h->heldout_spill_bytes = need;
    }
  }
  const void *kernels[] = {reinterpret_cast<const void *>(heldout_particles_kernel<uint8_t, false>), reinterpret_cast<const void *>(heldout_particles_kernel<uint16_t, false>),
                           reinterpret_cast<const void *>(heldout_particles_kernel<uint8_t, true>), reinterpret_cast<const void *>(heldout_particles_kernel<uint16_t, true>),
                           reinterpret_cast<const void *>(heldout_particles_kernel<uint32_t, true>)};
  for (const void *f : kernels) HIP_TRY(h, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
  // wordProbabilities of a batch of documents: tokens x particles doubles, at most ~4 GiB at a time (one launch for
  // the 2 M-token test set of the benchmark: every extra launch has its own tail of half-empty CUs)
  int64_t want_cells = (int64_t)1 << 29;
  if (const char *e = debug_env("GGS_DEBUG_HELDOUT_CELLS")) want_cells = std::max<int64_t>(1, std::atoll(e));   // tests: force several batches
  int64_t longest = 1;
  for (int64_t d = 0; d < D; ++d) longest = std::max(longest, h->test_ptr[d + 1] - h->test_ptr[d]);
  const int64_t cap_cells = std::max<int64_t>(want_cells, longest * num_particles);                                 // a document is never split
  int64_t max_cells = 0;
  std::vector<int64_t> cuts{0};
  for (int64_t d = 0; d < D;) {
    int64_t e = d;
    while (e < D && (h->test_ptr[e + 1] - h->test_ptr[d]) * num_particles <= cap_cells) ++e;
    max_cells = std::max(max_cells, (h->test_ptr[e] - h->test_ptr[d]) * num_particles);
    cuts.push_back(e);
    d = e;
  }
  const size_t tab_bytes = sizeof(double) * (size_t)(2 * K + 2);
  if ((rc = ensure_scratch(h, tab_bytes + sizeof(double) * (size_t)std::max<int64_t>(max_cells, 1)))) return rc;
  HeldoutParams hp{};
  hp.doc_ptr = h->d_test_ptr; hp.tok = h->d_test_tok; hp.n_wk = h->d_n_wk;
  auto *tab = static_cast<double *>(h->d_scratch);
  hp.tab = tab; hp.probs = tab + 2 * K + 2; hp.doc_ll = h->d_test_ll; hp.status = h->d_status;
  hp.beta = h->beta;
  hp.alpha_sum = h->alpha_sum;                         // the k-order sum
  hp.seed = h->seed; hp.iteration = (uint32_t)h->iteration; hp.doc_base = h->test_doc_base;
  hp.K = K; hp.V = h->V; hp.P = num_particles; hp.blocks_per_doc = (num_particles + 63) / 64;
  hipLaunchKernelGGL(heldout_setup_kernel, dim3(1), dim3(64), 0, h->stream, h->d_alpha, h->d_n_k, h->beta, h->beta_sum, K, tab);
  for (size_t b = 0; b + 1 < cuts.size(); ++b) {
    hp.d0 = cuts[b]; hp.d1 = cuts[b + 1];
    if (hp.d1 == hp.d0) continue;
    // the batch's short and long documents: sub-ranges of the two ascending id lists
    auto range = [&](const std::vector<int32_t> &ids, size_t &lo, size_t &hi) {
      lo = std::lower_bound(ids.begin(), ids.end(), (int32_t)hp.d0) - ids.begin();
      hi = std::lower_bound(ids.begin(), ids.end(), (int32_t)hp.d1) - ids.begin();
    };
    // one launch per class of documents present in the batch: counts in LDS where they fit, in global memory otherwise
    struct Class { const std::vector<int32_t> *ids; size_t offset; int bytes; bool spill; Shape shape; };
    const Class classes[] = {{&h->test_short, 0, 1, spill8, spill8 ? shape_spill : shape8},
                             {&h->test_long, h->test_short.size(), 2, spill16, spill16 ? shape_spill : shape16},
                             {&h->test_huge, h->test_short.size() + h->test_long.size(), 4, true, shape_spill}};
    for (const Class &c : classes) {
      size_t lo, hi;
      range(*c.ids, lo, hi);
      if (hi <= lo) continue;
      hp.docs = h->d_test_docs + c.offset + lo; hp.n_docs = (int64_t)(hi - lo); hp.waves = c.shape.waves; hp.cap = c.shape.cap;
      hp.cnt_spill = c.spill ? h->d_heldout_spill : nullptr;
      const int64_t units = hp.n_docs * hp.blocks_per_doc, blocks = (units + hp.waves - 1) / hp.waves;
      const dim3 grid((unsigned)(c.spill ? std::min(blocks, spill_blocks) : blocks)), block((unsigned)(hp.waves * 64));
      const size_t lds = lds_of(hp.waves, c.spill ? 0 : c.bytes, hp.cap);
      const void *f = c.spill ? (c.bytes == 1 ? kernels[2] : c.bytes == 2 ? kernels[3] : kernels[4]) : (c.bytes == 1 ? kernels[0] : kernels[1]);
      void *args[] = {&hp};
      HIP_TRY(h, hipLaunchKernel(f, grid, block, args, lds, h->stream));
    }
    hipLaunchKernelGGL(heldout_reduce_kernel, dim3((unsigned)((hp.d1 - hp.d0 + 3) / 4)), dim3(256), 0, h->stream, hp);
  }
  HIP_TRY(h, hipGetLastError());
  std::vector<double> ll((size_t)D);
  if (D) HIP_TRY(h, hipMemcpyAsync(ll.data(), h->d_test_ll, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, h->stream));
  if ((rc = check_status(h))) return rc;                    // synchronises; MPE:416,447,455,464-469 surface here
  double t = 0;
  for (int64_t d = 0; d < D; ++d) t += ll[(size_t)d];       // MPE:116: in document order
  *total = t;
  if (doc_ll && D) std::memcpy(doc_ll, ll.data(), sizeof(double) * (size_t)D);
  return GGS_OK;
}
}  // namespace
