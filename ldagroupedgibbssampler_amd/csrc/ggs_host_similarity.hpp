// ggs_host_similarity.hpp -- the host side of csrc/ggs_similarity.hpp: the launches of the distance family and of the n nearest,
// the training rows (theta estimate, z-bar) produced on the device in pieces, and what ggs_get_theta_estimate, ggs_get_zbar,
// ggs_nearest_documents, ggs_document_distances and ggs_row_distances share.
#pragma once
#include "ggs_host_end_of_run.hpp"
#include "ggs_host_debug.hpp"
#include "ggs_similarity.hpp"

namespace {
constexpr size_t kSimPieceBytes = (size_t)64 << 20;    // the training rows of a piece of documents, a piece of queries, a piece of the [Q][D] output
size_t sim_piece_bytes() { return (size_t)debug_shrunk("GGS_DEBUG_SIM_PIECE_BYTES", (int64_t)kSimPieceBytes); }   // tests: several pieces
constexpr int64_t kSimMaxSegments = 1024;

int sim_aux_kind(int32_t metric) {
  switch (metric) {
    case GGS_DISTANCE_COSINE: case GGS_DISTANCE_UBER: return kSimAuxNorm;
    case GGS_DISTANCE_STATISTICAL: case GGS_DISTANCE_BHATTACHARYYA: return kSimAuxMoments;
    default: return kSimAuxNone;
  }
}
// The segments of A's tiles a query tile is split into: enough workgroups for four per CU, never more than there are tiles.
// GGS_DEBUG_SIM_SEGMENTS (tests: 1 and a number past every tile count) replaces the choice, not the bounds.
int64_t sim_segments(int64_t tiles_a, int64_t tiles_q, int32_t num_cus) {
  int64_t s = (4 * (int64_t)std::max(num_cus, 1) + tiles_q - 1) / std::max<int64_t>(tiles_q, 1);
  if (const char *e = debug_env("GGS_DEBUG_SIM_SEGMENTS")) s = std::atoll(e);
  return std::max<int64_t>(1, std::min<int64_t>(s, std::min<int64_t>(tiles_a, kSimMaxSegments)));
}
void sim_launch_tiles(hipStream_t st, int32_t metric, const SimParams &p, unsigned grid) {
  const dim3 g(grid), b(kDistBlock);
  switch (metric) {
    case GGS_DISTANCE_MANHATTAN: hipLaunchKernelGGL(sim_tile_kernel<SimManhattan>, g, b, 0, st, p); break;
    case GGS_DISTANCE_EUCLIDIAN: hipLaunchKernelGGL(sim_tile_kernel<SimEuclidian>, g, b, 0, st, p); break;
    case GGS_DISTANCE_HELLINGER: hipLaunchKernelGGL(sim_tile_kernel<SimHellinger>, g, b, 0, st, p); break;
    case GGS_DISTANCE_COSINE: hipLaunchKernelGGL(sim_tile_kernel<SimCosine>, g, b, 0, st, p); break;
    case GGS_DISTANCE_CANBERRA: hipLaunchKernelGGL(sim_tile_kernel<SimCanberra>, g, b, 0, st, p); break;
    case GGS_DISTANCE_CHEBYCHEV: hipLaunchKernelGGL(sim_tile_kernel<SimChebychev>, g, b, 0, st, p); break;
    case GGS_DISTANCE_JACCARD: hipLaunchKernelGGL(sim_tile_kernel<SimJaccard>, g, b, 0, st, p); break;
    case GGS_DISTANCE_KL: hipLaunchKernelGGL(sim_tile_kernel<SimKL>, g, b, 0, st, p); break;
    case GGS_DISTANCE_JENSEN_SHANNON: hipLaunchKernelGGL(sim_tile_kernel<SimJensenShannon>, g, b, 0, st, p); break;
    case GGS_DISTANCE_UBER: hipLaunchKernelGGL(sim_tile_kernel<SimUber>, g, b, 0, st, p); break;
    case GGS_DISTANCE_STATISTICAL: hipLaunchKernelGGL(sim_tile_kernel<SimStatistical>, g, b, 0, st, p); break;
    default: hipLaunchKernelGGL(sim_tile_kernel<SimBhattacharyya>, g, b, 0, st, p); break;
  }
}
void sim_launch_aux(hipStream_t st, int32_t metric, const double *rows, int64_t n, int64_t len, double *aux) {
  const int kind = sim_aux_kind(metric);
  if (kind != kSimAuxNone && n > 0) hipLaunchKernelGGL(sim_aux_kernel, dim3(grid_for(n, 256)), dim3(256), 0, st, rows, n, len, kind, aux);
}

// One block of A against one block of B, both on the device with their aux rows made.
struct SimBlock {
  const double *A = nullptr, *auxA = nullptr, *B = nullptr, *auxB = nullptr;
  const int64_t *ptrA = nullptr, *lenB = nullptr;
  int64_t n = 0, m = 0, len = 0, base_a = 0;
};
// dense: out[q * pitch + r] for every pair of the block
void sim_launch_dense(hipStream_t st, int32_t metric, const SimBlock &b, int32_t num_cus, double *out, int64_t pitch) {
  if (b.n <= 0 || b.m <= 0) return;
  const int T = 16 * kSimR[metric];
  SimParams p{};
  p.A = b.A; p.B = b.B; p.auxA = b.auxA; p.auxB = b.auxB; p.ptrA = b.ptrA; p.lenB = b.lenB; p.n = b.n; p.m = b.m; p.len = b.len; p.base_a = b.base_a;
  p.tiles_a = (b.n + T - 1) / T;
  const int64_t tiles_q = (b.m + T - 1) / T;
  p.segs = sim_segments(p.tiles_a, tiles_q, num_cus);
  p.tiles_per_seg = (p.tiles_a + p.segs - 1) / p.segs;
  p.out = out; p.out_pitch = pitch; p.n_nearest = 0;
  sim_launch_tiles(st, metric, p, (unsigned)(tiles_q * p.segs));
}
// nearest: the block's lists into part [m][segs][nn], then merged into res [m][nn] (`first`: res holds nothing yet)
void sim_launch_nearest(hipStream_t st, int32_t metric, const SimBlock &b, int32_t num_cus, int32_t nn, double *part_d, int64_t *part_i, bool first, double *res_d,
                        int64_t *res_i) {
  if (b.m <= 0) return;
  const int T = 16 * kSimR[metric];
  SimParams p{};
  p.A = b.A; p.B = b.B; p.auxA = b.auxA; p.auxB = b.auxB; p.ptrA = b.ptrA; p.lenB = b.lenB; p.n = b.n; p.m = b.m; p.len = b.len; p.base_a = b.base_a;
  p.tiles_a = (b.n + T - 1) / T;
  const int64_t tiles_q = (b.m + T - 1) / T;
  p.segs = sim_segments(p.tiles_a, tiles_q, num_cus);
  p.tiles_per_seg = (p.tiles_a + p.segs - 1) / p.segs;
  p.part_d = part_d; p.part_i = part_i; p.n_nearest = nn;
  sim_launch_tiles(st, metric, p, (unsigned)(tiles_q * p.segs));
  hipLaunchKernelGGL(sim_merge_kernel, dim3((unsigned)((b.m + kSimMergeBlock - 1) / kSimMergeBlock)), dim3(kSimMergeBlock), 0, st, part_d, part_i, b.m, p.segs, (int)nn,
                     first ? 1 : 0, res_d, res_i);
}

// the documents of a piece: at most kSimPieceBytes of counts (4 bytes a cell) and rows (8), at least one document
int64_t sim_doc_piece(int64_t D, int32_t K) { return std::max<int64_t>(1, std::min<int64_t>(D, (int64_t)(sim_piece_bytes() / (12 * (size_t)K)))); }
// rows [nd][K] <- the theta estimate (the handle's current alpha) or the z-bar of documents d0 .. d0 + nd; cnt [nd][K] and norm [nd] are its work space
void sim_launch_doc_rows(ggs_handle *h, int64_t d0, int64_t nd, bool zbar, int32_t *cnt, double *norm, double *rows) {
  if (nd <= 0) return;
  (void)hipMemsetAsync(cnt, 0, sizeof(int32_t) * (size_t)nd * h->K, h->stream);
  hipLaunchKernelGGL(doc_topic_kernel, dim3((unsigned)nd), dim3(64), 0, h->stream, h->d_doc_ptr, h->d_z, d0, h->K, cnt);
  if (!zbar)
    hipLaunchKernelGGL(sim_doc_norm_kernel, dim3((unsigned)((nd + kSimNormDocs - 1) / kSimNormDocs)), dim3(kSimNormDocs), 0, h->stream, cnt, h->d_alpha, nd, h->K, norm);
  hipLaunchKernelGGL(sim_doc_rows_kernel, dim3(grid_for(nd * h->K, 256)), dim3(256), 0, h->stream, cnt, h->d_doc_ptr + d0, h->d_alpha, norm, nd, h->K, zbar ? 1 : 0, rows);
}
// a corpus and a z: the all-zero z that ggs_set_corpus leaves is not a state (a corpus without tokens needs none)
int sim_require_z(ggs_handle *h) {
  const int rc = require_ready(h, false);
  if (rc) return rc;
  if (!h->have_z && h->N > 0) return set_err(h, GGS_ERR_STATE, "no z: call ggs_init_z_java_lcg or ggs_set_z first");
  return GGS_OK;
}
int sim_get_doc_rows(ggs_handle *h, int64_t doc_begin, int64_t doc_end, bool zbar, double *out) {
  int rc = sim_require_z(h);
  if (rc) return rc;
  if (doc_begin < 0 || doc_end > h->D || doc_begin > doc_end || (!out && doc_end > doc_begin)) return set_err(h, GGS_ERR_BAD_ARG, "bad document range");
  const int64_t K = h->K, piece = sim_doc_piece(doc_end - doc_begin, h->K);
  if (doc_end == doc_begin) return GGS_OK;
  const size_t cnt_bytes = (sizeof(int32_t) * (size_t)piece * K + 255) & ~(size_t)255, norm_bytes = (sizeof(double) * (size_t)piece + 255) & ~(size_t)255;
  if ((rc = ensure_scratch(h, cnt_bytes + norm_bytes + sizeof(double) * (size_t)piece * K))) return rc;
  auto *cnt = static_cast<int32_t *>(h->d_scratch);
  auto *norm = reinterpret_cast<double *>(static_cast<char *>(h->d_scratch) + cnt_bytes);
  auto *rows = reinterpret_cast<double *>(static_cast<char *>(h->d_scratch) + cnt_bytes + norm_bytes);
  for (int64_t d0 = doc_begin; d0 < doc_end; d0 += piece) {
    const int64_t nd = std::min(piece, doc_end - d0);
    sim_launch_doc_rows(h, d0, nd, zbar, cnt, norm, rows);
    HIP_TRY(h, hipGetLastError());
    if ((rc = copy_out(h, out + (d0 - doc_begin) * K, rows, sizeof(double) * (size_t)nd * K))) return rc;
  }
  return GGS_OK;
}

int sim_check_metric(ggs_handle *h, int32_t metric) {
  if (metric < 0 || metric >= kSimMetrics) return h ? set_err(h, GGS_ERR_BAD_ARG, "unknown metric: GGS_DISTANCE_* are 0 .. 11") : GGS_ERR_BAD_ARG;
  return GGS_OK;
}
// The handle's documents (theta estimate rows, in pieces) against the queries (in pieces): nn > 0 the nn nearest into idx / dist
// [Q][nn], nn == 0 every distance into dist [Q][D].
int sim_handle_distances(ggs_handle *h, int32_t metric, const double *query, const int64_t *query_len, int64_t Q, int32_t nn, int64_t *idx, double *dist) {
  int rc = sim_require_z(h);
  if (rc) return rc;
  if ((rc = sim_check_metric(h, metric))) return rc;
  if (Q < 0 || (Q > 0 && !query)) return set_err(h, GGS_ERR_BAD_ARG, "null query or negative size");
  const int64_t D = h->D, K = h->K;
  if (nn ? (!idx || !dist) && Q > 0 : !dist && Q > 0 && D > 0) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  for (int64_t q = 0; query_len && q < Q; ++q)
    if (query_len[q] < 0) return set_err(h, GGS_ERR_BAD_ARG, "negative query length");
  if (Q == 0) return GGS_OK;
  if (D == 0) {
    for (int64_t e = 0; e < Q * nn; ++e) { idx[e] = -1; dist[e] = std::numeric_limits<double>::infinity(); }
    return GGS_OK;
  }
  const int64_t dp = sim_doc_piece(D, h->K);
  const size_t row_bytes = sizeof(double) * (size_t)K;
  int64_t qp = std::max<int64_t>(1, (int64_t)(sim_piece_bytes() / row_bytes));
  if (!nn) qp = std::min(qp, std::max<int64_t>(1, (int64_t)(sim_piece_bytes() / (sizeof(double) * (size_t)D))));
  qp = std::min(qp, Q);
  const int T = 16 * kSimR[metric];
  // the lists of a piece of queries: the last piece has fewer tiles and may take more segments
  auto part_cells = [&](int64_t nq) { return nq * sim_segments((dp + T - 1) / T, (nq + T - 1) / T, h->num_cus) * nn; };
  const int64_t part = nn ? std::max(part_cells(qp), Q % qp ? part_cells(Q % qp) : 0) : 0;
  size_t at = 0;
  auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
  const size_t o_cnt = take(sizeof(int32_t) * (size_t)dp * K), o_a = take(row_bytes * (size_t)dp), o_auxa = take(16 * (size_t)dp), o_norm = take(8 * (size_t)dp);
  const size_t o_b = take(row_bytes * (size_t)qp), o_auxb = take(16 * (size_t)qp), o_lenb = take(8 * (size_t)qp);
  const size_t o_pd = take(8 * (size_t)part), o_pi = take(8 * (size_t)part);
  const size_t o_rd = take(nn ? 8 * (size_t)qp * nn : 8 * (size_t)qp * D), o_ri = take(nn ? 8 * (size_t)qp * nn : 0);
  if ((rc = ensure_scratch(h, at))) return rc;
  char *w = static_cast<char *>(h->d_scratch);
  auto Dp = [&](size_t o) { return reinterpret_cast<double *>(w + o); };
  auto Lp = [&](size_t o) { return reinterpret_cast<int64_t *>(w + o); };
  for (int64_t q0 = 0; q0 < Q; q0 += qp) {
    const int64_t nq = std::min(qp, Q - q0);
    HIP_TRY(h, hipMemcpyAsync(Dp(o_b), query + q0 * K, row_bytes * (size_t)nq, hipMemcpyHostToDevice, h->stream));
    if (query_len) HIP_TRY(h, hipMemcpyAsync(Lp(o_lenb), query_len + q0, 8 * (size_t)nq, hipMemcpyHostToDevice, h->stream));
    sim_launch_aux(h->stream, metric, Dp(o_b), nq, K, Dp(o_auxb));
    for (int64_t d0 = 0; d0 < D; d0 += dp) {
      const int64_t nd = std::min(dp, D - d0);
      sim_launch_doc_rows(h, d0, nd, false, reinterpret_cast<int32_t *>(w + o_cnt), Dp(o_norm), Dp(o_a));
      sim_launch_aux(h->stream, metric, Dp(o_a), nd, K, Dp(o_auxa));
      SimBlock b;
      b.A = Dp(o_a); b.auxA = Dp(o_auxa); b.B = Dp(o_b); b.auxB = Dp(o_auxb); b.ptrA = h->d_doc_ptr + d0; b.lenB = query_len ? Lp(o_lenb) : nullptr;
      b.n = nd; b.m = nq; b.len = K; b.base_a = h->doc_base + d0;
      if (nn) sim_launch_nearest(h->stream, metric, b, h->num_cus, nn, Dp(o_pd), Lp(o_pi), d0 == 0, Dp(o_rd), Lp(o_ri));
      else sim_launch_dense(h->stream, metric, b, h->num_cus, Dp(o_rd) + d0, D);
    }
    HIP_TRY(h, hipGetLastError());
    if (nn) {
      if ((rc = copy_out(h, dist + q0 * nn, Dp(o_rd), 8 * (size_t)nq * nn)) || (rc = copy_out(h, idx + q0 * nn, Lp(o_ri), 8 * (size_t)nq * nn))) return rc;
    } else if ((rc = copy_out(h, dist + q0 * D, Dp(o_rd), 8 * (size_t)nq * D))) {
      return rc;
    }
  }
  return GGS_OK;
}

// the handle-free primitive: out [m][n] = distance(a[r], b[q]) at out[q][r]; both blocks whole on the device
int sim_row_distances(int32_t device_id, int32_t metric, const double *a, const double *b, int64_t n, int64_t m, int64_t len, double *out) {
  if (sim_check_metric(nullptr, metric) || n < 0 || m < 0 || len < 1 || ((!a || !b || !out) && n > 0 && m > 0)) return GGS_ERR_BAD_ARG;
  if (n == 0 || m == 0) return GGS_OK;
  if (hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return GGS_ERR_HIP;
  TmpDev t;
  auto *da = static_cast<double *>(t.get(8 * (size_t)n * len)), *db = static_cast<double *>(t.get(8 * (size_t)m * len));
  auto *xa = static_cast<double *>(t.get(16 * (size_t)n)), *xb = static_cast<double *>(t.get(16 * (size_t)m));
  auto *dout = static_cast<double *>(t.get(8 * (size_t)n * m));
  if (!da || !db || !xa || !xb || !dout) return GGS_ERR_HIP;
  if (hipMemcpy(da, a, 8 * (size_t)n * len, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(db, b, 8 * (size_t)m * len, hipMemcpyHostToDevice) != hipSuccess)
    return GGS_ERR_HIP;
  sim_launch_aux(nullptr, metric, da, n, len, xa);
  sim_launch_aux(nullptr, metric, db, m, len, xb);
  SimBlock blk;
  blk.A = da; blk.auxA = xa; blk.B = db; blk.auxB = xb; blk.n = n; blk.m = m; blk.len = len;
  sim_launch_dense(nullptr, metric, blk, prop.multiProcessorCount, dout, n);
  if (hipGetLastError() != hipSuccess || hipMemcpy(out, dout, 8 * (size_t)n * m, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}
}  // namespace
