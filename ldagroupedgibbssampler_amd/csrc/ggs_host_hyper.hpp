// ggs_host_hyper.hpp -- the hyperparameter step (UPLDA:647-649, 891-902; optimizeAlpha / optimizeBeta, MSLDA:812-905): the two
// histograms a handle answers from its device-resident state (ggs_hyper_hist.hpp), the two estimators of MALLET's Dirichlet on the
// host, and the setter that makes a handle the handle of other alpha and beta.
#pragma once
#include "ggs_host_sweep.hpp"

namespace {
// ---- MALLET 2.0.8's Dirichlet.digamma / learnParameters / learnSymmetricConcentration ---------------------------------------------
// The jar is in neither the reference tree nor here: the text of include/ggs_hip.h is the specification, restated line by line in
// tests/hyperparameter_restatement.py.  fp64, left to right, exactly this order (the build has -ffp-contract=off); log is libm's.
double mallet_digamma(double z) {
  if (z < 1e-6) return -0.5772156649015328606065121 - 1 / z;
  double psi = 0;
  while (z < 9.5) { psi -= 1 / z; z += 1; }
  const double x = 1 / z, y = x * x;
  psi += std::log(z) - .5 * x - y * (1 / 12. - y * (1 / 120. - y * (1 / 252. - y * (1 / 240. - y * (1 / 132. - y * (691 / 32760. - y * (1 / 12.)))))));
  return psi;
}

double mallet_learn_parameters(double *params, int32_t K, const int32_t *obs, int64_t n_bins, const int32_t *obs_lengths, int64_t n_len, double shape,
                               double scale, int32_t iterations) {
  double parametersSum = 0;
  for (int32_t k = 0; k < K; ++k) parametersSum += params[k];
  std::vector<int64_t> nonZeroLimit((size_t)K, -1);
  for (int32_t k = 0; k < K; ++k)
    for (int64_t i = 0; i < n_bins; ++i)
      if (obs[(size_t)k * n_bins + i] > 0) nonZeroLimit[(size_t)k] = i;
  for (int32_t it = 0; it < iterations; ++it) {
    double denominator = 0, dg = 0;
    for (int64_t i = 1; i < n_len; ++i) {
      dg += 1 / (parametersSum + (double)i - 1);
      denominator += (double)obs_lengths[i] * dg;
    }
    denominator -= 1 / scale;
    parametersSum = 0;
    for (int32_t k = 0; k < K; ++k) {
      const double old = params[k];
      double p = 0;
      dg = 0;
      for (int64_t i = 1; i <= nonZeroLimit[(size_t)k]; ++i) {
        dg += 1 / (old + (double)i - 1);
        p += (double)obs[(size_t)k * n_bins + i] * dg;
      }
      params[k] = old * (p + shape) / denominator;
      parametersSum += params[k];
    }
  }
  return parametersSum;
}

double mallet_learn_symmetric_concentration(const int32_t *count_hist, int64_t n_hist, const int32_t *obs_lengths, int64_t n_len, int32_t num_dimensions,
                                            double current) {
  int64_t largest = 0;
  for (int64_t i = 0; i < n_hist; ++i)
    if (count_hist[i] > 0) largest = i;
  std::vector<int64_t> nz;
  for (int64_t i = 0; i < n_len; ++i)
    if (obs_lengths[i] > 0) nz.push_back(i);
  for (int it = 0; it < 200; ++it) {
    const double cp = current / (double)num_dimensions;
    double dg = 0, num = 0;
    for (int64_t i = 1; i <= largest; ++i) {
      dg += 1.0 / (cp + (double)i - 1);
      num += (double)count_hist[i] * dg;
    }
    dg = 0;
    double den = 0;
    int64_t prev = 0;
    const double cached = mallet_digamma(current);
    for (const int64_t len : nz) {
      if (len - prev > 20) dg = mallet_digamma(current + (double)len) - cached;
      else
        for (int64_t i = prev; i < len; ++i) dg += 1.0 / (current + (double)i);
      den += dg * (double)obs_lengths[len];
      prev = len;
    }
    current = cp * num / den;
  }
  return current;
}

// ---- the histograms ---------------------------------------------------------------------------------------------------------------
// Bin 0 of a row = items - the row's other bins, modulo 2^32: the bins are Java ints, and bin 0 of the symmetric document histogram
// (D * K pairs) can pass 2^31.
void hist_fill_zero_bins(uint32_t *hist, int64_t rows, int64_t n_bins, uint64_t items) {
  for (int64_t r = 0; r < rows; ++r) {
    uint32_t s = 0;
    for (int64_t c = 1; c < n_bins; ++c) s += hist[r * n_bins + c];
    hist[r * n_bins] = (uint32_t)items - s;
  }
}
constexpr size_t kHistHeadBytes = 16;                   // the flag word, then the bins 16-byte aligned

int doc_topic_histogram(ggs_handle *h, int32_t symmetric, int64_t n_bins, int32_t *hist, int32_t *doc_lengths) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (n_bins < 1 || !hist) return set_err(h, GGS_ERR_BAD_ARG, "ggs_doc_topic_histogram: n_bins < 1 or a null output");
  if (!h->plan.dochist.fn) return set_err(h, GGS_ERR_UNSUPPORTED, "ggs_doc_topic_histogram: num_topics too large for the kernel's LDS");
  const int64_t rows = symmetric ? 1 : h->K;
  const size_t cells = (size_t)rows * (size_t)n_bins, ints = cells + (doc_lengths ? (size_t)n_bins : 0);
  const size_t bytes = kHistHeadBytes + sizeof(uint32_t) * ints;
  if ((rc = ensure_scratch(h, bytes))) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  DocHistParams p{};
  p.doc_ptr = h->d_doc_ptr; p.z = h->d_z;
  p.flag = static_cast<uint32_t *>(h->d_scratch);
  p.hist = p.flag + kHistHeadBytes / sizeof(uint32_t);
  p.len_hist = doc_lengths ? p.hist + cells : nullptr;
  p.num_docs = h->D; p.n_bins = n_bins; p.K = h->K; p.rows = (int32_t)rows; p.tab_bins = doc_hist_tab_bins((int32_t)rows, n_bins);
  void *args[] = {&p};
  if (h->D > 0) HIP_TRY(h, launch(h, h->plan.dochist, h->D, args, h->stream));
  std::vector<uint32_t> out(kHistHeadBytes / sizeof(uint32_t) + ints);
  if ((rc = copy_out(h, out.data(), h->d_scratch, bytes))) return rc;
  if (out[0] & HIST_OVERFLOW) return set_err(h, GGS_ERR_BAD_ARG, "ggs_doc_topic_histogram: a count or a document length >= n_bins");
  uint32_t *bins = out.data() + kHistHeadBytes / sizeof(uint32_t);
  hist_fill_zero_bins(bins, rows, n_bins, symmetric ? (uint64_t)h->D * (uint64_t)h->K : (uint64_t)h->D);
  std::memcpy(hist, bins, sizeof(uint32_t) * cells);
  if (doc_lengths) std::memcpy(doc_lengths, bins + cells, sizeof(uint32_t) * (size_t)n_bins);
  return GGS_OK;
}

int type_topic_count_histogram(ggs_handle *h, int64_t n_bins, int32_t *hist) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (n_bins < 1 || !hist) return set_err(h, GGS_ERR_BAD_ARG, "ggs_type_topic_count_histogram: n_bins < 1 or a null output");
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = ensure_global_counts(h))) return rc;         // with an exchange: the collective gather, as in ggs_get_type_topic_counts
  const size_t bytes = kHistHeadBytes + sizeof(uint32_t) * (size_t)n_bins;
  if ((rc = ensure_scratch(h, bytes))) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  CellHistParams p{};
  p.n_wk = h->d_n_wk;
  p.flag = static_cast<uint32_t *>(h->d_scratch);
  p.hist = p.flag + kHistHeadBytes / sizeof(uint32_t);
  p.n = (int64_t)h->V * h->K; p.n_bins = n_bins;
  void *args[] = {&p};
  const int64_t item_cells = (int64_t)64 * kCellHistPerLane;          // a wave's cells per trip
  HIP_TRY(h, launch(h, h->plan.cellhist, (p.n + item_cells - 1) / item_cells, args, h->stream));
  std::vector<uint32_t> out(kHistHeadBytes / sizeof(uint32_t) + (size_t)n_bins);
  if ((rc = copy_out(h, out.data(), h->d_scratch, bytes))) return rc;
  if (out[0] & HIST_OVERFLOW) return set_err(h, GGS_ERR_BAD_ARG, "ggs_type_topic_count_histogram: a count >= n_bins");
  uint32_t *bins = out.data() + kHistHeadBytes / sizeof(uint32_t);
  hist_fill_zero_bins(bins, 1, n_bins, (uint64_t)p.n);
  std::memcpy(hist, bins, sizeof(uint32_t) * (size_t)n_bins);
  return GGS_OK;
}

// ---- the setter -------------------------------------------------------------------------------------------------------------------
// Everything a handle derives from alpha and beta, refreshed so that it equals a handle created with the new values: the fields
// ggs_create fills, d_alpha behind the queued work of the handle's stream, the Poisson table of the Polya-urn Phi draw; the tables
// over alpha * phi go stale and are rebuilt by the next z step or getter (launch_pcgs_z, refresh_tables); a theta drawn ahead was
// drawn under the old alpha and is dropped.  What the count-form schemes build from alpha and beta (adlda's den0 and S0, the tables
// and lists over the counts, collapsed's ratios) is rebuilt at the head of every sweep anyway (launch_sweep_head).
int set_hyperparameters(ggs_handle *h, const double *alpha, double beta, double beta_sum) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!(beta > 0) || !std::isfinite(beta)) return set_err(h, GGS_ERR_BAD_ARG, "ggs_set_hyperparameters: beta must be positive and finite");
  if (!(beta_sum >= 0) || !std::isfinite(beta_sum)) return set_err(h, GGS_ERR_BAD_ARG, "ggs_set_hyperparameters: beta_sum must be positive and finite, or 0.0 for beta * V");
  for (int32_t k = 0; alpha && k < h->K; ++k)
    if (!(alpha[k] > 0) || !std::isfinite(alpha[k])) return set_err(h, GGS_ERR_BAD_ARG, "ggs_set_hyperparameters: every alpha must be positive and finite");
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_set_hyperparameters inside a split sweep");
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = drop_theta_ahead(h))) return rc;
  if (poisson_phi(h->scheme)) {
    std::vector<double> T;
    build_poisson_table(beta, h->pa_L, T);
    HIP_TRY(h, hipMemcpyAsync(h->d_pa_table, T.data(), sizeof(double) * T.size(), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));         // T leaves the scope
    h->pa_t00 = T[0];
  }
  if (alpha) {
    std::copy(alpha, alpha + h->K, h->alpha.begin());
    HIP_TRY(h, hipMemcpyAsync(h->d_alpha, h->alpha.data(), sizeof(double) * (size_t)h->K, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->alpha_sum = 0;
    for (double a : h->alpha) h->alpha_sum = h->alpha_sum + a;
    h->alpha_symmetric = std::all_of(h->alpha.begin(), h->alpha.end(), [&](double a) { return std::memcmp(&a, &h->alpha[0], sizeof a) == 0; });
  }
  h->beta = beta;
  h->beta_sum = beta_sum == 0.0 ? beta * (double)h->V : beta_sum;
  h->alias_stale = true;
  return GGS_OK;
}
}  // namespace
