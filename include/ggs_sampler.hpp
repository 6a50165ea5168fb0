// ggs_sampler.hpp -- C++ host-side mirror of the reference's sampler interface for the GGS
// path, header-only over the C-ABI of ggs_hip.h.
//
// The reference is Java; its toolchain (JDK, Maven, MALLET 2.0.8) is not in the build image, so
// the host side above the C-ABI is written in C++ with the reference's names and call order:
//   cc.mallet.topics.LDAGibbsSampler   (topics/LDAGibbsSampler.java:10-47)
//   cc.mallet.topics.LDASamplerWithPhi (topics/LDASamplerWithPhi.java:5-12)
//   driver call order                  (topics/tui/ParallelLDA.java:173-296):
//     ctor(config) -> setRandomSeed -> addInstances -> sample(iterations) -> getters
// sample() is the per-iteration loop of UncollapsedParallelLDA.sample (UPLDA:645-930): abort flag, exec_time budget
// on cumulative z+Phi time, the eight hooks, and the diagnostics that have a device implementation (log posterior,
// held-out and model log likelihood, topic indicators), written in the Java driver's file formats by ggs_formats.hpp.
// Errors: the Java code throws IllegalStateException / IllegalArgumentException; here a
// non-zero C-ABI return becomes ggs::SamplerError carrying the code and ggs_last_error().
#pragma once
#include <algorithm>
#include <atomic>
#include <fstream>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include <chrono>

#include "ggs_formats.hpp"
#include "ggs_hip.h"

namespace ggs {

struct SamplerError : std::runtime_error {
  int code;
  SamplerError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

// keys of cc.mallet.configuration.LDAConfiguration read on the GGS path, reference defaults
// (LDAConfiguration.java:10-56)
struct LDAConfiguration {
  int topics = 10;                 // NO_TOPICS_DEFAULT
  double alpha = 50.0 / 10;        // ALPHA_DEFAULT
  double beta = 0.01;              // BETA_DEFAULT
  int iterations = 1500;           // NO_ITER_DEFAULT
  int seed = 0;                    // SEED_DEFAULT
  double exec_time = 10;           // seconds, EXEC_TIME_DEFAULT (UPLDA:577,926-928)
  bool save_phi_mean = false;
  int phi_mean_burnin = 0;         // percent of iterations
  int phi_mean_thin = 1;
  bool paranoid = false;
  int hyperparam_optim_interval = -1;   // HYPERPARAM_OPTIM_INTERVAL_DEFAULT (LDAConfiguration.java:46): optimised when > 1 and iteration % interval == 0 (UPLDA:647,891)
  bool symmetric_alpha = false;         // SYMMETRIC_ALPHA_DEFAULT (LDAConfiguration.java:47)
  bool pcgs = false;              // scheme=pcgs instead of ggs (ParallelLDA.java:414-416): the z step of UPLDA:1466-1544
  bool collapsed = false;         // scheme=collapsed (ParallelLDA.java:424-428, SerialCollapsedLDA): the serial chain of MSLDA:158-226
  bool polyaurn = false;          // scheme=polyaurn (ParallelLDA.java:444-447, PolyaUrnSpaliasLDA): the pcgs z step over a Poisson-drawn Phi
  bool spalias = false;           // scheme=spalias (ParallelLDA.java:439-442, SpaliasUncollapsedParallelLDA): the pcgs model, a sparse z step over alias tables
  bool lightpclda = false;        // scheme=lightpclda (ParallelLDA.java:469-473, LightPCLDA): the pcgs model, a Metropolis-Hastings z step over alias tables
  bool polyaurn_sparse = false;   // scheme=polyaurn_sparse (PolyaUrnSpaliasLDA.java:180-334): polyaurn's model, the doubly sparse z step
  bool adlda = false;             // scheme=adlda (ParallelLDA.java:409-412, ADLDA): the collapsed model, the SparseLDA bucket z step over the counts
  bool lightcollapsed = false;    // scheme=lightcollapsed (ParallelLDA.java:429-433, CollapsedLightLDA): the collapsed model, a Metropolis-Hastings z step over the counts
  int alias_poisson_threshold = 100;   // ALIAS_POISSON_DEFAULT_THRESHOLD (LDAConfiguration.java:44); read under polyaurn and polyaurn_sparse only
  int device_id = 0;
  // the diagnostics of the sampling loop (UPLDA:695-905), computed on the device, written as the Java driver writes them
  bool compute_likelihood = false;   // model LL (+ held-out LL with a test set) every iteration, UPLDA:838-850
  int start_diagnostic = 500;        // START_DIAG_DEFAULT; log posterior from this iteration on, UPLDA:706,818-821
  bool compute_doc_topic_distances = false;   // COMPUTE_DOC_TOPIC_DISTANCES_DEFAULT; min_doc_distances.csv / min_topic_distances.csv, UPLDA:723-753,778-806
  int nr_top_words = 20;             // NO_TOP_WORDS_DEFAULT (LDAConfiguration.java:38): words per topic of TopWords.txt / RelevanceWords.txt
  double lambda = 0.6;               // LAMBDA_DEFAULT (LDAConfiguration.java:41): the relevance weight
  bool log_topic_indicators = false; // z_<iteration>.csv, UPLDA:637-638,871-872
  std::string log_dir;               // where the files go (LoggingUtils' run directory in Java); empty = no files
};

// integer CSR of the training InstanceList: FeatureSequence.getFeatures() in instance order
struct InstanceList {
  std::vector<int64_t> doc_ptr;    // D+1
  std::vector<int32_t> tokens;     // N
  int32_t num_types = 0;           // alphabet size
  int64_t size() const { return (int64_t)doc_ptr.size() - 1; }
};

class LDAGroupedGibbsSampler {
 public:
  explicit LDAGroupedGibbsSampler(const LDAConfiguration &config) : config_(config), startSeed_(config.seed) {}
  virtual ~LDAGroupedGibbsSampler() { if (h_) ggs_destroy(h_); }
  LDAGroupedGibbsSampler(const LDAGroupedGibbsSampler &) = delete;
  LDAGroupedGibbsSampler &operator=(const LDAGroupedGibbsSampler &) = delete;

  void setRandomSeed(int seed) { startSeed_ = seed; }                       // MSLDA:153-156
  int getStartSeed() const { return startSeed_; }

  void addInstances(const InstanceList &training) {                         // UPLDA:357-456, GGS:33-37
    if (h_) { ggs_destroy(h_); h_ = nullptr; }
    ggs_config c{};
    c.struct_size = (int32_t)sizeof(ggs_config);
    c.num_topics = config_.topics; c.num_types = training.num_types; c.device_id = config_.device_id;
    c.alpha = nullptr; c.alpha_scalar = config_.alpha; c.beta = config_.beta;
    c.seed = (uint64_t)(int64_t)startSeed_;
    c.flags = (config_.paranoid ? GGS_FLAG_PARANOID : 0) | (config_.save_phi_mean ? GGS_FLAG_SAVE_PHI_MEAN : 0) |
              (config_.pcgs ? GGS_FLAG_PCGS : 0) | (config_.collapsed ? GGS_FLAG_COLLAPSED : 0) | (config_.polyaurn ? GGS_FLAG_POLYAURN : 0) |
              (config_.spalias ? GGS_FLAG_SPALIAS : 0) | (config_.lightpclda ? GGS_FLAG_LIGHTPCLDA : 0) |
              (config_.polyaurn_sparse ? GGS_FLAG_POLYAURN_SPARSE : 0) | (config_.lightcollapsed ? GGS_FLAG_LIGHTCOLLAPSED : 0) | (config_.adlda ? GGS_FLAG_ADLDA : 0);
    c.alias_poisson_threshold = config_.alias_poisson_threshold;
    c.phi_burn_in = (int32_t)(((double)config_.phi_mean_burnin / 100) * config_.iterations);   // UPLDA:206-207
    c.phi_mean_thin = config_.phi_mean_thin;
    int rc = ggs_create(&c, &h_);
    if (rc) { h_ = nullptr; throw SamplerError(rc, "ggs_create failed"); }
    D_ = training.size(); N_ = training.doc_ptr.back(); V_ = training.num_types;
    doc_ptr_ = training.doc_ptr;
    alpha_.assign((size_t)config_.topics, config_.alpha);
    alphaSum_ = config_.alpha * config_.topics;
    chk(ggs_get_hyperparameters(h_, nullptr, &beta_, &betaSum_));              // betaSum = beta * numTypes, UPLDA:372,435
    // docLengthCounts (UPLDA:377-432) and maxTypeCount, once, from the corpus
    int64_t longest = 0;
    for (int64_t d = 0; d < D_; ++d) longest = std::max(longest, doc_ptr_[(size_t)d + 1] - doc_ptr_[(size_t)d]);
    docLengthCounts_.assign((size_t)longest + 1, 0);
    for (int64_t d = 0; d < D_; ++d) docLengthCounts_[(size_t)(doc_ptr_[(size_t)d + 1] - doc_ptr_[(size_t)d])] += 1;
    std::vector<int32_t> typeCounts((size_t)V_, 0);
    for (int32_t w : training.tokens) typeCounts[(size_t)w] += 1;
    maxTypeCount_ = 0;
    for (int32_t n : typeCounts) maxTypeCount_ = std::max(maxTypeCount_, n);
    chk(ggs_set_corpus(h_, D_, training.doc_ptr.data(), training.tokens.data(), 0, 0));
    chk(ggs_init_z_java_lcg(h_, startSeed_));                               // UPLDA:458-460
    chk(ggs_init_phi(h_));                                                  // UPLDA:1287-1294
    currentIteration_ = 0;
  }

  void sample(int iterations) {                                             // UPLDA:552-943
    need();
    preSample();
    const double maxExecMs = config_.exec_time > 0 ? config_.exec_time * 1000.0 : std::numeric_limits<double>::infinity();
    for (int iteration = 1; iteration <= iterations && !abort_.load(); ++iteration) {
      preIteration();
      ggs_timings t0{}, t1{};
      chk(ggs_get_timings(h_, &t0));
      preZ();
      if (config_.collapsed) chk(ggs_collapsed_serial_sweep(h_, startSeed_, 1));   // SerialCollapsedLDA.java:159-172
      else chk(ggs_sweep_begin(h_));                                        // loopOverBatches (+ this device's counts)
      postZ();
      prePhi();
      if (!config_.collapsed) chk(ggs_sweep_end(h_));                       // samplePhi
      postPhi();
      chk(ggs_get_iteration(h_, &currentIteration_));
      chk(ggs_get_timings(h_, &t1));
      zSamplingTimeCum += (t1.theta_ms - t0.theta_ms) + (t1.z_ms - t0.z_ms) + (t1.merge_ms - t0.merge_ms);
      phiSamplingTimeCum += t1.phi_ms - t0.phi_ms;
      diagnostics(iteration);
      if (optimizesAt(iteration)) {                                         // UPLDA:891-894
        optimizeAlpha();
        optimizeBeta();
        chk(ggs_set_hyperparameters(h_, alpha_.data(), beta_, betaSum_));
      }
      postIteration();
      if (std::ifstream("abort").good()) abort();                           // the sentinel file of UPLDA:131,908-910
      if (zSamplingTimeCum + phiSamplingTimeCum >= maxExecMs) break;        // UPLDA:926-928
    }
    postSample();
  }

  void sampleZGivenPhi(int iterations) {                                    // UPLDA:975-1014
    need();
    preSample();
    chk(ggs_sample_z_given_phi(h_, iterations));
    chk(ggs_get_iteration(h_, &currentIteration_));
    postSample();
  }

  int getNoTopics() const { return config_.topics; }
  int getNumTopics() const { return config_.topics; }
  int getNoTypes() const { return V_; }
  int getCurrentIteration() const { return currentIteration_; }
  int64_t getCorpusSize() const { return N_; }
  double getBeta() const { return h_ ? beta_ : config_.beta; }
  double getBetaSum() const { return betaSum_; }
  double getAlphaSum() const { return alphaSum_; }
  std::vector<double> getAlpha() const { return h_ ? alpha_ : std::vector<double>((size_t)config_.topics, config_.alpha); }

  // ---- the hyperparameter step (MALLET's --optimize-interval): the histograms from the device, the estimators in the library ----
  // The count-form classes (SerialCollapsedLDA, CollapsedLightLDA, ADLDA) do not read the key, as in Java.
  bool optimizesAt(int iteration) const {
    return !config_.collapsed && !config_.lightcollapsed && !config_.adlda && config_.hyperparam_optim_interval > 1 &&
           iteration % config_.hyperparam_optim_interval == 0;
  }
  void optimizeAlpha() {                                                    // MSLDA:812-861
    need();
    const int K = config_.topics;
    const int64_t n_bins = (int64_t)docLengthCounts_.size();
    std::vector<int32_t> hist((size_t)(config_.symmetric_alpha ? 1 : K) * (size_t)n_bins);
    chk(ggs_doc_topic_histogram(h_, config_.symmetric_alpha ? 1 : 0, n_bins, hist.data(), nullptr));
    if (config_.symmetric_alpha) {
      chk(ggs_learn_symmetric_concentration(hist.data(), n_bins, docLengthCounts_.data(), n_bins, K, alphaSum_, &alphaSum_));
      for (double &a : alpha_) a = alphaSum_ / K;
    } else {
      chk(ggs_learn_parameters(alpha_.data(), K, hist.data(), n_bins, docLengthCounts_.data(), n_bins, 1.001, 1.0, 1, &alphaSum_));
    }
  }
  void optimizeBeta() {                                                     // MSLDA:863-905
    need();
    std::vector<int32_t> countHistogram((size_t)maxTypeCount_ + 1);
    chk(ggs_type_topic_count_histogram(h_, (int64_t)countHistogram.size(), countHistogram.data()));
    const std::vector<int32_t> tokensPerTopic = getTopicTotals();
    int32_t maxTopicSize = 0;
    for (int32_t n : tokensPerTopic) maxTopicSize = std::max(maxTopicSize, n);
    std::vector<int32_t> topicSizeHistogram((size_t)maxTopicSize + 1, 0);
    for (int32_t n : tokensPerTopic) topicSizeHistogram[(size_t)n] += 1;
    chk(ggs_learn_symmetric_concentration(countHistogram.data(), (int64_t)countHistogram.size(), topicSizeHistogram.data(), (int64_t)topicSizeHistogram.size(), V_,
                                          betaSum_, &betaSum_));
    beta_ = betaSum_ / V_;
  }

  std::vector<std::vector<int32_t>> getZIndicators() {                      // MSLDA:464-477
    need();
    std::vector<int32_t> z((size_t)N_);
    chk(ggs_get_z(h_, z.data()));
    std::vector<std::vector<int32_t>> out((size_t)D_);
    for (int64_t d = 0; d < D_; ++d) out[(size_t)d].assign(z.begin() + doc_ptr_[(size_t)d], z.begin() + doc_ptr_[(size_t)d + 1]);
    return out;
  }
  void setZIndicators(const std::vector<std::vector<int32_t>> &zIndicators) {   // UPLDA:1797-1843
    need();
    std::vector<int32_t> flat;
    flat.reserve((size_t)N_);
    for (const auto &d : zIndicators) flat.insert(flat.end(), d.begin(), d.end());
    if ((int64_t)zIndicators.size() != D_ || (int64_t)flat.size() != N_)
      throw SamplerError(GGS_ERR_BAD_ARG, "Count does not sum to nr. types!");   // UPLDA:1828-1830
    chk(ggs_set_z(h_, flat.data(), 1));
  }
  std::vector<int32_t> getTypeTopicMatrix() {                               // [V][K], UPLDA:226-234
    need();
    std::vector<int32_t> m((size_t)V_ * config_.topics);
    chk(ggs_get_type_topic_counts(h_, m.data()));
    return m;
  }
  std::vector<int32_t> getDocumentTopicMatrix() {                           // [D][K], MSLDA:536-547
    need();
    std::vector<int32_t> m((size_t)D_ * config_.topics);
    chk(ggs_get_doc_topic_counts(h_, 0, D_, m.data()));
    return m;
  }
  std::vector<int32_t> getTopicTotals() {
    need();
    std::vector<int32_t> t((size_t)config_.topics);
    chk(ggs_get_topic_totals(h_, t.data()));
    return t;
  }
  std::vector<double> getZbar() {                                           // [D][K], MSLDA:647-668
    const std::vector<int32_t> ndk = getDocumentTopicMatrix();
    const int K = config_.topics;
    std::vector<double> out((size_t)D_ * K, 0.0);
    for (int64_t d = 0; d < D_; ++d) {
      const double len = (double)(doc_ptr_[(size_t)d + 1] - doc_ptr_[(size_t)d]);
      if (len > 0)
        for (int k = 0; k < K; ++k) out[(size_t)d * K + k] = (double)ndk[(size_t)d * K + k] / len;
    }
    return out;
  }
  std::vector<double> getThetaEstimate() {                                  // [D][K], MSLDA:709-753
    const std::vector<int32_t> ndk = getDocumentTopicMatrix();
    const int K = config_.topics;
    std::vector<double> out((size_t)D_ * K);
    for (int64_t d = 0; d < D_; ++d) {
      double normalizer = 0.0;
      for (int k = 0; k < K; ++k) normalizer += (double)ndk[(size_t)d * K + k] + alpha_[(size_t)k];
      for (int k = 0; k < K; ++k) out[(size_t)d * K + k] = ((double)ndk[(size_t)d * K + k] + alpha_[(size_t)k]) / normalizer;
    }
    return out;
  }
  std::vector<double> getPhi() {                                            // [K][V], UPLDA:1946-1948
    need();
    std::vector<double> p((size_t)V_ * config_.topics);
    chk(ggs_get_phi(h_, p.data()));
    return p;
  }
  void setPhi(const std::vector<double> &phi) {                             // UPLDA:1897-1926
    need();
    if (phi.size() != (size_t)V_ * config_.topics) throw SamplerError(GGS_ERR_BAD_ARG, "phi must be [K][V]");
    chk(ggs_set_phi(h_, phi.data()));
  }
  // empty vector == the Java `null` before any Phi was accumulated (UPLDA:1955-1958)
  std::vector<double> getPhiMeans() {
    need();
    std::vector<double> p((size_t)V_ * config_.topics);
    int32_t n = 0;
    chk(ggs_get_phi_mean(h_, p.data(), &n));
    if (n == 0) p.clear();
    return p;
  }
  std::vector<double> getTheta() {                                          // thetaMatrix, GGS:72
    need();
    std::vector<double> t((size_t)D_ * config_.topics);
    chk(ggs_get_theta(h_, 0, D_, t.data()));
    return t;
  }

  double modelLogLikelihood() {                                             // UPLDA:1644-1758, on the device
    need();
    double a = 0, b = 0;
    chk(ggs_model_log_likelihood(h_, &a, &b));
    return a + b;
  }
  double computeLogPosterior() {                                            // UPLDA:1573-1634, on the device
    need();
    double a = 0, b = 0;
    chk(ggs_log_posterior(h_, &a, &b));
    return a + b;
  }
  std::vector<double> minDocumentDistances() {                              // "Quantity A", UPLDA:723-753, on the device
    need();
    std::vector<double> d((size_t)D_);
    chk(ggs_min_doc_distances(h_, nullptr, 0, d.data()));
    return d;
  }
  double minTopicDistance() {                                               // "Quantity B", UPLDA:778-806, on the device
    need();
    double v = 0;
    chk(ggs_min_topic_distance(h_, &v));
    return v;
  }
  // The topic summaries of LDAUtils.java:566-911 on the device-resident counts (ggs_top_words): [K][n] word ids in IDSorter's
  // order; kind = GGS_TOP_WORDS (getTopWordIndices / getTopWords), GGS_TOP_RELEVANCE (getTopRelevanceWords, config lambda),
  // GGS_TOP_DISTINCTIVE, GGS_TOP_SALIENT, GGS_TOP_K1.
  std::vector<std::vector<int32_t>> getTopWordIndices(int n, int kind = GGS_TOP_WORDS) {
    need();
    if (n > V_)                                                             // LDAUtils.java:568-570
      throw std::invalid_argument("Asked for more words (" + std::to_string(n) + ") than there are types (unique words = noTypes = " + std::to_string(V_) + ").");
    std::vector<int32_t> flat((size_t)config_.topics * (size_t)(n > 0 ? n : 0));
    chk(ggs_top_words(h_, kind, n, config_.lambda, flat.data(), nullptr));
    std::vector<std::vector<int32_t>> out((size_t)config_.topics);
    for (int k = 0; k < config_.topics; ++k) out[(size_t)k].assign(flat.begin() + (size_t)k * n, flat.begin() + (size_t)(k + 1) * n);
    return out;
  }
  // ... and as strings of the alphabet (id -> word): the rows formats::write_top_words takes
  std::vector<std::vector<std::string>> getTopWords(int n, const std::vector<std::string> &alphabet, int kind = GGS_TOP_WORDS) {
    std::vector<std::vector<std::string>> out;
    for (const auto &row : getTopWordIndices(n, kind)) {
      out.emplace_back();
      for (int32_t id : row) out.back().push_back(alphabet.at((size_t)id));
    }
    return out;
  }
  std::vector<std::vector<std::string>> getTopRelevanceWords(int n, const std::vector<std::string> &alphabet) { return getTopWords(n, alphabet, GGS_TOP_RELEVANCE); }
  void addTestInstances(const InstanceList &testSet) {                      // MSLDA:918-923; ids of the training alphabet
    need();
    chk(ggs_set_test_corpus(h_, testSet.size(), testSet.doc_ptr.data(), testSet.tokens.data(), 0));
    haveTestSet_ = true;
  }
  // what sample() logs at UPLDA:622,841: MarginalProbEstimatorPlain(...).evaluateLeftToRight(testSet, numParticles, null)
  double heldOutLogLikelihood(int numParticles = 100) {
    need();
    if (!haveTestSet_) throw SamplerError(GGS_ERR_STATE, "addTestInstances has not been called");
    double total = 0;
    chk(ggs_heldout_log_likelihood(h_, numParticles, nullptr, &total));
    return total;
  }

  // The per-iteration diagnostics of UPLDA:695-905 that have a device implementation, in the Java order; each value is
  // kept in the Java-named list and, with a log_dir, appended in the Java file format.
  std::vector<double> loglikelihood, heldOutLoglikelihood, logPosterior;    // MSLDA:114-115; UPLDA:591,843,849
  std::vector<std::vector<double>> minDocDistances;                         // per diagnostic iteration: the line of min_doc_distances.csv
  std::vector<double> minTopicDistances;                                    // ... and of min_topic_distances.csv
  void diagnostics(int iteration) {
    const bool files = !config_.log_dir.empty();
    if (config_.start_diagnostic > 0 && iteration >= config_.start_diagnostic && !config_.collapsed && !config_.lightcollapsed && !config_.adlda) {   // pcgs: with a fresh theta, UPLDA:710-714
      if (config_.compute_doc_topic_distances) {                            // theta, document distances, topic distance: UPLDA:710-806
        minDocDistances.push_back(minDocumentDistances());
        minTopicDistances.push_back(minTopicDistance());
        if (files) {
          formats::append_min_doc_distances(config_.log_dir, iteration, minDocDistances.back().data(), D_);
          formats::append_min_topic_distance(config_.log_dir, iteration, minTopicDistances.back());
        }
      }
      const double lp = computeLogPosterior();                              // UPLDA:818-821
      logPosterior.push_back(lp);
      if (files)
        formats::append_log_posterior(config_.log_dir, iteration, lp,
                                      std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count());
    }
    if (config_.compute_likelihood) {
      if (haveTestSet_) {                                                   // UPLDA:840-844
        const double ho = heldOutLogLikelihood(100);
        heldOutLoglikelihood.push_back(ho);
        if (files) formats::append_heldout_log_likelihood(config_.log_dir, iteration, ho);
      }
      const double ll = modelLogLikelihood();                               // UPLDA:846-850
      loglikelihood.push_back(ll);
      if (files) formats::append_log_likelihood(config_.log_dir, iteration, ll);
      if (config_.log_topic_indicators && files) {                          // UPLDA:871-872
        std::vector<int32_t> z((size_t)N_);
        chk(ggs_get_z(h_, z.data()));
        formats::write_topic_indicators(doc_ptr_.data(), D_, z.data(), config_.log_dir, iteration);
      }
    }
  }

  void abort() { abort_.store(true); }                                      // MSLDA:601-603; may come from another thread
  bool getAbort() const { return abort_.load(); }

  // hooks: no-ops in the reference (MSLDA:783-810), virtual so a subclass can observe the loop
  virtual void preIteration() {}
  virtual void postIteration() {}
  virtual void preSample() {}
  virtual void postSample() {}
  virtual void preZ() {}
  virtual void postZ() {}
  virtual void prePhi() {}
  virtual void postPhi() {}

  double zSamplingTimeCum = 0, phiSamplingTimeCum = 0;                       // ms, UPLDA:642-693
  ggs_handle *native_handle() { return h_; }

 private:
  void need() const { if (!h_) throw SamplerError(GGS_ERR_STATE, "addInstances has not been called"); }
  void chk(int rc) { if (rc) throw SamplerError(rc, ggs_last_error(h_)); }
  LDAConfiguration config_;
  ggs_handle *h_ = nullptr;
  int startSeed_ = 0;
  int32_t currentIteration_ = 0;
  int64_t D_ = 0, N_ = 0;
  int32_t V_ = 0;
  std::vector<int64_t> doc_ptr_;
  std::vector<double> alpha_;                                                // the current hyperparameters: the configuration's until the step learns others
  double alphaSum_ = 0, beta_ = 0, betaSum_ = 0;
  std::vector<int32_t> docLengthCounts_;
  int32_t maxTypeCount_ = 0;
  std::atomic<bool> abort_{false};
  bool haveTestSet_ = false;
};

}  // namespace ggs
