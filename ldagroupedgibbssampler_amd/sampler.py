"""Host-side mirror of the reference's sampler interface for the GGS path.

``LDAGroupedGibbsSampler`` keeps the method names, argument meaning and error behaviour of
``cc.mallet.topics.LDAGibbsSampler`` + ``LDASamplerWithPhi`` (LDAGibbsSampler.java:10-47,
LDASamplerWithPhi.java:5-12) for the calls the driver makes on the hot path
(tui/ParallelLDA.java:173-296): ctor(config) -> setRandomSeed -> addInstances -> sample ->
getters.  All numerics happen in libggs_hip.so through the C-ABI; this file is orchestration
(the per-iteration loop of UncollapsedParallelLDA.sample, UPLDA:645-930: abort flag, exec_time
budget, hooks) plus the cheap host-side helpers z-bar / theta estimate (MSLDA:617-778).

The reference toolchain (JDK, Maven, MALLET) is absent from the build image, so this mirror is
Python over ctypes for the tests and the benchmark; include/ggs_sampler.hpp is the same mirror
in C++, and INTEGRATION.md shows the JNI subclass a maintainer would add on the Java side.
"""
import os
import time

import numpy as np

from . import native
from .corpus import Corpus


class SimpleLDAConfiguration:
    """The keys of cc.mallet.configuration.LDAConfiguration the GGS path reads, with the
    reference's defaults (LDAConfiguration.java:10-56).  Mirrors the test-side POJO
    SimpleLDAConfiguration; INI parsing / CLI overrides stay in Java (out of scope)."""

    def __init__(self, **kw):
        self.scheme = kw.pop("scheme", "ggs")
        self.topics = int(kw.pop("topics", 10))                      # NO_TOPICS_DEFAULT
        self.alpha = float(kw.pop("alpha", 50.0 / 10))               # ALPHA_DEFAULT = 50.0 / NO_TOPICS_DEFAULT
        self.beta = float(kw.pop("beta", 0.01))                      # BETA_DEFAULT
        self.iterations = int(kw.pop("iterations", 1500))            # NO_ITER_DEFAULT
        self.seed = int(kw.pop("seed", 0))                           # SEED_DEFAULT: 0 = use the clock (ParsedLDAConfiguration.java:137-141)
        self.exec_time = kw.pop("exec_time", 10)                     # EXEC_TIME_DEFAULT seconds of z+Phi time (UPLDA:577,926-928)
        self.save_phi_mean = bool(kw.pop("save_phi_mean", False))    # SAVE_PHI_MEAN_DEFAULT
        self.phi_mean_burnin = int(kw.pop("phi_mean_burnin", 0))     # percent of iterations, PHI_BURN_IN_DEFAULT
        self.phi_mean_thin = int(kw.pop("phi_mean_thin", 1))         # PHI_THIN_DEFAULT
        self.alias_poisson_threshold = int(kw.pop("alias_poisson_threshold", 100))   # ALIAS_POISSON_DEFAULT_THRESHOLD; scheme=polyaurn and polyaurn_sparse only
        self.topic_prior_filename = kw.pop("topic_prior_filename", None)   # TOPIC_PRIOR_FILENAME, default none; scheme=spalias_priors only
        self.variable_selection_prior = float(kw.pop("variable_selection_prior", 0.5))   # VARIABLE_SELECTION_PRIOR_DEFAULT; scheme=nzvsspalias only
        self.hyperparam_optim_interval = int(kw.pop("hyperparam_optim_interval", -1))   # HYPERPARAM_OPTIM_INTERVAL_DEFAULT (LDAConfiguration.java:46): optimised when > 1 and iteration % interval == 0, UPLDA:647,891
        self.symmetric_alpha = bool(kw.pop("symmetric_alpha", False))                   # SYMMETRIC_ALPHA_DEFAULT (LDAConfiguration.java:47)
        self.paranoid = bool(kw.pop("paranoid", False))              # run the UPLDA:299-338 invariants every sweep
        self.device_id = int(kw.pop("device_id", 0))                 # optional gpu_* key; default first visible GPU
        # the diagnostics of the sampling loop (UPLDA:695-905), computed on the device and written in the Java driver's formats
        self.compute_likelihood = bool(kw.pop("compute_likelihood", False))   # model LL (+ held-out LL with a test set) every iteration, UPLDA:838-850
        self.start_diagnostic = int(kw.pop("start_diagnostic", 500))          # START_DIAG_DEFAULT; log posterior from this iteration on, UPLDA:706,818-821
        self.compute_doc_topic_distances = bool(kw.pop("compute_doc_topic_distances", False))   # COMPUTE_DOC_TOPIC_DISTANCES_DEFAULT; min_doc_distances.csv / min_topic_distances.csv from start_diagnostic on, UPLDA:723-753,778-806
        self.nr_top_words = int(kw.pop("nr_top_words", 20))                   # NO_TOP_WORDS_DEFAULT (LDAConfiguration.java:38): the words per topic of TopWords.txt / RelevanceWords.txt
        self.lambda_ = float(kw.pop("lambda", 0.6))                           # LAMBDA_DEFAULT (LDAConfiguration.java:41), the relevance weight; `lambda` is a Python keyword: pass **{"lambda": x}
        self.save_doc_topic_diagnostics = bool(kw.pop("save_doc_topic_diagnostics", False))   # ParsedLDAConfiguration.java:324-327: the driver writes TopicModelDiagnosticsPlain.topicsToCsv, tui/ParallelLDA.java:218-225
        self.doc_topic_diagnostics_filename = kw.pop("doc_topic_diagnostics_filename", None)   # ParsedLDAConfiguration.java:330-332: its file name in the run directory (no default in Java either)
        self.log_topic_indicators = bool(kw.pop("log_topic_indicators", False))  # z_<iteration>.csv, UPLDA:637-638,871-872
        self.log_dir = kw.pop("log_dir", None)                       # where the files go (LoggingUtils' run directory in Java); None = no files
        if kw:
            raise TypeError("unknown configuration keys: %s" % sorted(kw))

    def get_seed(self):
        if self.seed == 0:
            return int(time.time() * 1000) & 0x7FFFFFFF
        return self.seed


def calc_zbar(num_topics, one_doc_topics):
    """ModifiedSimpleLDA.calcZBar (MSLDA:647-668): topic frequencies of one document; an empty
    document gives zeros."""
    z = np.asarray(one_doc_topics, np.int64)
    counts = np.bincount(z, minlength=num_topics).astype(np.float64)
    if z.size == 0:
        return np.zeros(num_topics)
    return counts / z.size


def calc_theta_estimate(num_topics, alpha, one_doc_topics):
    """ModifiedSimpleLDA.calcThetaEstimate (MSLDA:709-753): (n_k + alpha_k) / sum_k (n_k + alpha_k),
    the normaliser summed in k order exactly as the Java loop does."""
    a = np.broadcast_to(np.asarray(alpha, np.float64), (num_topics,))
    counts = np.bincount(np.asarray(one_doc_topics, np.int64), minlength=num_topics).astype(np.float64)
    normalizer = 0.0
    for k in range(num_topics):
        normalizer += counts[k] + a[k]
    est = (counts + a) / normalizer
    if not np.all(np.isfinite(est)) or (est < 0).any():
        raise RuntimeError("theta estimate is broken")               # IllegalStateException, MSLDA:727-729
    return est


def model_log_likelihood(n_dk, n_wk, n_k, alpha, beta):
    """UncollapsedParallelLDA.modelLogLikelihood (UPLDA:1644-1758): Dirichlet-multinomial log
    likelihood of the topic assignments, from the count matrices alone.  Host-side diagnostic
    (it stays on the host in the reference too).  MALLET's Dirichlet.logGammaStirling is not
    in the reference tree; scipy's gammaln stands in for it (restate from the public
    formula, ~1e-6 relative), so against a JVM value this is pinned only to that accuracy."""
    from scipy.special import gammaln
    n_dk = np.asarray(n_dk, np.float64)
    n_wk = np.asarray(n_wk, np.float64)
    n_k = np.asarray(n_k, np.float64)
    K = n_dk.shape[1]
    V = n_wk.shape[0]
    a = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    alpha_sum = float(a.sum())
    ll = 0.0
    nz = n_dk > 0                                                    # UPLDA:1680-1685
    ll += float((gammaln(n_dk + a)[nz]).sum() - (np.broadcast_to(gammaln(a), n_dk.shape)[nz]).sum())
    ll -= float(gammaln(alpha_sum + n_dk.sum(1)).sum())              # UPLDA:1689
    ll += n_dk.shape[0] * float(gammaln(alpha_sum))                  # UPLDA:1694
    nzw = n_wk > 0                                                   # UPLDA:1701-1722
    ll += float(gammaln(beta + n_wk[nzw]).sum())
    ll -= float(gammaln(beta * V + n_k).sum())                       # UPLDA:1724-1728
    ll += float(gammaln(beta * V)) * K                               # UPLDA:1742-1743
    ll -= float(gammaln(beta)) * int(nzw.sum())                      # UPLDA:1746-1747
    return ll


class LDAGroupedGibbsSampler:
    """scheme=ggs on MI355X.  One instance drives one GPU (doc-sharded runs wrap the same
    native handle with ldagroupedgibbssampler_amd.sharded.ShardedGGS)."""
    _scheme_flags = 0
    _optimizes_hyperparameters = True    # the samplers on the UncollapsedParallelLDA base (UPLDA:891-894); the count-form classes do not

    def __init__(self, config):
        self.config = config
        self.numTopics = config.topics
        self.alpha = np.full(self.numTopics, config.alpha, np.float64)       # MSLDA:129-135
        self.alphaSum = config.alpha * self.numTopics
        self.beta = config.beta
        self.betaSum = None                                                  # beta * numTypes at addInstances (UPLDA:372,435)
        self.startSeed = config.get_seed()
        self.currentIteration = 0
        self._abort = False
        self._h = None
        self._corpus = None
        self.zSamplingTimeCum = 0.0      # ms, as UPLDA:642-693 accumulates them
        self.phiSamplingTimeCum = 0.0
        self.loglikelihood, self.heldOutLoglikelihood, self.logPosterior = [], [], []   # the Java lists (MSLDA:114-115; UPLDA:591,843,849) + the posterior values
        self.minDocDistances, self.minTopicDistances = [], []    # per diagnostic iteration: the line of min_doc_distances.csv ([D]) and of min_topic_distances.csv

    # ---- LDAGibbsSampler ----
    def setConfiguration(self, config):
        self.config = config

    def getConfiguration(self):
        return self.config

    def setRandomSeed(self, seed):
        """MSLDA:153-156: only the initial z depends on it (called before addInstances,
        tui/ParallelLDA.java:176,189); it also keys this build's Philox streams."""
        self.startSeed = int(seed)

    def addInstances(self, training):
        """UPLDA:357-456 + GGS:33-37.  `training` is a Corpus (integer CSR of the
        FeatureSequences in instance order)."""
        if not isinstance(training, Corpus):
            raise TypeError("addInstances expects a ldagroupedgibbssampler_amd.corpus.Corpus")
        cfg = self.config
        flags = (native.FLAG_PARANOID if cfg.paranoid else 0) | (native.FLAG_SAVE_PHI_MEAN if cfg.save_phi_mean else 0) | self._scheme_flags
        burn_in = int((cfg.phi_mean_burnin / 100.0) * cfg.iterations)        # UPLDA:206-207
        self._h = native.GGSHandle(self.numTopics, training.num_types, self.alpha, self.beta, self.startSeed,
                                   device_id=cfg.device_id, flags=flags, phi_burn_in=burn_in, phi_mean_thin=cfg.phi_mean_thin,
                                   alias_poisson_threshold=getattr(cfg, "alias_poisson_threshold", 100))
        self._corpus = training
        self.betaSum = self._h.hyperparameters()[2]
        self._doc_length_counts = None
        self._h.set_corpus(training.doc_ptr, training.tokens)
        self._before_initial_state(training)
        self._h.init_z_java_lcg(self.startSeed)          # initialDrawTopicIndicator, UPLDA:458-460
        self._h.init_phi()                               # initialSamplePhi, UPLDA:1287-1294
        self.currentIteration = 0

    def _before_initial_state(self, training):
        """what a scheme sets on the new handle before the initial z and Phi are drawn"""

    def addTestInstances(self, test_set):
        """MSLDA:918-923: the test set of the held-out estimator; it must share the training alphabet
        ("Alphabets on training and test sets do not match!")."""
        self._need_data()
        if not isinstance(test_set, Corpus):
            raise TypeError("addTestInstances expects a ldagroupedgibbssampler_amd.corpus.Corpus")
        if test_set.num_types != self._corpus.num_types:
            raise ValueError("Alphabets on training and test sets do not match!")
        self._h.set_test_corpus(test_set.doc_ptr, test_set.tokens)
        self._test_set = test_set

    def heldOutLogLikelihood(self, num_particles=100):
        """What the sampling loop logs when a test set is present (UPLDA:604-622,840-844):
        MarginalProbEstimatorPlain(...).evaluateLeftToRight(testSet, 100, null), on the device."""
        self._need_data()
        if getattr(self, "_test_set", None) is None:
            raise ValueError("no test set: call addTestInstances first")
        return self._h.heldout_log_likelihood(num_particles)[0]

    def sample(self, iterations):
        """UPLDA:552-943 without the host-side diagnostics: one native sweep per iteration so the
        abort flag and the exec_time budget keep their per-iteration granularity."""
        self._need_data()
        self.preSample()
        max_exec_ms = float(self.config.exec_time) * 1000.0 if self.config.exec_time is not None else float("inf")
        for iteration in range(1, int(iterations) + 1):
            if self._abort:
                break
            self.preIteration()
            self.preZ()
            t0 = self._h.get_timings()
            self._z_half()                               # loopOverBatches + the local half of updateCounts
            self.postZ()
            self.prePhi()
            self._phi_half()                             # samplePhi
            self.postPhi()
            self.currentIteration = self._h.iteration
            t1 = self._h.get_timings()
            self.zSamplingTimeCum += (t1["theta_ms"] - t0["theta_ms"]) + (t1["z_ms"] - t0["z_ms"]) + (t1["merge_ms"] - t0["merge_ms"])
            self.phiSamplingTimeCum += t1["phi_ms"] - t0["phi_ms"]
            self._diagnostics(iteration)
            if self.optimizes_at(iteration):             # UPLDA:891-894
                self.optimizeAlpha()
                self.optimizeBeta()
                self._h.set_hyperparameters(self.alpha, self.beta, self.betaSum)
            self.postIteration()
            if os.path.exists("abort"):                  # the sentinel file of UPLDA:131,908-910 (relative to the working directory)
                self.abort()
            if self.zSamplingTimeCum + self.phiSamplingTimeCum >= max_exec_ms:   # UPLDA:926-928
                break
        self.postSample()

    def _z_half(self):
        self._h.sweep_begin()

    def _phi_half(self):
        self._h.sweep_end()

    # ---- the hyperparameter step (hyperparam_optim_interval, MALLET's --optimize-interval) ----
    def optimizes_at(self, iteration):
        """UPLDA:647,891: hyperparameterOptimizationInterval > 1 && iteration % hyperparameterOptimizationInterval == 0"""
        interval = int(getattr(self.config, "hyperparam_optim_interval", -1))
        return self._optimizes_hyperparameters and interval > 1 and iteration % interval == 0

    def optimizeAlpha(self):
        """MSLDA:812-861: topicDocCounts from the device-resident z (ggs_doc_topic_histogram), docLengthCounts from the corpus (once,
        UPLDA:377-432), then Dirichlet.learnSymmetricConcentration or learnParameters(alpha, ..., 1.001, 1.0, 1).  The new values
        reach the device with the set_hyperparameters call of the step."""
        self._need_data()
        if self._doc_length_counts is None:
            lens = np.diff(self._corpus.doc_ptr)
            self._doc_length_counts = np.bincount(lens, minlength=int(lens.max()) + 1 if lens.size else 1).astype(np.int32)
        lengths = self._doc_length_counts
        symmetric = bool(getattr(self.config, "symmetric_alpha", False))
        hist, _ = self._h.doc_topic_histogram(symmetric, lengths.size, lengths=False)
        if symmetric:
            self.alphaSum = native.learn_symmetric_concentration(hist[0], lengths, self.numTopics, self.alphaSum)
            self.alpha[:] = self.alphaSum / self.numTopics
        else:
            self.alphaSum = native.learn_parameters(self.alpha, hist, lengths, 1.001, 1.0, 1)

    def optimizeBeta(self):
        """MSLDA:863-905: countHistogram from the device-resident counts (ggs_type_topic_count_histogram, maxTypeCount + 1 bins),
        topicSizeHistogram from tokensPerTopic, betaSum = Dirichlet.learnSymmetricConcentration(...), beta = betaSum / numTypes."""
        self._need_data()
        V = self._corpus.num_types
        tokens = self._corpus.tokens
        max_type_count = int(np.bincount(tokens, minlength=V).max()) if len(tokens) else 0
        count_hist = self._h.type_topic_count_histogram(max_type_count + 1)
        n_k = self._h.get_topic_totals()
        topic_size_hist = np.bincount(n_k, minlength=int(n_k.max()) + 1).astype(np.int32)
        self.betaSum = native.learn_symmetric_concentration(count_hist, topic_size_hist, V, self.betaSum)
        self.beta = self.betaSum / V

    def _diagnostics(self, iteration):
        """The per-iteration diagnostics of UPLDA:695-905 that have a device implementation, in the Java order: document and
        topic distances (compute_doc_topic_distances) and log
        posterior (ggs and pcgs, from start_diagnostic on), held-out and model log likelihood (compute_likelihood), topic
        indicators; each value is kept in the Java-named list and, with a log_dir, appended in the Java file format."""
        cfg = self.config
        from . import formats as F
        if cfg.start_diagnostic > 0 and iteration >= cfg.start_diagnostic and not (self._scheme_flags & (native.FLAG_COLLAPSED | native.FLAG_LIGHTCOLLAPSED | native.FLAG_ADLDA)):   # pcgs: with a fresh theta, UPLDA:710-714
            if getattr(cfg, "compute_doc_topic_distances", False):        # theta, document distances, topic distance: UPLDA:710-806
                dd, td = self.minDocumentDistances(), self.minTopicDistance()
                self.minDocDistances.append(dd)
                self.minTopicDistances.append(td)
                if cfg.log_dir:
                    F.append_min_doc_distances(cfg.log_dir, iteration, dd)
                    F.append_min_topic_distance(cfg.log_dir, iteration, td)
            lp = self.computeLogPosterior()                               # UPLDA:818-821
            self.logPosterior.append(lp)
            if cfg.log_dir:
                F.append_log_posterior(cfg.log_dir, iteration, lp, int(time.time() * 1000))
        if cfg.compute_likelihood:
            if getattr(self, "_test_set", None) is not None:             # UPLDA:840-844
                ho = self.heldOutLogLikelihood(100)
                self.heldOutLoglikelihood.append(ho)
                if cfg.log_dir:
                    F.append_heldout_log_likelihood(cfg.log_dir, iteration, ho)
            ll = self.modelLogLikelihood()                                # UPLDA:846-850
            self.loglikelihood.append(ll)
            if cfg.log_dir:
                F.append_log_likelihood(cfg.log_dir, iteration, ll)
            if cfg.log_topic_indicators and cfg.log_dir:                  # UPLDA:871-872
                F.write_topic_indicators(self._corpus.doc_ptr, self._h.get_z(), cfg.log_dir, iteration)

    def sampleZGivenPhi(self, iterations):
        self._need_data()
        self.preSample()
        self._h.sample_z_given_phi(int(iterations))
        self.currentIteration = self._h.iteration
        self.postSample()

    def getNoTopics(self):
        return self.numTopics

    getNumTopics = getNoTopics

    def getNoTypes(self):
        self._need_data()
        return self._corpus.num_types

    def getCurrentIteration(self):
        return self.currentIteration

    def getCorpusSize(self):
        self._need_data()
        return self._corpus.num_tokens

    def getStartSeed(self):
        return self.startSeed

    def getZIndicators(self):
        """int[D][] (MSLDA:464-477)"""
        self._need_data()
        z = self._h.get_z()
        p = self._corpus.doc_ptr
        return [z[p[d]:p[d + 1]] for d in range(self._corpus.num_docs)]

    def setZIndicators(self, z_indicators):
        """UPLDA:1797-1843: rebuilds the counts and re-draws Phi; throws when the lengths do not
        add up to the corpus size (IllegalArgumentException, UPLDA:1828-1830)."""
        self._need_data()
        flat = np.concatenate([np.asarray(z, np.int32) for z in z_indicators]) if len(z_indicators) else np.zeros(0, np.int32)
        lens = [len(z) for z in z_indicators]
        if len(z_indicators) != self._corpus.num_docs or lens != list(np.diff(self._corpus.doc_ptr)):
            raise ValueError("Count does not sum to nr. types! Sumtotal: %d no.types: %d" % (flat.size, self._corpus.num_tokens))
        self._h.set_z(flat, redraw_phi=True)

    def getTypeTopicMatrix(self):
        self._need_data()
        return self._h.get_type_topic_counts()           # [V][K], UPLDA:226-234

    def getDocumentTopicMatrix(self):
        self._need_data()
        return self._h.get_doc_topic_counts()            # [D][K], MSLDA:536-547

    def getTopicTotals(self):
        self._need_data()
        return self._h.get_topic_totals()

    def getZbar(self):
        n_dk = self.getDocumentTopicMatrix().astype(np.float64)
        lens = np.diff(self._corpus.doc_ptr).astype(np.float64)
        out = np.zeros_like(n_dk)
        nz = lens > 0
        out[nz] = n_dk[nz] / lens[nz, None]              # MSLDA:655-660
        return out

    def getThetaEstimate(self):
        n_dk = self.getDocumentTopicMatrix()
        return np.stack([self._theta_estimate_from_counts(row) for row in n_dk]) if len(n_dk) else np.zeros((0, self.numTopics))

    def _theta_estimate_from_counts(self, counts):
        normalizer = 0.0
        for k in range(self.numTopics):
            normalizer += float(counts[k]) + self.alpha[k]
        return (counts.astype(np.float64) + self.alpha) / normalizer

    def getTheta(self):
        """thetaMatrix of the last z step (GGS:72; what UPLDA:716-720 copies for scheme ggs)."""
        self._need_data()
        return self._h.get_theta()

    def modelLogLikelihood(self):
        """UPLDA:1644-1758, on the device (ggs_model_log_likelihood): nothing is copied back but two doubles.
        model_log_likelihood() above is the host-side formula the tests check it against."""
        self._need_data()
        doc_side, topic_side = self._h.model_log_likelihood()
        return doc_side + topic_side

    def computeLogPosterior(self):
        """UPLDA:1573-1634 (Doss and George 2025), on the device (ggs_log_posterior)."""
        self._need_data()
        doc_side, topic_side = self._h.log_posterior()
        return doc_side + topic_side

    def minDocumentDistances(self):
        """"Quantity A" (UPLDA:723-753), on the device (ggs_min_doc_distances): per document the smallest Euclidean distance of
        its theta row to any other document's; scheme ggs on the thetaMatrix of the last z step, the pcgs family on the
        diagnostic theta draw the log posterior makes too (UPLDA:710-714).  One line of min_doc_distances.csv."""
        self._need_data()
        return self._h.min_doc_distances()

    def minTopicDistance(self):
        """"Quantity B" (UPLDA:778-806), on the device (ggs_min_topic_distance): the smallest Euclidean distance between two
        rows of Phi.  One line of min_topic_distances.csv."""
        self._need_data()
        return self._h.min_topic_distance()

    # ---- the topic summaries of LDAUtils.java:566-911, on the device-resident counts (ggs_top_words) ----
    def _top(self, kind, n, lam=0.6, words=True):
        self._need_data()
        n, V = int(n), self._corpus.num_types
        if n > V:                                                     # the Java IllegalArgumentException, LDAUtils.java:568-570
            raise ValueError("Asked for more words (%d) than there are types (unique words = noTypes = %d)." % (n, V))
        idx = self._h.top_words(kind, n, lam)
        if not words:
            return idx
        vocab = self._corpus.vocab
        if vocab is None:
            raise ValueError("the corpus has no vocabulary: getTopWordIndices returns the ids")
        return [[vocab[i] for i in row] for row in idx.tolist()]

    def getTopWordIndices(self, n):
        """LDAUtils.getTopWordIndices (:895-911): [K][n] word ids by falling count, equal counts by falling id."""
        return self._top("top", n, words=False)

    def getTopWords(self, n):
        """LDAUtils.getTopWords (:874-893), the rows of TopWords.txt (tui/ParallelLDA.java:272-283)."""
        return self._top("top", n)

    def getTopRelevanceWords(self, n, lam=None):
        """LDAUtils.getTopRelevanceWords (:566-590; Sievert & Shirley's relevance), the rows of RelevanceWords.txt
        (tui/ParallelLDA.java:285-296).  lam: the configuration's `lambda` unless given."""
        return self._top("relevance", n, getattr(self.config, "lambda_", 0.6) if lam is None else lam)

    def getTopDistinctiveWords(self, n):
        """LDAUtils.getTopDistinctiveWords (:592-617; Chuang, Manning & Heer's distinctiveness)."""
        return self._top("distinctive", n)

    def getTopSalientWords(self, n):
        """LDAUtils.getTopSalientWords (:619-644)."""
        return self._top("salient", n)

    def getK1ReWeightedWords(self, n):
        """LDAUtils.getK1ReWeightedWords (:752-801; Song et al.'s keyword re-ranking)."""
        return self._top("k1", n)

    def getTopicModelDiagnostics(self, n=None):
        """new TopicModelDiagnosticsPlain(model, n) on the device-resident z and counts (ggs_topic_doc_statistics,
        ggs_topic_scores): native.TopicDiagnostics with the eleven scores per topic, the word scores, the codocument matrices
        and topics_to_csv().  n: the configuration's nr_top_words unless given.  Unlike the Java (which reads word 0 for the
        positions beyond the vocabulary), n > V is refused: the driver clamps first."""
        self._need_data()
        n = int(getattr(self.config, "nr_top_words", 20) if n is None else n)
        V = self._corpus.num_types
        if n > V:
            raise ValueError("Asked for more words (%d) than there are types (unique words = noTypes = %d)." % (n, V))
        return self._h.topic_diagnostics(n, self._corpus.vocab)

    def getBeta(self):
        return self.beta

    def getAlpha(self):
        return self.alpha

    # ---- LDASamplerWithPhi ----
    def getPhi(self):
        self._need_data()
        return self._h.get_phi()                         # [K][V]

    def setPhi(self, phi, data_alphabet=None, target_alphabet=None):
        self._need_data()
        self._h.set_phi(np.asarray(phi, np.float64))

    def getPhiMeans(self):
        self._need_data()
        return self._h.get_phi_mean()[0]                 # None before the first accumulated sample, UPLDA:1955-1958

    def getNoSampledPhi(self):
        self._need_data()
        return self._h.get_phi_mean()[1]

    # ---- AbortableSampler ----
    def abort(self):
        self._abort = True                               # volatile flag, MSLDA:88,601-603

    def getAbort(self):
        return self._abort

    # ---- hooks (no-ops, MSLDA:783-810) ----
    def preIteration(self):
        pass

    def postIteration(self):
        pass

    def preSample(self):
        pass

    def postSample(self):
        pass

    def preZ(self):
        pass

    def postZ(self):
        pass

    def prePhi(self):
        pass

    def postPhi(self):
        pass

    def _need_data(self):
        if self._h is None:
            raise RuntimeError("addInstances has not been called")


class LDAPartiallyCollapsedGibbsSampler(LDAGroupedGibbsSampler):
    """scheme=pcgs (topics/LDAPartiallyCollapsedGibbsSampler.java): the same driver, counts and Phi draw;
    the z step is UPLDA:1466-1544 (theta integrated out, sequential inside a document).  SURVEY 8(f)-1."""
    _scheme_flags = native.FLAG_PCGS

    def getTheta(self):
        raise NotImplementedError("scheme=pcgs never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")


class PolyaUrnSpaliasLDA(LDAPartiallyCollapsedGibbsSampler):
    """scheme=polyaurn (topics/PolyaUrnSpaliasLDA.java, ParallelLDA.java:444-447): the pcgs driver and z step, with Phi drawn
    as Poisson counts normalised by their integer row sums (exact zeros) and a uniform topic for one-token documents and
    all-zero score rows (PolyaUrnSpaliasLDA.java:261-278).  Config key alias_poisson_threshold (default 100): counts below it
    draw from a table, larger ones from the normal approximation."""
    _scheme_flags = native.FLAG_POLYAURN

    def getTheta(self):
        raise NotImplementedError("scheme=polyaurn never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")


class SpaliasUncollapsedParallelLDA(LDAPartiallyCollapsedGibbsSampler):
    """scheme=spalias (topics/SpaliasUncollapsedParallelLDA.java, ParallelLDA.java:439-442): the pcgs model and driver; the z
    step draws from the pcgs conditional split into alpha_k * phi[k][w] (a Walker alias table per word, rebuilt with every
    Phi) and n_dk * phi[k][w] (a walk over the document's non-zero topics): O(nnz_d) per token instead of O(K)."""
    _scheme_flags = native.FLAG_SPALIAS

    def getTheta(self):
        raise NotImplementedError("scheme=spalias never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeNorm [V]) of the current Phi"""
        return self._h.alias_tables()


class SpaliasUncollapsedParallelWithPriors(SpaliasUncollapsedParallelLDA):
    """scheme=spalias_priors (topics/SpaliasUncollapsedParallelWithPriors.java, ParallelLDA.java:464-468; LDASamplerWithPriors):
    spalias with topic priors, "anchor words".  The cfg key topic_prior_filename names a file of lines `topic,word,word,...`
    (priors.py); those words may only belong to that topic, and Phi is exactly zero for them everywhere else: the initial Phi is
    multiplied by the priors, every later Phi is the conditional Dirichlet draw over each topic's allowed words.  With no file
    named it is spalias (haveTopicPriors == false)."""

    def _before_initial_state(self, training):
        self._topic_priors = None
        path = getattr(self.config, "topic_prior_filename", None)
        if path is None:
            return
        if training.vocab is None:
            raise ValueError("topic_prior_filename needs a corpus with a vocabulary (Corpus.vocab)")
        from . import priors
        topics, words = priors.load_zero_cells(path, self.numTopics, training.vocab)     # initializePriors, :170-189
        self._h.set_topic_priors(topics, words)
        self._topic_priors = (topics, words)

    def getTopicPriors(self):
        """double[K][V], 1.0 or 0.0 (LDASamplerWithPriors.getTopicPriors), read back from the device"""
        self._need_data()
        return self._h.get_topic_priors()


class LightPCLDA(LDAPartiallyCollapsedGibbsSampler):
    """scheme=lightpclda (topics/LightPCLDA.java, ParallelLDA.java:469-473): the pcgs model and driver and spalias's alias
    tables; the z step makes two Metropolis-Hastings proposals per token, one from the word's table and one from the
    document's own indicator array: O(1) per token.  The chain is approximate by design."""
    _scheme_flags = native.FLAG_LIGHTPCLDA

    def getTheta(self):
        raise NotImplementedError("scheme=lightpclda never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeNorm [V]) of the current Phi"""
        return self._h.alias_tables()

    def getMHStats(self):
        """tokens whose word proposal was kept, whose document proposal was accepted, left on their old topic (cumulative)"""
        return self._h.mh_stats()


class LightPCLDAtypeTopicProposal(LDAPartiallyCollapsedGibbsSampler):
    """scheme=lightpcldaw2 (topics/LightPCLDAtypeTopicProposal.java, ParallelLDA.createModel's "lightpcldaw2"): the pcgs model
    and driver -- Phi is drawn -- under the LightLDA z step with scheme=lightcollapsed's word proposal: the word's alias table
    over n_wk / (n_k + betaSum) on its non-zero topics plus a beta * K smoothing branch, the acceptance ratio correcting for it
    with Phi; then scheme=lightpclda's document proposal.  O(1) per token.  The tables are the ones the class declares
    (DESIGN.md 6m); the chain is approximate as written.  Constructed directly: create_model does not know the name
    (tests/test_lightcollapsed_model.py pins its refusal)."""
    _scheme_flags = native.FLAG_LIGHTPCLDAW2

    def getTheta(self):
        raise NotImplementedError("scheme=lightpcldaw2 never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeMass [V]) of the current counts: a word's table in the first nw[w] entries of its row"""
        self._need_data()
        return self._h.alias_tables()

    def getWordTopicLists(self):
        """(nw [V], topics [V][K]): per word the topics with n_wk > 0 in ascending order, -1 behind them"""
        self._need_data()
        return self._h.word_topic_lists()

    def getMHStats(self):
        """tokens whose word proposal was kept, whose document proposal was accepted, left on their old topic (cumulative)"""
        return self._h.mh_stats()


class PolyaUrnSparseLDA(LDAPartiallyCollapsedGibbsSampler):
    """scheme=polyaurn_sparse (the sampler topics/PolyaUrnSpaliasLDA.java builds, sampleTopicAssignmentsParallel :180-334):
    polyaurn's model -- Phi drawn as Poisson counts with exact zeros, config key alias_poisson_threshold -- with the doubly
    sparse z step: the alias table of the word for alpha_k * phi[k][w], and n_dk * phi[k][w] walked over the shorter of the
    word's list of non-zero topics and the document's: O(min(nnz_w, nnz_d)) per token."""
    _scheme_flags = native.FLAG_POLYAURN_SPARSE

    def getTheta(self):
        raise NotImplementedError("scheme=polyaurn_sparse never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeNorm [V]) of the current Phi"""
        return self._h.alias_tables()

    def getWordTopicLists(self):
        """(nw [V], topics [V][K]): per word the topics with phi != 0 in ascending order, -1 behind them"""
        return self._h.word_topic_lists()

    def getSparseStats(self):
        """tokens that walked the word's list, the document's list, tokens drawn uniformly, the sum of candidates (cumulative)"""
        return self._h.sparse_stats()


class NZVSSpaliasUncollapsedParallelLDA(LDAPartiallyCollapsedGibbsSampler):
    """scheme=nzvsspalias (topics/NZVSSpaliasUncollapsedParallelLDA.java over types/VSDirichlet.java): the pcgs model with a
    variable-selection Dirichlet for Phi -- a cell without tokens keeps or loses its place in the topic by a Bernoulli
    indicator, so Phi has exact zeros -- and the doubly sparse z step over the shorter of the word's list of drawn topics and
    the document's list.  Config key variable_selection_prior (default 0.5).  Constructed directly: create_model() keeps
    refusing the name "nzvsspalias" (tests/test_spalias_model.py pins that refusal)."""
    _scheme_flags = native.FLAG_NZVSSPALIAS

    def _before_initial_state(self, training):
        self._h.set_variable_selection_prior(self.config.variable_selection_prior)

    def getTheta(self):
        raise NotImplementedError("scheme=nzvsspalias never draws theta; use getThetaEstimate() (UPLDA:716-720 does the same)")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeNorm [V]) of the current Phi"""
        return self._h.alias_tables()

    def getWordTopicLists(self):
        """(nw [V], topics [V][K]): per word the topics whose cell the last Phi draw drew, ascending, -1 behind them"""
        return self._h.word_topic_lists()

    def getSparseStats(self):
        """tokens that walked the word's list, the document's list, tokens drawn from the alias table alone, the sum of candidates"""
        return self._h.sparse_stats()

    def getVSStats(self):
        """cells the last Phi draw left undrawn, zero cells of the current Phi, the most rounds a topic's indicator chain took"""
        return self._h.vs_stats()


class SerialCollapsedLDA(LDAGroupedGibbsSampler):
    """scheme=collapsed (topics/SerialCollapsedLDA.java; the conditional it samples from is sampleTopicsForOneDoc,
    MSLDA:158-226).  `schedule`:
      "serial"    the reference's own chain -- one pass over all tokens, counts moved in place, initial topics and
                  sampling uniforms from the ONE Randoms(seed) the Java class owns (SerialCollapsedLDA.java:60-65,789):
                  bit-identical to the restated Java loop, no parallelism across tokens (BASELINE config 1)
      "parallel"  documents side by side on the sweep-start counts, merged after the sweep (the AD-LDA decomposition):
                  the device-speed variant, approximate as ADLDA is
    No theta and no Phi are drawn: getPhi() is the point estimate (beta + n_wk)/(betaSum + n_k)."""
    _scheme_flags = native.FLAG_COLLAPSED
    _optimizes_hyperparameters = False   # as the Java class: hyperparam_optim_interval is ignored (ADLDA.java:387-391 optimises through MALLET internals that are not in the tree)

    def __init__(self, config, schedule="serial"):
        super().__init__(config)
        if schedule not in ("serial", "parallel"):
            raise ValueError("schedule must be 'serial' or 'parallel'")
        self.schedule = schedule

    def _z_half(self):
        if self.schedule == "serial":
            self._h.collapsed_serial_sweep(self.startSeed, 1)
        else:
            self._h.sweep_begin()

    def _phi_half(self):
        if self.schedule == "parallel":
            self._h.sweep_end()

    def getTheta(self):
        raise NotImplementedError("scheme=collapsed never draws theta; use getThetaEstimate()")

    def sampleZGivenPhi(self, iterations):
        raise NotImplementedError("scheme=collapsed has no Phi to condition on")


class CollapsedLightLDA(LDAGroupedGibbsSampler):
    """scheme=lightcollapsed (topics/CollapsedLightLDA.java, ParallelLDA.java:429-433): the collapsed model -- no theta and no
    Phi are drawn, getPhi() is the point estimate (beta + n_wk)/(betaSum + n_k) -- under the LightLDA z step: per token a
    word proposal from the word's alias table over the counts and a document proposal from the document's own indicator
    array, each accepted on a product of count quotients: O(1) per token.  Documents are sampled side by side on the
    sweep-start counts and merged after the sweep (the AD-LDA decomposition of scheme=collapsed's parallel schedule); the chain
    is approximate as the reference writes it."""
    _scheme_flags = native.FLAG_LIGHTCOLLAPSED
    _optimizes_hyperparameters = False   # as the Java class: hyperparam_optim_interval is ignored (ADLDA.java:387-391 optimises through MALLET internals that are not in the tree)

    def getTheta(self):
        raise NotImplementedError("scheme=lightcollapsed never draws theta; use getThetaEstimate()")

    def sampleZGivenPhi(self, iterations):
        raise NotImplementedError("scheme=lightcollapsed has no Phi to condition on")

    def getAliasTables(self):
        """(ps [V][K], a [V][K], typeMass [V]) of the current counts: a word's table in the first nw[w] entries of its row"""
        self._need_data()
        return self._h.alias_tables()

    def getWordTopicLists(self):
        """(nw [V], topics [V][K]): per word the topics with n_wk > 0 in ascending order, -1 behind them"""
        self._need_data()
        return self._h.word_topic_lists()

    def getMHStats(self):
        """tokens whose word proposal was kept, whose document proposal was accepted, left on their old topic (cumulative)"""
        return self._h.mh_stats()


class ADLDA(LDAGroupedGibbsSampler):
    """scheme=adlda (topics/ADLDA.java, ParallelLDA.java:409-412; MyWorkerRunnable.sampleTopicsForOneDoc): the collapsed model --
    no theta and no Phi are drawn, getPhi() is the point estimate (beta + n_wk)/(betaSum + n_k) -- under the SparseLDA bucket z
    step: the conditional split into a smoothing, a document and a word mass, walked over the document's and the word's
    non-zero topics only.  The exact conditional and the schedule of scheme=collapsed's parallel (AD-LDA) schedule, at
    O(nnz_d + nnz_w) per token.  Constructed directly: create_model does not know the name."""
    _scheme_flags = native.FLAG_ADLDA
    _optimizes_hyperparameters = False   # as the Java class: hyperparam_optim_interval is ignored (ADLDA.java:387-391 optimises through MALLET internals that are not in the tree)

    def getTheta(self):
        raise NotImplementedError("scheme=adlda never draws theta; use getThetaEstimate()")

    def sampleZGivenPhi(self, iterations):
        raise NotImplementedError("scheme=adlda has no Phi to condition on")

    def getWordTopicLists(self):
        """(nw [V], topics [V][K]): per word the topics with n_wk > 0 in ascending order, -1 behind them"""
        self._need_data()
        return self._h.word_topic_lists()

    def getSparseStats(self):
        """tokens drawn from the word bucket, the document bucket, the smoothing bucket; the sum of nnz_w + nnz_d (cumulative)"""
        return self._h.sparse_stats()


def create_model(config, scheme=None):
    """The `case "ggs"` / `case "pcgs"` / `case "collapsed"` / `case "lightcollapsed"` / `case "polyaurn"` / `case "spalias"` / `case "lightpclda"` of tui/ParallelLDA.createModel
    (ParallelLDA.java:401-490); "spalias_priors" is :464-468; "polyaurn_sparse" is this build's name for polyaurn over the sparse z step the reference's class holds.
    "adlda" (:409-412) is not in this registry, as "nzvsspalias" and "lightpcldaw2" are not (tests/test_host_mirror.py and
    tests/test_lightcollapsed_model.py pin the refusal of the names): construct ADLDA(config) / LightPCLDAtypeTopicProposal(config) itself."""
    scheme = scheme or config.scheme
    if scheme == "ggs":
        return LDAGroupedGibbsSampler(config)
    if scheme == "pcgs":
        return LDAPartiallyCollapsedGibbsSampler(config)
    if scheme == "collapsed":
        return SerialCollapsedLDA(config)
    if scheme == "polyaurn":
        return PolyaUrnSpaliasLDA(config)
    if scheme == "spalias":
        return SpaliasUncollapsedParallelLDA(config)
    if scheme == "spalias_priors":
        return SpaliasUncollapsedParallelWithPriors(config)
    if scheme == "lightpclda":
        return LightPCLDA(config)
    if scheme == "polyaurn_sparse":
        return PolyaUrnSparseLDA(config)
    if scheme == "lightcollapsed":
        return CollapsedLightLDA(config)
    raise ValueError("scheme %r is not provided by this build (only the ggs, pcgs, collapsed, lightcollapsed, polyaurn, spalias, spalias_priors, lightpclda and polyaurn_sparse z loops are in scope)" % scheme)
