"""Using a trained model on unseen documents: similarity/LDADistancer (behind tui/LDASimilarity) and
classify/KLDivergenceClassifier (behind tui/KLClassifier), with the distance classes of cc/mallet/similarity on the device
(csrc/ggs_similarity.hpp).

The metric registry is keyed by the Java class names (`DISTANCES`); `KolmogorovSmirnovDistance`, `TDistance` (commons-math3) and
`BM25Distance` (not a distance between topic vectors) are not part of it.

The fold-in is the reference's: a spalias sampler on the test documents, setPhi(trained.getPhi()), sampleZGivenPhi(n).  Java
builds one sampler per test document (LDADistancer.java:57-62, KLDivergenceClassifier.java:50-55); here all test documents
share one handle.  Given Phi the documents are independent, so every document's z has the same law as in Java -- but the
Philox stream of a token is keyed by its position in the shared corpus, not restarted per document, so the draws differ from a
one-document handle's.  (The reference's generator is clock-seeded: no run of it reproduces another either.)"""
import numpy as np

from . import _lib, native
from .corpus import Corpus
from .sampler import SpaliasUncollapsedParallelLDA

DISTANCES = dict(_lib.DISTANCE_IDS)
NEAREST_MAX = _lib.NEAREST_MAX
INF = float("inf")


def merge_nearest(lists, n):
    """The n nearest of the whole from the lists of its parts: `lists` holds (idx [Q][m], dist [Q][m]) pairs as
    GGSHandle.nearest_documents returns them (global indices, -1 / +inf padding).  The order is the kernels': distance rising by
    value (-0.0 == 0.0), then index rising; it is total, so any split of the documents merges to the list of the whole."""
    lists = [(np.asarray(i, np.int64), np.asarray(d, np.float64)) for i, d in lists]
    if not lists:
        raise ValueError("nothing to merge")
    Q = lists[0][0].shape[0]
    idx, dist = np.full((Q, int(n)), -1, np.int64), np.full((Q, int(n)), INF)
    for q in range(Q):
        cand = [(float(d) + 0.0, int(i), float(d)) for li, ld in lists for i, d in zip(li[q], ld[q]) if i >= 0 and d < INF]
        cand.sort(key=lambda c: c[:2])
        for r, (_, i, d) in enumerate(cand[:int(n)]):
            idx[q, r], dist[q, r] = i, d
    return idx, dist


def _fold_in(config, trained, test_corpus, sweeps):
    """the spalias sampler of the test documents under the trained Phi, after `sweeps` z-only sweeps"""
    if not isinstance(test_corpus, Corpus):
        raise TypeError("expects a ldagroupedgibbssampler_amd.corpus.Corpus read against the training alphabet")
    if test_corpus.num_types != trained.getNoTypes():
        raise ValueError("Alphabets on training and test sets do not match!")
    fold = SpaliasUncollapsedParallelLDA(config)
    fold.addInstances(test_corpus)
    fold.setPhi(trained.getPhi())
    fold.sampleZGivenPhi(int(sweeps))
    return fold


class LDADistancer:
    """similarity/LDADistancer.java: train a spalias model, fold unseen documents into its Phi, and measure each one's theta
    estimate against every training document's under a pluggable distance (default KLDistance, as in Java)."""

    def __init__(self, config):
        self.config = config
        self.dist = "KLDistance"
        self.trainedSampler = None
        self.sampledTestTopics = None
        self.folded = None                              # the fold-in sampler of the last distance() / nearest() call

    def getDist(self):
        return self.dist

    def setDist(self, dist):
        native.distance_id(dist)                        # raises on an unknown name
        self.dist = dist

    def train(self, corpus):
        """LDADistancer.train (:108-119): spalias for config.iterations; the handle stays on the device"""
        self.trainedSampler = SpaliasUncollapsedParallelLDA(self.config)
        self.trainedSampler.addInstances(corpus)
        self.trainedSampler.sample(self.config.iterations)
        return self.trainedSampler

    def getTrainedSampler(self):
        return self.trainedSampler

    def setTrainedSampler(self, sampler):
        """a sampler trained elsewhere (any scheme with a Phi) in the place of train()'s"""
        self.trainedSampler = sampler

    def getSampledTestTopics(self):
        """the theta estimates [Q][K] of the last test corpus (sampledTestTopics)"""
        return self.sampledTestTopics

    def _queries(self, test_corpus, fold_in_sweeps):
        if self.trainedSampler is None:
            raise ValueError("no trained model: call train first")
        self.folded = _fold_in(self.config, self.trainedSampler, test_corpus, fold_in_sweeps)
        self.sampledTestTopics = self.folded._h.theta_estimate()
        return self.sampledTestTopics, np.diff(test_corpus.doc_ptr).astype(np.int64)

    def distance(self, test_corpus, fold_in_sweeps=2000):
        """LDADistancer.distance (:55-106) for every test document: [Q][D], the empty-document rule included"""
        query, lens = self._queries(test_corpus, fold_in_sweeps)
        return self.trainedSampler._h.document_distances(query, self.dist, lens)

    def nearest(self, test_corpus, n=1, fold_in_sweeps=2000):
        """(idx [Q][n], dist [Q][n]): per test document the n nearest training documents; n = 1 is tui/LDASimilarity.java:175-183"""
        query, lens = self._queries(test_corpus, fold_in_sweeps)
        return self.trainedSampler._h.nearest_documents(query, n, self.dist, lens)


class KLDivergenceClassifier:
    """classify/KLDivergenceClassifier.java: class centroids of the training documents' z-bar, unseen documents scored by
    1 / symmetrised KL to each centroid.  crossValidate (MALLET's Trial / CrossValidationIterator) is not part of this."""

    def __init__(self, config):
        self.config = config
        self.alpha = config.alpha
        self.trainedSampler = None
        self.classes, self.centroidClasses, self.classCentroids = [], [], None
        self.sampledTestTopics = None
        self.folded = None

    def train(self, corpus, labels, label_alphabet=None):
        """train (:94-129).  `labels`: one class per document; `label_alphabet`: the target alphabet, every class in index order
        -- LoadedDataset.labels (indices into it) and LoadedDataset.label_alphabet.  The score columns of classify() follow it, as
        Java writes scores[targetAlphabet.lookupIndex(key)]; a class of the alphabet without a training document has no centroid
        and keeps the score 0.0 of Java's new double[].  Without an alphabet the classes are the labels in order of first
        appearance.  The centroids are calculateCentroids' (:154-186): per class the z-bar rows summed in document order, then
        (sum + alpha) / count."""
        labels = labels.tolist() if isinstance(labels, np.ndarray) else list(labels)
        if len(labels) != corpus.num_docs:
            raise ValueError("one label per training document")
        if label_alphabet is not None:
            label_alphabet = list(label_alphabet)
            labels = [label_alphabet[x] if isinstance(x, (int, np.integer)) else x for x in labels]
            if any(x not in label_alphabet for x in labels):
                raise ValueError("a label that is not in the label alphabet")
        self.trainedSampler = SpaliasUncollapsedParallelLDA(self.config)
        self.trainedSampler.addInstances(corpus)
        self.trainedSampler.sample(self.config.iterations)
        zbar = self.trainedSampler._h.zbar()
        seen, rows, counts = [], {}, {}
        for d, name in enumerate(labels):
            if name not in rows:
                seen.append(name)
                rows[name] = np.zeros(zbar.shape[1])
                counts[name] = 0
            counts[name] += 1
            rows[name] = rows[name] + zbar[d]
        self.classes = label_alphabet if label_alphabet is not None else seen
        self.centroidClasses = [c for c in self.classes if c in rows]          # the classes that have a centroid, in column order
        self.classCentroids = np.stack([(rows[c] + self.alpha) / float(counts[c]) for c in self.centroidClasses])
        return self.trainedSampler

    def getTrainedSampler(self):
        return self.trainedSampler

    def classify(self, test_corpus, fold_in_sweeps=300):
        """classify (:46-85) for every test document: (scores [Q][C], labels [Q]).  The query row is (zbar + alpha) / sum(zbar)
        with the sequential sum (MatrixOps.sum); scores = 1.0 / symmetrised KL(centroid, row) on the device; the label is the
        first maximum (a NaN score is never one).  The columns are self.classes."""
        if self.trainedSampler is None:
            raise ValueError("no trained model: call train first")
        self.folded = _fold_in(self.config, self.trainedSampler, test_corpus, fold_in_sweeps)
        zbar = self.folded._h.zbar()
        self.sampledTestTopics = zbar
        with np.errstate(all="ignore"):
            total = np.cumsum(zbar, axis=1)[:, -1]      # sequential, from 0.0: 0.0 + x is x
            rows = (zbar + self.alpha) / total[:, None]
            kl = native.row_distances(self.classCentroids, rows, "KLDistance", device_id=self.config.device_id)
            scores = np.zeros((zbar.shape[0], len(self.classes)))
            scores[:, [self.classes.index(c) for c in self.centroidClasses]] = 1.0 / kl
        labels = []
        for row in scores:
            best = 0
            for c in range(1, len(row)):
                if row[c] > row[best]:
                    best = c
            labels.append(self.classes[best])
        return scores, labels
