"""Thin numpy wrapper over the C-ABI (include/ggs_hip.h); one object = one ggs_handle."""
import ctypes as C

import numpy as np

from . import _lib

OK = 0
ERR_NEGATIVE_COUNT, ERR_INVALID_TOPIC, ERR_RNG_EXHAUSTED, ERR_BAD_ARG = 1, 2, 3, 4
ERR_HIP, ERR_STATE, ERR_UNSUPPORTED, ERR_INVARIANT = 5, 6, 7, 8
FLAG_PARANOID, FLAG_SAVE_PHI_MEAN, FLAG_PCGS, FLAG_COLLAPSED, FLAG_POLYAURN, FLAG_SPALIAS, FLAG_LIGHTPCLDA = 1, 2, 4, 8, 16, 32, 64
FLAG_POLYAURN_SPARSE = 128
FLAG_LIGHTCOLLAPSED = 256
FLAG_NZVSSPALIAS = 512
FLAG_ADLDA = 1024
FLAG_LIGHTPCLDAW2 = 2048   # sampler.LightPCLDAtypeTopicProposal: constructed directly, so not a key of SCHEME_FLAGS (create_model refuses the name)
# scheme name -> its flag, in the order of the library's scheme table (csrc/ggs_host_state.hpp, kSchemes)
SCHEME_FLAGS = {"ggs": 0, "pcgs": FLAG_PCGS, "collapsed": FLAG_COLLAPSED, "polyaurn": FLAG_POLYAURN, "spalias": FLAG_SPALIAS, "lightpclda": FLAG_LIGHTPCLDA,
                "polyaurn_sparse": FLAG_POLYAURN_SPARSE, "lightcollapsed": FLAG_LIGHTCOLLAPSED, "nzvsspalias": FLAG_NZVSSPALIAS, "adlda": FLAG_ADLDA}
PURPOSE_Z, PURPOSE_THETA, PURPOSE_PHI, PURPOSE_INIT_PHI = 1, 2, 3, 4
# the rankings of ggs_top_words (GGS_TOP_*), and its cap on the words per topic (GGS_TOP_WORDS_MAX)
TOP_KINDS = {"top": 0, "relevance": 1, "distinctive": 2, "salient": 3, "k1": 4}
TOP_WORDS_MAX = 128
# the columns of TopicModelDiagnosticsPlain.topicsToCsv in its order; ggs_topic_scores' rows are these without word-length
TOPIC_DIAGNOSTIC_NAMES = ("tokens", "document_entropy", "word-length", "coherence", "uniform_dist", "corpus_dist", "eff_num_words", "token-doc-diff",
                          "rank_1_docs", "allocation_ratio", "allocation_count")
TOPIC_SCORE_ROWS = tuple(x for x in TOPIC_DIAGNOSTIC_NAMES if x != "word-length")
TOPIC_WORD_SCORE_ROWS = ("coherence", "uniform_dist", "corpus_dist", "token-doc-diff")


class GGSError(RuntimeError):
    """A non-zero return of the C-ABI.  ERR_INVALID_TOPIC / ERR_NEGATIVE_COUNT are the
    IllegalStateExceptions of LDAGroupedGibbsSampler.java:84-85,116-118; ERR_BAD_ARG the
    IllegalArgumentExceptions."""

    def __init__(self, code, msg):
        super().__init__("ggs error %d: %s" % (code, msg))
        self.code = code


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _lp(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _make_config(num_topics, num_types, alpha, beta, seed, device_id, flags, phi_burn_in, phi_mean_thin, alias_poisson_threshold=0):
    """(ggs_config, the alpha array it points into -- keep it alive for the duration of the call)"""
    cfg = _lib.GGSConfig()
    cfg.struct_size = C.sizeof(_lib.GGSConfig)
    cfg.num_topics, cfg.num_types, cfg.device_id = int(num_topics), int(num_types), int(device_id)
    alpha = np.asarray(alpha, np.float64)
    keep = None
    if alpha.ndim == 0:
        cfg.alpha = None
        cfg.alpha_scalar = float(alpha)
    else:
        keep = np.ascontiguousarray(alpha)
        if keep.size != int(num_topics):
            raise ValueError("alpha must have num_topics entries")
        cfg.alpha = _dp(keep)
    cfg.beta = float(beta)
    cfg.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    cfg.flags, cfg.phi_burn_in, cfg.phi_mean_thin = int(flags), int(phi_burn_in), int(phi_mean_thin)
    cfg.alias_poisson_threshold = int(alias_poisson_threshold)      # FLAG_POLYAURN, FLAG_POLYAURN_SPARSE only; 0 = the default 100
    return cfg, keep


def rccl_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 creates it; every rank passes it to GGSHandle.attach_rccl)."""
    _lib.share_rccl_with_torch()
    buf = C.create_string_buffer(128)
    rc = _lib.load().ggs_rccl_unique_id(C.cast(buf, C.c_void_p))
    if rc:
        raise GGSError(rc, "ggs_rccl_unique_id failed (librccl not loadable?)")
    return buf.raw


def _top_kind(kind):
    if isinstance(kind, str):
        if kind not in TOP_KINDS:
            raise ValueError("kind must be one of %s" % ", ".join(TOP_KINDS))
        return TOP_KINDS[kind]
    return int(kind)


class TopicDiagnostics:
    """What `new TopicModelDiagnosticsPlain(model, n)` holds (topics/TopicModelDiagnosticsPlain.java): ``names`` (the columns of
    topicsToCsv in its order), ``scores[name]`` ([K] doubles), ``word_scores[name]`` ([K][n], for coherence, uniform_dist,
    corpus_dist, token-doc-diff and -- with an alphabet -- word-length), ``idx`` ([K][n] top word ids), the document statistics
    ``codoc`` / ``doc_stats`` / ``clogc``.  word-length needs the words themselves: without an alphabet that column is left out
    of ``names`` (and of the CSV) instead of being filled with NaNs."""

    def __init__(self, idx, codoc, doc_stats, clogc, topic_scores, word_scores, alphabet=None):
        self.idx, self.codoc, self.doc_stats, self.clogc = idx, codoc, doc_stats, clogc
        self.n = idx.shape[1]
        self.scores = dict(zip(TOPIC_SCORE_ROWS, topic_scores))
        self.word_scores = dict(zip(TOPIC_WORD_SCORE_ROWS, word_scores)) if word_scores is not None else {}
        if alphabet is not None:                                  # getWordLengthScores (:399-418): String.length() is UTF-16 code units
            lengths = np.array([[len(alphabet[i].encode("utf-16-le")) // 2 for i in row] for row in idx.tolist()], np.float64)
            self.word_scores["word-length"] = lengths
            self.scores["word-length"] = np.array([float(int(r.sum())) for r in lengths]) / float(self.n)
        self.names = tuple(x for x in TOPIC_DIAGNOSTIC_NAMES if x in self.scores)

    def codocument_matrix(self, k):
        """getCodocumentMatrix(topic): [n][n], the diagonal = documents with the word under the topic"""
        return self.codoc[k]

    def topics_to_csv(self):
        from . import formats
        return formats.format_topic_diagnostics_csv(self.names, [self.scores[x] for x in self.names])


class GGSHandle:
    def __init__(self, num_topics, num_types, alpha, beta, seed, device_id=0, flags=0, phi_burn_in=0, phi_mean_thin=1, _adopt=None,
                 alias_poisson_threshold=0):
        self._L = _lib.load()
        self.K, self.V = int(num_topics), int(num_types)
        self.D = self.N = 0
        self._owned = _adopt is None
        self._keep = []
        if _adopt is not None:             # a handle created by ggs_group_create
            self._h = _adopt
            return
        cfg, self._alpha = _make_config(num_topics, num_types, alpha, beta, seed, device_id, flags, phi_burn_in, phi_mean_thin,
                                        alias_poisson_threshold)
        h = C.c_void_p()
        rc = self._L.ggs_create(C.byref(cfg), C.byref(h))
        if rc:
            raise GGSError(rc, "ggs_create failed")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if self._owned:
                self._L.ggs_destroy(self._h)
            self._h = None

    # ---- multi-GPU exchange (attach before set_corpus) ----
    def attach_rccl(self, rank, nranks, unique_id):
        """ncclCommInitRank on this handle's device: every rank of the job calls this together."""
        _lib.share_rccl_with_torch()
        uid = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.ggs_attach_rccl(self._h, int(rank), int(nranks), C.cast(uid, C.c_void_p)))

    def attach_null_exchange(self, rank, nranks):
        """Timing aid only (results are wrong by construction): rank `rank` of `nranks` with the peers missing."""
        self._chk(self._L.ggs_attach_null_exchange(self._h, int(rank), int(nranks)))

    def attach_exchange(self, rank, nranks, reduce_scatter_i32, all_gather_f64, all_gather_i32, all_to_all_v_i32=None):
        """Caller-supplied transport: three callables (send_ptr, recv_ptr, count, hip_stream_ptr) -> 0 on success, and
        optionally the one of the sparse count exchange: (send_ptr, send_offsets, send_counts, recv_ptr, recv_offsets,
        recv_counts, hip_stream_ptr) with the four lists in int32 elements, one entry per rank."""
        def wrap(fn):
            def cb(_ctx, send, recv, count, stream):
                try:
                    return int(fn(send, recv, count, stream) or 0)
                except Exception:          # an exception must not unwind through the C frame
                    import traceback
                    traceback.print_exc()
                    return 1
            return _lib.EXCHANGE_CB(cb)
        ops = _lib.GGSExchangeOps()
        ops.struct_size = C.sizeof(_lib.GGSExchangeOps)
        ops.reduce_scatter_i32, ops.all_gather_f64, ops.all_gather_i32 = wrap(reduce_scatter_i32), wrap(all_gather_f64), wrap(all_gather_i32)
        if all_to_all_v_i32 is not None:
            def a2a(_ctx, send, soff, scnt, recv, roff, rcnt, stream):
                try:
                    n = int(nranks)
                    return int(all_to_all_v_i32(send, [soff[i] for i in range(n)], [scnt[i] for i in range(n)], recv, [roff[i] for i in range(n)],
                                                [rcnt[i] for i in range(n)], stream) or 0)
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 1
            ops.all_to_all_v_i32 = _lib.A2AV_CB(a2a)
        self._keep.append(ops)             # the library copies the table, the thunks must outlive the handle
        self._chk(self._L.ggs_attach_exchange(self._h, int(rank), int(nranks), C.byref(ops)))

    def set_count_exchange(self, mode):
        """How the counts travel: "auto" (sparse where the dense buffer is large and mostly zero), "dense", "sparse"."""
        self._chk(self._L.ggs_set_count_exchange(self._h, {"auto": 0, "dense": 1, "sparse": 2}[mode]))

    def count_exchange(self):
        sp, pairs, cells = C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self._L.ggs_get_count_exchange(self._h, C.byref(sp), C.byref(pairs), C.byref(cells)))
        return {"sparse": bool(sp.value), "pairs_last": pairs.value, "dense_cells": cells.value}

    def exchange_info(self):
        r, n, a, b = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.ggs_get_exchange_info(self._h, C.byref(r), C.byref(n), C.byref(a), C.byref(b)))
        p, cn, cr = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.ggs_get_exchange_provider(self._h, C.byref(p), C.byref(cn), C.byref(cr)))
        return {"rank": r.value, "nranks": n.value, "k_begin": a.value, "k_end": b.value,
                "provider": {0: "none", 1: "rccl", 2: "callbacks", 3: "null (timing aid)"}.get(p.value, str(p.value)),
                "comm_nranks": cn.value, "comm_rank": cr.value}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc:
            raise GGSError(rc, self._L.ggs_last_error(self._h).decode())

    # ---- corpus / state ----
    def set_stream(self, stream_ptr):
        self._chk(self._L.ggs_set_stream(self._h, C.c_void_p(stream_ptr)))

    def set_corpus(self, doc_ptr, tokens, doc_base=0, tok_base=0):
        doc_ptr = np.ascontiguousarray(doc_ptr, np.int64)
        tokens = np.ascontiguousarray(tokens, np.int32)
        self._chk(self._L.ggs_set_corpus(self._h, doc_ptr.size - 1, _lp(doc_ptr), _ip(tokens), int(doc_base), int(tok_base)))
        self.D, self.N = doc_ptr.size - 1, int(doc_ptr[-1])

    def init_z_java_lcg(self, seed):
        self._chk(self._L.ggs_init_z_java_lcg(self._h, int(seed)))

    def set_z(self, z, redraw_phi=True):
        z = np.ascontiguousarray(z, np.int32)
        if z.size != self.N:
            raise ValueError("z must have one entry per token")
        self._chk(self._L.ggs_set_z(self._h, _ip(z), int(bool(redraw_phi))))

    def init_phi(self):
        self._chk(self._L.ggs_init_phi(self._h))

    def set_iteration(self, it):
        self._chk(self._L.ggs_set_iteration(self._h, int(it)))

    @property
    def iteration(self):
        it = C.c_int32()
        self._chk(self._L.ggs_get_iteration(self._h, C.byref(it)))
        return it.value

    # ---- sweeps ----
    def sweep(self, n=1):
        self._chk(self._L.ggs_sweep(self._h, int(n)))

    def collapsed_serial_sweep(self, java_seed, n=1):
        """SerialCollapsedLDA's own schedule (MSLDA:158-226, one chain, java.util.Random(java_seed)); needs FLAG_COLLAPSED."""
        self._chk(self._L.ggs_collapsed_serial_sweep(self._h, int(java_seed), int(n)))

    def sweep_begin(self):
        self._chk(self._L.ggs_sweep_begin(self._h))

    def sweep_end_async(self):
        self._chk(self._L.ggs_sweep_end_async(self._h))

    def sweep_end(self):
        self._chk(self._L.ggs_sweep_end(self._h))

    def sample_z_given_phi(self, n=1):
        self._chk(self._L.ggs_sample_z_given_phi(self._h, int(n)))

    def synchronize(self):
        self._chk(self._L.ggs_synchronize(self._h))

    def counts_device_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.ggs_counts_device_ptr(self._h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def set_global_token_count(self, n):
        self._chk(self._L.ggs_set_global_token_count(self._h, int(n)))

    # ---- getters ----
    def get_z(self):
        out = np.empty(self.N, np.int32)
        self._chk(self._L.ggs_get_z(self._h, _ip(out)))
        return out

    def get_type_topic_counts(self):
        out = np.empty((self.V, self.K), np.int32)
        self._chk(self._L.ggs_get_type_topic_counts(self._h, _ip(out)))
        return out

    def get_topic_totals(self):
        out = np.empty(self.K, np.int32)
        self._chk(self._L.ggs_get_topic_totals(self._h, _ip(out)))
        return out

    def get_phi(self):
        out = np.empty((self.K, self.V), np.float64)
        self._chk(self._L.ggs_get_phi(self._h, _dp(out)))
        return out

    def set_phi(self, phi):
        phi = np.ascontiguousarray(phi, np.float64)
        if phi.shape != (self.K, self.V):
            raise ValueError("phi must be [K][V]")
        self._chk(self._L.ggs_set_phi(self._h, _dp(phi)))

    def get_phi_mean(self):
        out = np.empty((self.K, self.V), np.float64)
        n = C.c_int32()
        self._chk(self._L.ggs_get_phi_mean(self._h, _dp(out), C.byref(n)))
        return (out, n.value) if n.value else (None, 0)

    def alias_tables(self):
        """scheme=spalias, lightpclda or polyaurn_sparse: the alias tables of the current Phi, (ps [V][K], a [V][K], type_norm [V]).
        scheme=lightcollapsed and lightpcldaw2: the tables of the current counts (what the next sweep builds at its head): row w holds the word's
        table in its first nw[w] entries, ps = 1.0 and a = the index behind them; type_norm [V] = typeMass."""
        ps, a, tn = np.empty((self.V, self.K), np.float64), np.empty((self.V, self.K), np.int32), np.empty(self.V, np.float64)
        self._chk(self._L.ggs_get_alias_tables(self._h, _dp(ps), _ip(a), _dp(tn)))
        return ps, a, tn

    def set_topic_priors(self, topics, words):
        """scheme=spalias_priors: the cells (topics[i], words[i]) of Phi are pinned to zero ("anchor words"); a FLAG_SPALIAS handle,
        before its first Phi.  Empty lists are allowed: the conditional Phi draw over an all-ones prior matrix."""
        topics, words = np.ascontiguousarray(topics, np.int32).ravel(), np.ascontiguousarray(words, np.int32).ravel()
        if topics.size != words.size:
            raise ValueError("one word per topic")
        self._chk(self._L.ggs_set_topic_priors(self._h, topics.size, _ip(topics), _ip(words)))

    def get_topic_priors(self):
        """getTopicPriors: [K][V], 1.0 or 0.0 (all 1.0 when no priors were set)."""
        out = np.empty((self.K, self.V), np.float64)
        self._chk(self._L.ggs_get_topic_priors(self._h, _dp(out)))
        return out

    def mh_stats(self):
        """scheme=lightpclda, lightcollapsed and lightpcldaw2: tokens whose word proposal was accepted and kept, whose document proposal was accepted, and
        tokens left on their old topic, cumulative since set_corpus (int64 [3]; they sum to the tokens sampled)."""
        out = np.zeros(3, np.int64)
        self._chk(self._L.ggs_get_mh_stats(self._h, _lp(out)))
        return out

    def word_topic_lists(self):
        """scheme=polyaurn_sparse: (nw [V], topics [V][K]) of the current Phi -- per word the number of topics with
        phi[k][w] != 0 and those topics in ascending order, -1 behind them.  scheme=lightcollapsed and lightpcldaw2: of the current counts, the
        topics with n_wk > 0; scheme=adlda: the same lists of the current counts."""
        nw, topics = np.empty(self.V, np.int32), np.empty((self.V, self.K), np.int32)
        self._chk(self._L.ggs_get_word_topic_lists(self._h, _ip(nw), _ip(topics)))
        return nw, topics

    def sparse_stats(self):
        """scheme=polyaurn_sparse: tokens that walked the word's list, the document's list, tokens drawn uniformly (no
        candidate) and the sum of the candidates' number over all tokens, cumulative since set_corpus (int64 [4]).  scheme=adlda:
        tokens drawn from the word bucket Q, the document bucket R, the smoothing bucket S, and the sum of nnz_w + nnz_d."""
        out = np.zeros(4, np.int64)
        self._chk(self._L.ggs_get_sparse_stats(self._h, _lp(out)))
        return out

    def set_variable_selection_prior(self, pi):
        """scheme=nzvsspalias: the prior probability that a cell without tokens keeps its place in its topic (0.5 until set); a
        FLAG_NZVSSPALIAS handle, before its first Phi."""
        self._chk(self._L.ggs_set_variable_selection_prior(self._h, float(pi)))

    def vs_stats(self):
        """scheme=nzvsspalias: the cells the last Phi draw left undrawn, the cells of the current Phi that are 0.0 and the largest
        number of rounds a topic's indicator chain took in that draw (int64 [3])."""
        out = np.zeros(3, np.int64)
        self._chk(self._L.ggs_get_vs_stats(self._h, _lp(out)))
        return out

    def get_theta(self, doc_begin=0, doc_end=None):
        doc_end = self.D if doc_end is None else doc_end
        out = np.empty((doc_end - doc_begin, self.K), np.float64)
        self._chk(self._L.ggs_get_theta(self._h, doc_begin, doc_end, _dp(out)))
        return out

    def get_doc_topic_counts(self, doc_begin=0, doc_end=None):
        doc_end = self.D if doc_end is None else doc_end
        out = np.empty((doc_end - doc_begin, self.K), np.int32)
        self._chk(self._L.ggs_get_doc_topic_counts(self._h, doc_begin, doc_end, _ip(out)))
        return out

    # ---- the hyperparameter step (optimizeAlpha / optimizeBeta, MSLDA:812-905) ----
    def doc_topic_histogram(self, symmetric, n_bins, lengths=True, out=None, lengths_out=None):
        """(topicDocCounts, docLengthCounts) of this handle's documents from the device: int32 [K][n_bins] (symmetric: [1][n_bins]) and
        int32 [n_bins] (None with lengths=False).  n_bins must exceed every n_dk (and length): ERR_BAD_ARG otherwise, outputs untouched."""
        rows = 1 if symmetric else self.K
        hist = np.empty((rows, int(n_bins)), np.int32) if out is None else out
        lens = (np.empty(int(n_bins), np.int32) if lengths_out is None else lengths_out) if lengths else None
        self._chk(self._L.ggs_doc_topic_histogram(self._h, 1 if symmetric else 0, int(n_bins), _ip(hist), _ip(lens) if lengths else None))
        return hist, lens

    def type_topic_count_histogram(self, n_bins, out=None):
        """countHistogram over the corpus-wide counts: int32 [n_bins], hist[c] = cells with n_wk == c (collective with an exchange)."""
        hist = np.empty(int(n_bins), np.int32) if out is None else out
        self._chk(self._L.ggs_type_topic_count_histogram(self._h, int(n_bins), _ip(hist)))
        return hist

    def set_hyperparameters(self, alpha, beta, beta_sum=0.0):
        """alpha: K values or None (keep); beta_sum: the Java field betaSum, 0.0 for beta * V.  From the next z step on the handle is
        a handle created with these values and given this one's state."""
        a = None if alpha is None else np.ascontiguousarray(alpha, np.float64)
        if a is not None and a.shape != (self.K,):
            raise ValueError("alpha must have num_topics entries")
        self._chk(self._L.ggs_set_hyperparameters(self._h, None if a is None else _dp(a), float(beta), float(beta_sum)))

    def hyperparameters(self):
        """(alpha [K], beta, betaSum): the current values"""
        a = np.empty(self.K, np.float64)
        b, bs = C.c_double(), C.c_double()
        self._chk(self._L.ggs_get_hyperparameters(self._h, _dp(a), C.byref(b), C.byref(bs)))
        return a, b.value, bs.value

    def get_timings(self):
        t = _lib.GGSTimings()
        self._chk(self._L.ggs_get_timings(self._h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in t._fields_}

    def reset_timings(self):
        self._chk(self._L.ggs_reset_timings(self._h))

    def check_invariants(self):
        self._chk(self._L.ggs_check_invariants(self._h))

    def model_log_likelihood(self):
        """(document side, topic side) of modelLogLikelihood (UPLDA:1644-1758), computed on the device."""
        a, b = C.c_double(), C.c_double()
        self._chk(self._L.ggs_model_log_likelihood(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def log_posterior(self):
        """(document side, topic side) of computeLogPosterior (UPLDA:1573-1634), computed on the device."""
        a, b = C.c_double(), C.c_double()
        self._chk(self._L.ggs_log_posterior(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def min_doc_distances(self, other=None):
        """min_doc_distances.csv (UPLDA:723-753), on the device: per document of this handle the smallest Euclidean distance
        of its theta row to every other row (other=None: the reference's loop), or to the rows of the foreign block
        `other` [n][K] (a doc-sharded run: once with None, once per foreign shard, element-wise minimum).  1e20 without a partner."""
        out = np.empty(self.D, np.float64)
        if other is None:
            op, n = None, 0
        else:
            other = np.ascontiguousarray(other, np.float64)
            if other.ndim != 2 or other.shape[1] != self.K:
                raise ValueError("other must be [n][K]")
            op, n = _dp(other), other.shape[0]
        self._chk(self._L.ggs_min_doc_distances(self._h, op, n, _dp(out)))
        return out

    def min_topic_distance(self):
        """min_topic_distances.csv (UPLDA:778-806), on the device: the smallest Euclidean distance between two rows of Phi."""
        v = C.c_double()
        self._chk(self._L.ggs_min_topic_distance(self._h, C.byref(v)))
        return v.value

    # ---- the nearest training documents (similarity/LDADistancer, tui/LDASimilarity; csrc/ggs_similarity.hpp) ----
    def theta_estimate(self, doc_begin=0, doc_end=None):
        """getThetaEstimate (MSLDA:709-753) of the handle's documents from the device-resident z and the current alpha: [n][K]"""
        doc_end = self.D if doc_end is None else doc_end
        out = np.empty((doc_end - doc_begin, self.K), np.float64)
        self._chk(self._L.ggs_get_theta_estimate(self._h, doc_begin, doc_end, _dp(out)))
        return out

    def zbar(self, doc_begin=0, doc_end=None):
        """getZbar (MSLDA:647-668) of the handle's documents from the device-resident z: [n][K], zeros for an empty document"""
        doc_end = self.D if doc_end is None else doc_end
        out = np.empty((doc_end - doc_begin, self.K), np.float64)
        self._chk(self._L.ggs_get_zbar(self._h, doc_begin, doc_end, _dp(out)))
        return out

    def _queries(self, query, query_len):
        query = np.ascontiguousarray(query, np.float64)
        if query.ndim != 2 or query.shape[1] != self.K:
            raise ValueError("query must be [Q][K]")
        if query_len is not None:
            query_len = np.ascontiguousarray(query_len, np.int64)
            if query_len.shape != (query.shape[0],):
                raise ValueError("query_len must have one entry per query")
        return query, query_len

    def nearest_documents(self, query, n=1, metric="KLDistance", query_len=None):
        """(idx int64 [Q][n], dist [Q][n]): per query row the n training documents of this handle with the smallest distance of
        the class `metric` (a Java class name of cc/mallet/similarity, or its id) between their theta estimate (v1) and the
        query (v2), ordered by (distance, global document index); -1 and +inf where fewer have a finite distance.  query_len:
        the queries' token counts for the empty-document rule of LDADistancer.java:84-87 (None: none is empty)."""
        query, query_len = self._queries(query, query_len)
        idx = np.empty((query.shape[0], int(n)), np.int64)
        dist = np.empty((query.shape[0], int(n)), np.float64)
        self._chk(self._L.ggs_nearest_documents(self._h, distance_id(metric), _dp(query), None if query_len is None else _lp(query_len), query.shape[0], int(n),
                                                _lp(idx), _dp(dist)))
        return idx, dist

    def document_distances(self, query, metric="KLDistance", query_len=None):
        """dist [Q][D]: what LDADistancer.distance returns per query row (LDADistancer.java:79-99), on the device"""
        query, query_len = self._queries(query, query_len)
        dist = np.empty((query.shape[0], self.D), np.float64)
        self._chk(self._L.ggs_document_distances(self._h, distance_id(metric), _dp(query), None if query_len is None else _lp(query_len), query.shape[0], _dp(dist)))
        return dist

    def top_words(self, kind, n, lam=0.6, scores=False):
        """The n best words of every topic (ggs_top_words) on the corpus-wide counts: idx [K][n] in IDSorter's order (falling
        score, ties by falling id); kind = "top" (LDAUtils.getTopWords, TopWords.txt), "relevance" (getTopRelevanceWords with
        lambda = lam, RelevanceWords.txt), "distinctive", "salient" or "k1".  scores=True: (idx, score [K][n])."""
        idx = np.empty((self.K, int(n)), np.int32)
        sc = np.empty((self.K, int(n)), np.float64) if scores else None
        self._chk(self._L.ggs_top_words(self._h, _top_kind(kind), int(n), float(lam), _ip(idx), _dp(sc) if scores else None))
        return (idx, sc) if scores else idx

    def top_words_phases(self, kind, n, lam=0.6, element_chain=False):
        """Device milliseconds of one top_words call by phase (ggs_debug_top_words_phases): mass_k, total, the words'
        statistics, selection and merge.  element_chain: the column sums by the one-lane chain kernel."""
        ms = np.zeros(4, np.float64)
        self._chk(self._L.ggs_debug_top_words_phases(self._h, _top_kind(kind), int(n), float(lam), int(bool(element_chain)), _dp(ms)))
        return dict(zip(("mass_k", "total", "words", "select_merge"), ms.tolist()))

    def topic_doc_statistics(self, n, idx=None, clogc_in=None):
        """collectDocumentStatistics of TopicModelDiagnosticsPlain over THIS handle's documents (ggs_topic_doc_statistics):
        (codoc [K][n][n] int32, doc_stats [K][9] int32 = nonzero, rank1, at_prop[7], clogc [K]).  idx [K][n]: the corpus-wide top
        words (default: this handle's own top_words("top", n)); clogc_in: the chain value the shards before this one left."""
        n = int(n)
        if idx is not None:
            idx = np.ascontiguousarray(idx, np.int32)
            if idx.shape != (self.K, n):
                raise ValueError("idx must be [K][n]")
        if clogc_in is not None:
            clogc_in = np.ascontiguousarray(clogc_in, np.float64)
            if clogc_in.shape != (self.K,):
                raise ValueError("clogc_in must be [K]")
        m = max(n, 0)
        codoc, stats, clogc = np.empty((self.K, m, m), np.int32), np.empty((self.K, 9), np.int32), np.empty(self.K, np.float64)
        self._chk(self._L.ggs_topic_doc_statistics(self._h, n, _ip(idx) if idx is not None else None, _dp(clogc_in) if clogc_in is not None else None,
                                                   _ip(codoc), _ip(stats), _dp(clogc)))
        return codoc, stats, clogc

    def topic_scores(self, n, idx, codoc, doc_stats, clogc, word_scores=False):
        """The topic scores from the corpus-wide counts and the (summed) document statistics (ggs_topic_scores): [10][K] in
        TOPIC_SCORE_ROWS' order; word_scores=True: (that, [4][K][n] in TOPIC_WORD_SCORE_ROWS' order)."""
        n = int(n)
        m = max(n, 0)
        idx, codoc = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(codoc, np.int32)
        doc_stats, clogc = np.ascontiguousarray(doc_stats, np.int32), np.ascontiguousarray(clogc, np.float64)
        if idx.shape != (self.K, m) or codoc.shape != (self.K, m, m) or doc_stats.shape != (self.K, 9) or clogc.shape != (self.K,):
            raise ValueError("idx [K][n], codoc [K][n][n], doc_stats [K][9], clogc [K]")
        ts = np.empty((len(TOPIC_SCORE_ROWS), self.K), np.float64)
        ws = np.empty((len(TOPIC_WORD_SCORE_ROWS), self.K, m), np.float64) if word_scores else None
        self._chk(self._L.ggs_topic_scores(self._h, n, _ip(idx), _ip(codoc), _ip(doc_stats), _dp(clogc), _dp(ts), _dp(ws) if word_scores else None))
        return (ts, ws) if word_scores else ts

    def topic_diagnostics(self, n, alphabet=None):
        """TopicModelDiagnosticsPlain(model, n) of a one-handle run: top words, document statistics, scores -> TopicDiagnostics.
        alphabet (the words by id) adds the word-length column; without it that column is left out."""
        idx = self.top_words("top", n)
        codoc, stats, clogc = self.topic_doc_statistics(n, idx)
        ts, ws = self.topic_scores(n, idx, codoc, stats, clogc, word_scores=True)
        return TopicDiagnostics(idx, codoc, stats, clogc, ts, ws, alphabet)

    def topic_diagnostics_phases(self, n):
        """Device milliseconds of topic_doc_statistics + topic_scores by phase (ggs_debug_topic_diagnostics_phases)."""
        ms = np.zeros(7, np.float64)
        self._chk(self._L.ggs_debug_topic_diagnostics_phases(self._h, int(n), _dp(ms)))
        return dict(zip(("membership", "document_pass", "column_statistics", "clogc_chain", "totals", "sort_and_sorted_chains", "small_scores"), ms.tolist()))

    def set_test_corpus(self, doc_ptr, tokens, doc_base=0):
        """addTestInstances (MSLDA:918-923): the held-out estimator's test set; ids >= num_types are out of vocabulary."""
        doc_ptr = np.ascontiguousarray(doc_ptr, np.int64)
        tokens = np.ascontiguousarray(tokens, np.int32)
        self._test_docs = doc_ptr.size - 1
        self._chk(self._L.ggs_set_test_corpus(self._h, self._test_docs, doc_ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                              tokens.ctypes.data_as(C.POINTER(C.c_int32)), int(doc_base)))

    def heldout_log_likelihood(self, num_particles=100):
        """MarginalProbEstimatorPlain.evaluateLeftToRight (MPE:85-121) on the current counts, on the device:
        (total, per-document values)."""
        doc_ll = np.zeros(getattr(self, "_test_docs", 0), np.float64)
        tot = C.c_double()
        self._chk(self._L.ggs_heldout_log_likelihood(self._h, int(num_particles), doc_ll.ctypes.data_as(C.POINTER(C.c_double)), C.byref(tot)))
        return tot.value, doc_ll

    def launch_info(self):
        c, l, b, nh, zp = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.ggs_get_launch_info(self._h, C.byref(c), C.byref(l), C.byref(b)))
        self._chk(self._L.ggs_get_num_hot_words(self._h, C.byref(nh)))
        self._chk(self._L.ggs_get_z_parts(self._h, C.byref(zp)))
        zk, zf, zc = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.ggs_get_z_form(self._h, C.byref(zk), C.byref(zf), C.byref(zc)))
        wt, ww, wd = C.c_int32(), C.c_int32(), C.c_int32()
        self._chk(self._L.ggs_get_warm_tiers(self._h, C.byref(wt), C.byref(ww), C.byref(wd)))
        hp, hc, hn, ht = C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self._L.ggs_get_hot_pairs(self._h, C.byref(hp), C.byref(hc), C.byref(hn), C.byref(ht)))
        zname = "z_sliced_kernel + z_pairs_kernel (score registers)" if zk.value == 1 and hp.value else Z_KERNEL_NAMES.get(zk.value, str(zk.value))
        return {"num_chunks": c.value, "lds_bytes_z": l.value, "docs_per_block_theta": b.value, "num_hot": nh.value, "z_parts": zp.value,
                "warm_tiers": wt.value, "num_warm": ww.value, "warm_docs_per_chunk": wd.value,
                "hot_pairs": bool(hp.value), "hot_pair_chunks": hc.value, "hot_pairs_per_token": (hn.value / ht.value) if ht.value else 0.0,
                "z_kernel": zname + (" + z_warm_kernel (%d tiers)" % wt.value if wt.value else ""), "z_form": {0: "n/a", 1: "split", 2: "fused"}.get(zf.value, str(zf.value)),
                "z_form_calibrated": bool(zc.value)}


Z_KERNEL_NAMES = {0: "z_kernel (whole-row tiles)", 1: "z_sliced_kernel + z_hot_kernel (score registers)", 2: "z_stream1_kernel (one pass)",
                  3: "z_stream_kernel (two passes)", 4: "pcgs_sliced_kernel (lane per document)", 5: "pcgs_wave_kernel (wave per document)",
                  6: "spalias_wave_kernel (wave per document)", 7: "lightpc_wave_kernel (wave per document)",
                  8: "polyaurn_sparse_wave_kernel (wave per document)", 9: "lightcollapsed_wave_kernel (wave per document)",
                  10: "nzvs_wave_kernel (wave per document)", 11: "adlda_wave_kernel (wave per document)", 12: "lightpcw2_wave_kernel (wave per document)"}


class GGSGroup:
    """ONE process driving several GPUs (ggs_group_create): the handles of the group in rank order, joined by
    ncclCommInitAll; sweeps are issued for all devices from the calling thread."""

    @classmethod
    def adopt(cls, handles):
        """ggs_group_adopt: handles 0..n-1, each already joined by attach_exchange(i, n, ...), driven as one group over
        the caller's transport.  The group does not own the handles (close() leaves them alone)."""
        self = cls.__new__(cls)
        self._L = _lib.load()
        n = len(handles)
        self._arr = (C.c_void_p * n)(*[h._h for h in handles])
        self.handles, self._owns = list(handles), False
        self._chk(self._L.ggs_group_adopt(self._arr, n))
        return self

    def __init__(self, num_topics, num_types, alpha, beta, seed, device_ids, flags=0, phi_burn_in=0, phi_mean_thin=1, alias_poisson_threshold=0):
        self._L = _lib.load()
        self._owns = True
        _lib.share_rccl_with_torch()
        cfg, keep = _make_config(num_topics, num_types, alpha, beta, seed, 0, flags, phi_burn_in, phi_mean_thin, alias_poisson_threshold)
        n = len(device_ids)
        devs = (C.c_int32 * n)(*[int(d) for d in device_ids])
        self._arr = (C.c_void_p * n)()
        rc = self._L.ggs_group_create(C.byref(cfg), n, devs, self._arr)
        if rc:
            raise GGSError(rc, "ggs_group_create failed")
        self.handles = [GGSHandle(num_topics, num_types, alpha, beta, seed, _adopt=C.c_void_p(self._arr[i])) for i in range(n)]

    def _chk(self, rc):
        if rc:
            msgs = [self._L.ggs_last_error(h._h).decode() for h in self.handles]
            raise GGSError(rc, next((m for m in msgs if m), ""))

    def set_z(self, z_list, redraw_phi=True):
        zs = [np.ascontiguousarray(z, np.int32) for z in z_list]
        ptrs = (C.POINTER(C.c_int32) * len(zs))(*[_ip(z) for z in zs])
        self._chk(self._L.ggs_group_set_z(self._arr, len(zs), ptrs, int(bool(redraw_phi))))

    def sweep(self, n=1):
        self._chk(self._L.ggs_group_sweep(self._arr, len(self.handles), int(n)))

    def gather_counts(self):
        """Corpus-wide counts onto every handle (grouped collectives); call before the per-handle getters that read them."""
        self._chk(self._L.ggs_group_gather_counts(self._arr, len(self.handles)))

    def close(self):
        if getattr(self, "handles", None):
            if getattr(self, "_owns", True):
                for h in self.handles:
                    h._h = None
                self._L.ggs_group_destroy(self._arr, len(self.handles))
            self.handles = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the estimators of the hyperparameter step (host, no GPU) ----
def learn_symmetric_concentration(count_hist, obs_lengths, num_dimensions, current):
    """MALLET's Dirichlet.learnSymmetricConcentration as include/ggs_hip.h states it"""
    ch, ol = np.ascontiguousarray(count_hist, np.int32), np.ascontiguousarray(obs_lengths, np.int32)
    out = C.c_double()
    rc = _lib.load().ggs_learn_symmetric_concentration(_ip(ch), ch.size, _ip(ol), ol.size, int(num_dimensions), float(current), C.byref(out))
    if rc:
        raise GGSError(rc, "ggs_learn_symmetric_concentration: bad argument")
    return out.value


def learn_parameters(params, obs, obs_lengths, shape=1.001, scale=1.0, iterations=1):
    """MALLET's Dirichlet.learnParameters as include/ggs_hip.h states it: params (float64 [K]) is updated IN PLACE, the new
    parameters' sum is returned.  obs: int32 [K][n_bins]."""
    if not (isinstance(params, np.ndarray) and params.dtype == np.float64 and params.flags.c_contiguous and params.ndim == 1):
        raise ValueError("params must be a contiguous float64 vector: it is updated in place")
    ob, ol = np.ascontiguousarray(obs, np.int32), np.ascontiguousarray(obs_lengths, np.int32)
    if ob.ndim != 2 or ob.shape[0] != params.size:
        raise ValueError("obs must be [K][n_bins]")
    out = C.c_double()
    rc = _lib.load().ggs_learn_parameters(_dp(params), params.size, _ip(ob), ob.shape[1], _ip(ol), ol.size, float(shape), float(scale), int(iterations),
                                          C.byref(out))
    if rc:
        raise GGSError(rc, "ggs_learn_parameters: bad argument")
    return out.value


# ---- primitives (parity tests) ----
def debug_philox(ctr, key, device_id=0):
    L = _lib.load()
    ctr = np.ascontiguousarray(ctr, np.uint32).reshape(-1, 4)
    key = np.ascontiguousarray(key, np.uint32).reshape(-1, 2)
    out = np.empty_like(ctr)
    up = C.POINTER(C.c_uint32)
    rc = L.ggs_debug_philox(device_id, ctr.shape[0], ctr.ctypes.data_as(up), key.ctypes.data_as(up), out.ctypes.data_as(up))
    if rc:
        raise GGSError(rc, "ggs_debug_philox")
    return out


def debug_math(op, x, y=None, device_id=0):
    L = _lib.load()
    x = np.ascontiguousarray(x, np.float64)
    y = x if y is None else np.ascontiguousarray(y, np.float64)
    out = np.empty_like(x)
    rc = L.ggs_debug_math(device_id, {"log": 0, "pow": 1, "sqrt": 2, "div": 3, "exp": 4, "boost_pow": 5, "u53": 6}[op], x.size, _dp(x), _dp(y), _dp(out))
    if rc:
        raise GGSError(rc, "ggs_debug_math")
    return out


def debug_draw(kind, seed, iteration, purpose, elem0, n=None, shape=None, device_id=0):
    L = _lib.load()
    if shape is not None:
        shape = np.ascontiguousarray(shape, np.float64)
        n = shape.size
    out = np.empty(n, np.float64)
    st = C.c_int32()
    rc = L.ggs_debug_draw(device_id, {"uniform": 0, "gaussian": 1, "gamma": 2, "gamma_first_try": 3, "gamma_first_try_marked": 4}[kind], seed, iteration, purpose, elem0, n,
                          _dp(shape) if shape is not None else None, _dp(out), C.byref(st))
    if rc:
        raise GGSError(rc, "ggs_debug_draw")
    return out, st.value


def debug_poisson(counts, beta, threshold, seed, iteration, purpose, elem0, device_id=0):
    """scheme=polyaurn's Poisson variates X of elements elem0 + i with counts[i], as the Phi kernel draws them (int32)."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int32)
    out = np.empty(counts.size, np.int32)
    rc = L.ggs_debug_poisson(device_id, float(beta), int(threshold), seed, iteration, purpose, elem0, counts.size, _ip(counts), _ip(out))
    if rc:
        raise GGSError(rc, "ggs_debug_poisson")
    return out


def debug_alias(phi, alpha, device_id=0):
    """scheme=spalias's alias tables of phi [K][V] under alpha, built by the product kernel: (ps [V][K], a [V][K], type_norm [V])."""
    L = _lib.load()
    phi = np.ascontiguousarray(phi, np.float64)
    K, V = phi.shape
    alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float64), (K,)))
    ps, a, tn = np.empty((V, K), np.float64), np.empty((V, K), np.int32), np.empty(V, np.float64)
    rc = L.ggs_debug_alias(device_id, V, K, _dp(phi), _dp(alpha), _dp(ps), _ip(a), _dp(tn))
    if rc:
        raise GGSError(rc, "ggs_debug_alias")
    return ps, a, tn


def debug_vs_indicators(counts, prev_phi, beta, pi, seed, iteration, u=None, device_id=0):
    """scheme=nzvsspalias's indicator chain alone, for counts [K][V] and prev_phi [K][V]: (drawn [K][V] bool, s_end [K], rounds [K]).
    u [K][V], if given, replaces the Philox uniforms."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int32)
    prev_phi = np.ascontiguousarray(prev_phi, np.float64)
    K, V = counts.shape
    if prev_phi.shape != (K, V):
        raise ValueError("prev_phi must have the shape of counts")
    if u is not None:
        u = np.ascontiguousarray(u, np.float64)
        if u.shape != (K, V):
            raise ValueError("u must have the shape of counts")
    drawn, s_end, rounds = np.empty((K, V), np.uint8), np.empty(K, np.int32), np.empty(K, np.int32)
    rc = L.ggs_debug_vs_indicators(device_id, V, K, _ip(counts), _dp(prev_phi), float(beta), float(pi), seed, iteration, _dp(u) if u is not None else None,
                                   drawn.ctypes.data_as(C.POINTER(C.c_uint8)), _ip(s_end), _ip(rounds))
    if rc:
        raise GGSError(rc, "ggs_debug_vs_indicators")
    return drawn.astype(bool), s_end, rounds


def debug_column_sum(x=None, counts=None, beta=0.0, device_id=0):
    """Column sums in index order (Java's sequential rounding) of x [V][K], or of beta + counts [V][K]."""
    L = _lib.load()
    if (x is None) == (counts is None):
        raise ValueError("exactly one of x / counts")
    if x is not None:
        x = np.ascontiguousarray(x, np.float64)
        V, K = x.shape
        xp, cp = _dp(x), None
    else:
        counts = np.ascontiguousarray(counts, np.int32)
        V, K = counts.shape
        xp, cp = None, _ip(counts)
    out = np.empty(K, np.float64)
    rc = L.ggs_debug_column_sum(device_id, V, K, xp, cp, float(beta), _dp(out))
    if rc:
        raise GGSError(rc, "ggs_debug_column_sum")
    return out


def debug_column_sum_guided(x=None, counts=None, beta=0.0, guess=None, device_id=0):
    """The same with the caller's guess [ceil(V/64) + 1][K] of the running sums at the segment starts (None: the kernels
    make their own).  Returns (sums [K], the exact running sums the walk left [ceil(V/64) + 1][K], tokensPerTopic [K] or None)."""
    L = _lib.load()
    if (x is None) == (counts is None):
        raise ValueError("exactly one of x / counts")
    if x is not None:
        x = np.ascontiguousarray(x, np.float64)
        V, K = x.shape
        xp, cp = _dp(x), None
    else:
        counts = np.ascontiguousarray(counts, np.int32)
        V, K = counts.shape
        xp, cp = None, _ip(counts)
    nseg = (V + 63) // 64
    gp = None
    if guess is not None:
        guess = np.ascontiguousarray(guess, np.float64)
        if guess.shape != (nseg + 1, K):
            raise ValueError("guess must be [ceil(V/64) + 1][K]")
        gp = _dp(guess)
    out = np.empty(K, np.float64)
    pref = np.empty((nseg + 1, K), np.float64)
    n_k = np.empty(K, np.int32)
    rc = L.ggs_debug_column_sum_guided(device_id, V, K, xp, cp, float(beta), gp, _dp(out), _dp(pref), _ip(n_k) if counts is not None else None)
    if rc:
        raise GGSError(rc, "ggs_debug_column_sum_guided")
    return out, pref, (n_k if counts is not None else None)


def debug_min_distances(a, b=None, element_major=False, device_id=0):
    """The distance kernels on arbitrary inputs: (min_dist [n], min_sq [n]).  a is [n][len] (element_major: [len][n]); b [m][len]
    or None = a against itself with the diagonal skipped."""
    L = _lib.load()
    a = np.ascontiguousarray(a, np.float64)
    if a.ndim != 2:
        raise ValueError("a must be a matrix")
    length, n = a.shape if element_major else a.shape[::-1]
    bp, m = None, 0
    if b is not None:
        b = np.ascontiguousarray(b, np.float64)
        if b.ndim != 2 or b.shape[1] != length:
            raise ValueError("b must be [m][len]")
        bp, m = _dp(b), b.shape[0]
    dist, sq = np.empty(n, np.float64), np.empty(n, np.float64)
    rc = L.ggs_debug_min_distances(device_id, _dp(a), n, bp, m, length, 1 if element_major else 0, _dp(dist), _dp(sq))
    if rc:
        raise GGSError(rc, "ggs_debug_min_distances")
    return dist, sq


def distance_id(metric):
    """GGS_DISTANCE_* of a Java class name (cc/mallet/similarity), or of the id itself"""
    if isinstance(metric, str):
        if metric not in _lib.DISTANCE_IDS:
            raise ValueError("unknown distance %r: one of %s" % (metric, ", ".join(_lib.DISTANCE_IDS)))
        return _lib.DISTANCE_IDS[metric]
    return int(metric)


def row_distances(a, b, metric, device_id=0):
    """out [m][n]: out[j][i] = Distance.calculate(a[i], b[j]) of the class `metric` for the rows of a [n][len] (v1) and b [m][len]
    (v2), on the device (ggs_row_distances): the distance kernels without a handle and without the empty-document rule."""
    L = _lib.load()
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.ndim != 2 or b.ndim != 2 or a.shape[1] != b.shape[1]:
        raise ValueError("a must be [n][len] and b [m][len]")
    out = np.empty((b.shape[0], a.shape[0]), np.float64)
    rc = L.ggs_row_distances(device_id, distance_id(metric), _dp(a), _dp(b), a.shape[0], b.shape[0], a.shape[1], _dp(out))
    if rc:
        raise GGSError(rc, "ggs_row_distances")
    return out


def debug_topic_summaries(counts, beta, kind, n, lam=0.6, device_id=0):
    """The topic-summary kernels on an arbitrary count matrix [V][K]: a dict with idx [K][n], score [K][n], mass_k [K],
    rowsum_w [V], total and all_scores [V][K] (ggs_debug_topic_summaries)."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int32)
    if counts.ndim != 2:
        raise ValueError("counts must be [V][K]")
    V, K = counts.shape
    n = int(n)
    idx, score = np.empty((K, max(n, 0)), np.int32), np.empty((K, max(n, 0)), np.float64)
    mass, rowsum, total, every = np.empty(K, np.float64), np.empty(V, np.float64), np.empty(1, np.float64), np.empty((V, K), np.float64)
    rc = L.ggs_debug_topic_summaries(device_id, V, K, _ip(counts), float(beta), float(lam), _top_kind(kind), n, _ip(idx), _dp(score), _dp(mass), _dp(rowsum),
                                     _dp(total), _dp(every))
    if rc:
        raise GGSError(rc, "ggs_debug_topic_summaries")
    return {"idx": idx, "score": score, "mass_k": mass, "rowsum_w": rowsum, "total": float(total[0]), "all_scores": every}


def debug_topic_doc_statistics(doc_ptr, tokens, z, V, K, alpha, n, idx, clogc_in=None, device_id=0):
    """The document-statistics kernels on an arbitrary corpus and assignment (ggs_debug_topic_doc_statistics):
    (codoc [K][n][n], doc_stats [K][9], clogc [K])."""
    L = _lib.load()
    doc_ptr, tokens, z = np.ascontiguousarray(doc_ptr, np.int64), np.ascontiguousarray(tokens, np.int32), np.ascontiguousarray(z, np.int32)
    alpha = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, np.float64), (K,)))
    idx = np.ascontiguousarray(idx, np.int32)
    n = int(n)
    if idx.shape != (K, max(n, 0)) or len(tokens) != len(z) or len(tokens) != int(doc_ptr[-1]):
        raise ValueError("idx must be [K][n], tokens and z as long as doc_ptr says")
    clogc_in = None if clogc_in is None else np.ascontiguousarray(clogc_in, np.float64)
    m = max(n, 0)
    codoc, stats, clogc = np.empty((K, m, m), np.int32), np.empty((K, 9), np.int32), np.empty(K, np.float64)
    rc = L.ggs_debug_topic_doc_statistics(device_id, len(doc_ptr) - 1, _lp(doc_ptr), _ip(tokens), _ip(z), int(V), int(K), _dp(alpha), n,
                                          _ip(idx), _dp(clogc_in) if clogc_in is not None else None, _ip(codoc), _ip(stats), _dp(clogc))
    if rc:
        raise GGSError(rc, "ggs_debug_topic_doc_statistics")
    return codoc, stats, clogc


def debug_topic_scores(counts, beta, n, idx, codoc, doc_stats, clogc, device_id=0):
    """The topic-score kernels on an arbitrary count matrix [V][K] (ggs_debug_topic_scores): (topic_scores [10][K],
    word_scores [4][K][n], sorted_ids [K][n])."""
    L = _lib.load()
    counts = np.ascontiguousarray(counts, np.int32)
    V, K = counts.shape
    n = int(n)
    m = max(n, 0)
    idx, codoc = np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(codoc, np.int32)
    doc_stats, clogc = np.ascontiguousarray(doc_stats, np.int32), np.ascontiguousarray(clogc, np.float64)
    if idx.shape != (K, m) or codoc.shape != (K, m, m) or doc_stats.shape != (K, 9) or clogc.shape != (K,):
        raise ValueError("idx [K][n], codoc [K][n][n], doc_stats [K][9], clogc [K]")
    ts, ws, head = np.empty((len(TOPIC_SCORE_ROWS), K), np.float64), np.empty((len(TOPIC_WORD_SCORE_ROWS), K, m), np.float64), np.empty((K, m), np.int32)
    rc = L.ggs_debug_topic_scores(device_id, V, K, _ip(counts), float(beta), n, _ip(idx), _ip(codoc), _ip(doc_stats), _dp(clogc), _dp(ts), _dp(ws), _ip(head))
    if rc:
        raise GGSError(rc, "ggs_debug_topic_scores")
    return ts, ws, head
