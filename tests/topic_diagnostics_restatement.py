"""topics/TopicModelDiagnosticsPlain.java restated in vectorised numpy, for tests/test_topic_diagnostics_model.py (CPU) and
tests/test_topic_diagnostics_gpu.py (the kernels of csrc/ggs_topic_diagnostics.hpp, bit for bit), and `literal`, the Java
statement for statement on Python floats, sets and a full IDSorter sort, which checks the numpy form.

The contract is the table at ggs_topic_doc_statistics in include/ggs_hip.h.  numpy rounds every element-wise
product, sum and quotient on its own; np.cumsum is sequential, so cumsum(...)[-1] is a Java running sum (its first step,
0.0 + x, is x for every x that is not -0.0, and none of the addends here can be -0.0).  log is the oracle's fdlibm log."""
import numpy as np

NAMES = ("tokens", "document_entropy", "word-length", "coherence", "uniform_dist", "corpus_dist", "eff_num_words", "token-doc-diff",
         "rank_1_docs", "allocation_ratio", "allocation_count")
SCORE_ROWS = tuple(x for x in NAMES if x != "word-length")        # the rows of ggs_topic_scores' topic_scores
WORD_ROWS = ("coherence", "uniform_dist", "corpus_dist", "token-doc-diff")
PROPORTIONS = np.array([0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5])    # DEFAULT_DOC_PROPORTIONS


def _log(x):
    from oracle import oracle as O
    O.build()
    return O.log(np.ascontiguousarray(x, np.float64)).reshape(np.shape(x))


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same_doubles(a, b):
    """bit for bit, NaN as NaN whatever its bits"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def top_words(counts, n):
    """T_k[r]: ggs_top_words(GGS_TOP_WORDS) -- falling count, ties by falling id"""
    counts = np.asarray(counts)
    V, K = counts.shape
    ids = np.arange(V)
    return np.stack([np.lexsort((-ids, -counts[:, k].astype(np.int64)))[:n] for k in range(K)]).astype(np.int32)


def doc_statistics(doc_ptr, tokens, z, V, K, alpha, n, idx, clogc_in=None, chunk=None):
    """(codoc [K][n][n] int32, doc_stats [K][9] int32, clogc [K]) of collectDocumentStatistics (:108-220)"""
    doc_ptr, tokens, z = np.asarray(doc_ptr, np.int64), np.asarray(tokens, np.int64), np.asarray(z, np.int64)
    alpha, idx = np.asarray(alpha, np.float64), np.asarray(idx, np.int64)
    D = len(doc_ptr) - 1
    chunk = chunk or max(64, min(4096, 2000000 // K))                # documents per dense [chunk][K] block
    lens = np.diff(doc_ptr)
    doc_of = np.repeat(np.arange(D), lens)
    alpha_sum = np.cumsum(alpha)[-1]
    stats = np.zeros((K, 9), np.int64)
    clogc = np.zeros(K) if clogc_in is None else np.array(clogc_in, np.float64)
    for d0 in range(0, D, chunk):
        d1 = min(D, d0 + chunk)
        t0, t1 = doc_ptr[d0], doc_ptr[d1]
        c = np.zeros((d1 - d0, K), np.int64)
        np.add.at(c, (doc_of[t0:t1] - d0, z[t0:t1]), 1)
        pos = c > 0
        stats[:, 0] += pos.sum(0)
        has = lens[d0:d1] > 0
        stats[:, 1] += np.bincount(np.argmax(c[has], axis=1), minlength=K) if has.any() else 0     # argmax: the first (lowest k) maximum
        prop = (alpha[None, :] + c) / (alpha_sum + lens[d0:d1])[:, None]
        go = np.cumsum(prop[:, :, None] < PROPORTIONS[None, None, :], axis=2) == 0                  # until the first prop < P[i]
        stats[:, 2:] += (go & pos[:, :, None]).sum(0)
        cd = c.astype(np.float64)
        add = np.where(c > 1, cd * _log(np.where(c > 1, cd, 1.0)), 0.0)                             # 1 * log(1) = +0.0
        run = np.cumsum(np.vstack([clogc[None, :], add]), axis=0)[-1]
        clogc = np.where(pos.any(0), run, clogc)                                                    # no document, no addition
    # codoc: the distinct (document, topic, position) triples, grouped by (topic, document)
    where = np.full((K, V), -1, np.int16)
    where[np.arange(K)[:, None], idx] = np.arange(n)[None, :]
    r = where[z, tokens].astype(np.int64) if len(tokens) else np.zeros(0, np.int64)
    sel = r >= 0
    key = np.unique((z[sel] * max(D, 1) + doc_of[sel]) * n + r[sel])
    groups, inv = np.unique(key // n, return_inverse=True)
    M = np.zeros((len(groups), n))
    M[inv, key % n] = 1.0
    codoc = np.zeros((K, n, n), np.int32)
    bounds = np.searchsorted(groups // max(D, 1), np.arange(K + 1))
    for k in range(K):
        Mk = M[bounds[k]:bounds[k + 1]]
        codoc[k] = (Mk.T @ Mk).astype(np.int32)                   # 0/1 products summed in doubles: exact
    return codoc, stats.astype(np.int32), clogc


def sorted_cells(counts, k):
    """IDSorter's order of ALL V words of topic k: falling count, ties by falling id"""
    col = np.asarray(counts)[:, k].astype(np.int64)
    return np.lexsort((-np.arange(len(col)), -col))


def scores(counts, beta, n, idx, codoc, doc_stats, clogc):
    """(topic_scores [10][K] in SCORE_ROWS' order, word_scores [4][K][n] in WORD_ROWS' order, sorted_ids [K][n])"""
    counts, idx = np.asarray(counts, np.int64), np.asarray(idx, np.int64)
    codoc, st, clogc = np.asarray(codoc, np.int64), np.asarray(doc_stats, np.int64).astype(np.float64), np.asarray(clogc, np.float64)
    V, K = counts.shape
    beta = np.float64(beta)
    n_k = counts.sum(0)
    wtc = counts.sum(1)
    nk = n_k.astype(np.float64)
    num_tokens = np.float64(int(n_k.sum()))
    ts = np.zeros((10, K))
    ws = np.zeros((4, K, n))
    head = np.zeros((K, n), np.int32)
    with np.errstate(all="ignore"):
        ts[0] = nk
        ts[1] = -clogc / nk + _log(nk)
        # coherence (:474-499)
        M = codoc.astype(np.float64)
        diag = np.diagonal(M, axis1=1, axis2=2)                                   # [K][n]
        S = _log((M + beta) / (diag[:, None, :] + beta))                          # [K][row][col]
        lower = np.tril(np.ones((n, n), bool), -1)[None]
        run = np.cumsum(np.where(lower, S, 0.0), axis=2)                          # the addends of col >= row come after the chain's end
        row_score = np.concatenate([np.zeros((K, 1)), run[:, np.arange(1, n), np.arange(0, n - 1)]], axis=1)
        ts[2] = np.cumsum(row_score, axis=1)[:, -1]
        ws[0] = np.fmin.reduce(np.where(lower, S, np.inf), axis=2, initial=0.0)   # `score < minScore` never takes a NaN
        coef = num_tokens / nk
        for k in range(K):
            order = sorted_cells(counts, k)
            c = counts[order, k].astype(np.float64)
            p = c / nk[k]
            u = p * _log((c * np.float64(V)) / nk[k])
            g = p * _log(coef[k] * c / wtc[order].astype(np.float64))
            ts[3, k] = np.cumsum(u)[-1]
            ts[4, k] = np.cumsum(g)[-1]
            ts[5, k] = 1.0 / np.cumsum(p * p)[-1]
            ws[1, k], ws[2, k] = u[:n], g[:n]
            head[k] = np.where(c[:n] > 0, order[:n], -1)
        # token-doc-diff (:345-396)
        w = counts[idx, np.arange(K)[:, None]].astype(np.float64)                 # [K][n]
        word_sum, doc_sum = np.cumsum(w, axis=1)[:, -1:], np.cumsum(diag, axis=1)[:, -1:]
        p, q = w / word_sum, diag / doc_sum
        mean = 0.5 * (p + q)
        sc = np.zeros((K, n))
        sc = np.where(p > 0, sc + 0.5 * p * _log(p / mean), sc)
        sc = np.where(q > 0, sc + 0.5 * q * _log(q / mean), sc)
        ws[3] = sc
        ts[6] = np.cumsum(sc, axis=1)[:, -1]
        ts[7] = st[:, 1] / st[:, 0]
        ts[8] = st[:, 2 + 6] / st[:, 2 + 1]
        ts[9] = st[:, 2 + 5] / st[:, 0]
    return ts, ws, head


def word_length(vocab, idx):
    """getWordLengthScores (:399-418): Java String.length() counts UTF-16 code units"""
    n = np.shape(idx)[1]
    return np.array([float(sum(len(vocab[i].encode("utf-16-le")) // 2 for i in row)) / n for row in np.asarray(idx).tolist()])


def diagnostics(doc_ptr, tokens, z, counts, alpha, beta, n):
    """the whole object from z and the counts: what get_z() + get_type_topic_counts() + numpy cost a user"""
    counts = np.asarray(counts)
    V, K = counts.shape
    idx = top_words(counts, n)
    codoc, stats, clogc = doc_statistics(doc_ptr, tokens, z, V, K, np.broadcast_to(np.asarray(alpha, np.float64), (K,)), n, idx)
    ts, ws, _ = scores(counts, beta, n, idx, codoc, stats, clogc)
    return dict(idx=idx, codoc=codoc, doc_stats=stats, clogc=clogc, topic_scores=ts, word_scores=ws)


# ---- TopicModelDiagnosticsPlain.java, statement for statement ---------------------------------------------------------------
def literal(doc_ptr, tokens, z, counts, alpha, beta, n, vocab=None):
    """dict of the Java object's fields: codoc, rank1, nonzero, at_prop, clogc, and scores[name] = (topic scores, word scores)"""
    import functools
    import math
    from oracle import oracle as O
    from tests.topic_summaries_restatement import IDSorter
    O.build()

    def log(v):
        v = float(v)
        if v != v or v < 0:
            return math.nan
        if v == 0:
            return -math.inf
        return float(O.log(np.array([v], np.float64))[0])

    def div(a, b):                                                # Java double division: no exception
        a, b = float(a), float(b)
        if b == 0.0:
            return math.nan if (a == 0.0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
        return a / b

    c = np.asarray(counts)
    V, K = c.shape
    alpha = [float(a) for a in np.broadcast_to(np.asarray(alpha, np.float64), (K,))]
    beta = float(beta)
    tokens_per_topic = [int(c[:, k].sum()) for k in range(K)]
    sorted_words = [sorted((IDSorter(w, float(int(c[w, k]))) for w in range(V)), key=functools.cmp_to_key(lambda a, b: a.compare_to(b))) for k in range(K)]
    in_order = [[sorted_words[k][i].wi for i in range(n)] for k in range(K)]
    top_sets = [set(row) for row in in_order]
    codoc = [[[0] * n for _ in range(n)] for _ in range(K)]
    word_type_counts, num_tokens = [0] * V, 0
    rank1, nonzero, at_prop, clogc = [0] * K, [0] * K, [[0] * 7 for _ in range(K)], [0.0] * K
    doc_sets = [set() for _ in range(K)]
    topic_counts = [0] * K
    P = [float(x) for x in PROPORTIONS]
    for d in range(len(doc_ptr) - 1):
        for t in range(int(doc_ptr[d]), int(doc_ptr[d + 1])):
            typ, topic = int(tokens[t]), int(z[t])
            num_tokens += 1
            word_type_counts[typ] += 1
            topic_counts[topic] += 1
            if typ in top_sets[topic]:
                doc_sets[topic].add(typ)
        doc_length = int(doc_ptr[d + 1] - doc_ptr[d])
        alpha_sum = 0.0
        for a in alpha:
            alpha_sum += a
        if doc_length > 0:
            max_topic, max_count = -1, -1
            for topic in range(K):
                if topic_counts[topic] > 0:
                    nonzero[topic] += 1
                    if topic_counts[topic] > max_count:
                        max_topic, max_count = topic, topic_counts[topic]
                    clogc[topic] += topic_counts[topic] * log(topic_counts[topic])
                    proportion = (alpha[topic] + topic_counts[topic]) / (alpha_sum + doc_length)
                    for i in range(7):
                        if proportion < P[i]:
                            break
                        at_prop[topic][i] += 1
                    supported, indices = doc_sets[topic], in_order[topic]
                    for i in range(n):
                        if indices[i] in supported:
                            for j in range(i, n):
                                if i == j:
                                    codoc[topic][i][i] += 1
                                elif indices[j] in supported:
                                    codoc[topic][i][j] += 1
                                    codoc[topic][j][i] += 1
                    doc_sets[topic].clear()
                    topic_counts[topic] = 0
            if max_topic > -1:
                rank1[max_topic] += 1
    out = {}
    out["tokens"] = ([float(t) for t in tokens_per_topic], None)
    out["document_entropy"] = ([div(-clogc[k], tokens_per_topic[k]) + log(tokens_per_topic[k]) for k in range(K)], None)
    if vocab is not None:
        out["word-length"] = ([float(sum(len(vocab[w].encode("utf-16-le")) // 2 for w in in_order[k])) / n for k in range(K)], None)
    coh, coh_w = [], []
    for k in range(K):
        topic_score, words = 0.0, []
        for row in range(n):
            row_score, min_score = 0.0, 0.0
            for col in range(row):
                score = log(div(codoc[k][row][col] + beta, codoc[k][col][col] + beta))
                row_score += score
                if score < min_score:
                    min_score = score
            topic_score += row_score
            words.append(min_score)
        coh.append(topic_score)
        coh_w.append(words)
    out["coherence"] = (coh, coh_w)
    uni, uni_w, cor, cor_w, eff = [], [], [], [], []
    for k in range(K):
        tk = tokens_per_topic[k]
        s_u, s_c, s_e, w_u, w_c = 0.0, 0.0, 0.0, [], []
        coefficient = div(float(num_tokens), tk)
        for position, info in enumerate(sorted_words[k]):
            count = info.p
            su = div(count, tk) * log(div(count * V, tk))
            sc = div(count, tk) * log(div(coefficient * count, word_type_counts[info.wi]))
            if position < n:
                w_u.append(su)
                w_c.append(sc)
            s_u += su
            s_c += sc
            probability = div(count, tk)
            s_e += probability * probability
        uni.append(s_u); uni_w.append(w_u); cor.append(s_c); cor_w.append(w_c); eff.append(div(1.0, s_e))
    out["uniform_dist"], out["corpus_dist"], out["eff_num_words"] = (uni, uni_w), (cor, cor_w), (eff, None)
    tdd, tdd_w = [], []
    for k in range(K):
        wdist = [sorted_words[k][r].p for r in range(n)]
        ddist = [float(codoc[k][r][r]) for r in range(n)]
        word_sum = doc_sum = 0.0
        for r in range(n):
            word_sum += wdist[r]
            doc_sum += ddist[r]
        topic_score, words = 0.0, []
        for r in range(n):
            p, q = div(wdist[r], word_sum), div(ddist[r], doc_sum)
            mean = 0.5 * (p + q)
            score = 0.0
            if p > 0:
                score += 0.5 * p * log(div(p, mean))
            if q > 0:
                score += 0.5 * q * log(div(q, mean))
            words.append(score)
            topic_score += score
        tdd.append(topic_score)
        tdd_w.append(words)
    out["token-doc-diff"] = (tdd, tdd_w)
    out["rank_1_docs"] = ([div(rank1[k], nonzero[k]) for k in range(K)], None)
    out["allocation_ratio"] = ([div(at_prop[k][6], at_prop[k][1]) for k in range(K)], None)
    out["allocation_count"] = ([div(at_prop[k][5], nonzero[k]) for k in range(K)], None)
    return dict(idx=in_order, codoc=codoc, rank1=rank1, nonzero=nonzero, at_prop=at_prop, clogc=clogc, scores=out)


def random_case(D, V, K, seed, mean_len=12, lengths=None):
    """(doc_ptr, tokens, z, counts): a random corpus with a random assignment and ITS counts"""
    rng = np.random.default_rng([D, V, K, seed])
    lens = np.asarray(lengths, np.int64) if lengths is not None else rng.poisson(mean_len, D)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(doc_ptr[-1])
    tokens = np.minimum((V * rng.random(N) ** 2.0).astype(np.int32), V - 1)          # a skewed vocabulary: repeated words within documents
    z = rng.integers(0, K, N).astype(np.int32)
    counts = np.zeros((V, K), np.int32)
    np.add.at(counts, (tokens, z), 1)
    return doc_ptr, tokens, z, counts


def edge_case():
    """(doc_ptr, tokens, z, counts, V, K, n) built by hand, K = 5, V = 10, n = 4: document 0 holds every top word of topic 0
    (T_0 = [0, 3, 2, 1]: the full n x n block) and word 0 three times; words 2 and 3 are top words of topics 0, 1 and 2 at once
    (membership lists longer than one entry) and occur under other topics than the one asked about; topic 3 has two non-zero words (< n: its list
    continues with zero-count words, whose rows stay zero); topic 4 has no token; document 3 ties topics 0 and 3 for rank 1,
    document 4 ties all four topics it has; document 5 is empty; document 6 has word 5 (a top word of topic 3) under topic 0
    only, beside another word under topic 3."""
    docs = [[(0, 0), (1, 0), (2, 0), (3, 0), (0, 0), (0, 0)],
            [(0, 1), (1, 1), (0, 0), (1, 0), (2, 0), (3, 0)],
            [(2, 1), (3, 1), (0, 1), (2, 2), (3, 2), (0, 2), (1, 2)],
            [(5, 3), (6, 3), (4, 0), (8, 0)],
            [(7, 0), (7, 1), (7, 2), (5, 3)],
            [],
            [(5, 0), (6, 3), (9, 0)]]
    V, K, n = 10, 5, 4
    doc_ptr = np.concatenate([[0], np.cumsum([len(d) for d in docs])]).astype(np.int64)
    tokens = np.array([w for d in docs for w, _ in d], np.int32)
    z = np.array([k for d in docs for _, k in d], np.int32)
    counts = np.zeros((V, K), np.int32)
    np.add.at(counts, (tokens, z), 1)
    return doc_ptr, tokens, z, counts, V, K, n


def threshold_cases(K, c, length, target):
    """Documents whose topic-0 proportion (alpha_0 + c) / (alphaSum + length) is exactly the double `target`, its lower and its
    upper neighbour: alpha_0 moves by a few ulps around 1 and alpha_1 takes the difference back, so that alphaSum stays K.
    Returns {"at" | "below" | "above": (alpha [K], doc_ptr, tokens, z)}; the document has c tokens of topic 0, the others spread
    over topics 1.. ; V = 2."""
    target = np.float64(target)
    want = {"at": target, "below": np.nextafter(target, 0.0), "above": np.nextafter(target, 1.0)}
    z = np.array([0] * c + [1 + (i % (K - 1)) for i in range(length - c)], np.int32)
    tokens = (np.arange(length) % 2).astype(np.int32)
    doc_ptr = np.array([0, length], np.int64)
    out = {}
    for j in range(-64, 65):
        a0 = np.float64(1.0) + j * 2.0 ** -53
        alpha = np.ones(K)
        alpha[0], alpha[1] = a0, np.float64(2.0) - a0
        if np.cumsum(alpha)[-1] != K:
            continue
        prop = (alpha[0] + np.float64(c)) / (np.cumsum(alpha)[-1] + np.float64(length))
        for name, v in want.items():
            if prop == v and name not in out:
                out[name] = (alpha, doc_ptr, tokens, z)
    return out
