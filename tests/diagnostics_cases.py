"""The shapes at which the two diagnostics (ggs_model_log_likelihood, ggs_log_posterior: csrc/ggs_loglik.hpp) are judged,
shared by tests/test_diagnostics_model.py (the reference, on the CPU) and tests/test_diagnostics_gpu.py (the kernels).

The reference of a side of a diagnostic is the exact sum (math.fsum) of the terms the oracle's Java-order loop adds; the
device evaluates the same term expressions bit for bit (strict_log, -ffp-contract=off), so the only legitimate difference
is the order of summation, and that is bounded by the longest chain of additions an addend passes through: chains() below.
"""
import math
from collections import namedtuple

import numpy as np

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus

U = 2.0 ** -53                                   # unit roundoff of a double

# ---- the launch shapes of csrc/ggs_loglik.hpp and their launchers (the entry points of ggs_api.hip), restated ----
LL_BLOCK = 256                                   # kLLBlock: threads of every block of these kernels
LL_GRID = 1024                                   # blocks of the grid-stride kernels over n_wk and over Phi
MAX_LDS = 160 * 1024                             # kMaxLdsBytes
LANE_TREE = 6                                    # ll_block_sum: __shfl_down by 32, 16, 8, 4, 2, 1
WAVE_PARTIALS = 4                                # ll_block_sum: thread 0 adds wave_part[0..3] to 0.0


DOC_WAVES = LL_BLOCK // 64                       # documents per block of ll_docs_kernel / lp_docs_kernel: a wave and a K-long int32 histogram each
MAX_TOPICS = (MAX_LDS - 32) // (4 * DOC_WAVES)   # kLLMaxTopics = 10238: four histograms and the 32 bytes of wave partials fill 160 KiB


def ceil_div(a, b):
    return -(-a // b)


def chains(D, K, V, longest_doc):
    """c of the bound |device - exact| <= (c + 2) * 2^-53 * sum|t| for each side of each diagnostic: the longest chain of
    floating additions one addend passes through on the device, read off the kernels (none of it is fitted).

    Every kernel ends in ll_block_sum: the lane tree (6 additions) and thread 0's sum of the 4 wave partials (4).  Every
    finish kernel is one block whose thread i adds partials i, i + 256, ... and ends in ll_block_sum again.

    model log likelihood, document side
        ll_docs_kernel: a lane adds the terms of topics lane, lane + 64, ...: ceil(K / 64); lane 0 then subtracts
        lgS(alphaSum + N_d): 1; block sum: 10.  ll_finish_kernel: ceil(blocks / 256) with blocks = ceil(D / 4);
        block sum: 10; + D * lgS(alphaSum): 1.
    model log likelihood, topic side
        ll_types_kernel: grid-stride over V * K cells with 1024 * 256 threads: ceil(V * K / 262144); block sum: 10.
        ll_finish_kernel: 1024 / 256 = 4 partials, then the same thread's lgS(V * beta + n_k) of topics i, i + 256, ...:
        ceil(K / 256); block sum: 10; + lgS(V * beta) * K and - lgS(beta) * nonZero: 2.
    log posterior, document side
        lp_docs_kernel: a lane adds log(phi) of tokens lane, lane + 64, ... of its document: ceil(longest / 64), then the
        theta terms of topics lane, lane + 64, ...: ceil(K / 64); block sum: 10.  lp_finish_kernel: ceil(blocks / 256) + 10.
    log posterior, topic side
        lp_phi_kernel: ceil(V * K / 262144) + 10.  lp_finish_kernel: 4 + 10.  The product with (beta - 1) is no addition:
        it is one of the two roundings the bound's "+ 2" stands for (the other: the oracle's terms are rounded products
        count * log(phi) and (beta - 1) * log(phi), where the device adds log(phi) per token and multiplies once).
    """
    block_sum = LANE_TREE + WAVE_PARTIALS
    blocks = ceil_div(D, DOC_WAVES)
    finish_docs = ceil_div(blocks, LL_BLOCK) + block_sum
    grid = ceil_div(V * K, LL_GRID * LL_BLOCK) + block_sum
    return dict(ll_doc=ceil_div(K, 64) + 1 + block_sum + finish_docs + 1,
                ll_topic=grid + LL_GRID // LL_BLOCK + ceil_div(K, LL_BLOCK) + block_sum + 2,
                lp_doc=ceil_div(longest_doc, 64) + ceil_div(K, 64) + block_sum + finish_docs,
                lp_topic=grid + LL_GRID // LL_BLOCK + block_sum)


Exact = namedtuple("Exact", "value abs_sum n")


def exact(terms):
    """(the exact sum of the terms, correctly rounded; sum |t|, rounded up a hair; how many)"""
    terms = np.asarray(terms, np.float64)
    return Exact(math.fsum(terms.tolist()), math.fsum(np.abs(terms).tolist()) * (1 + 4 * U), terms.size)


# ---- alpha -----------------------------------------------------------------------------------------------------------
def asymmetric_alpha(K):
    """Per-topic alpha from 0.01 to 5, log-spaced and shuffled: no two topics share a value."""
    if K == 1:
        return np.array([0.7])
    a = np.exp(np.linspace(np.log(0.01), np.log(5.0), K))
    a[0], a[-1] = 0.01, 5.0
    return np.random.default_rng(K).permutation(a)


# ---- the corpora -----------------------------------------------------------------------------------------------------
def _from_lens(lens, V, seed):
    lens = np.asarray(lens, np.int64)
    tokens = np.random.default_rng(seed).integers(0, V, int(lens.sum())).astype(np.int32)
    return Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens, V)


def wide_corpus(K):
    """41 = 4 * 10 + 1 ragged documents on 60 types: a small V keeps the K x V side cheap at K = 4096."""
    return random_corpus(41, 60, 150, seed=K, empty_every=11)


TOPICS = (1, 2, 63, 64, 65, 127, 257, 1024, 2049, 4094, 4095, 4096)
TOPICS_GGS_MAX = 2049                            # scheme ggs runs the list up to here; pcgs, spalias, polyaurn all of it
BEYOND_FOUR_HISTOGRAMS = 10240                   # 4 * 4 * K + 32 > 160 KiB from K = 10239 = MAX_TOPICS + 1
# (scheme, K) of the topic list; spalias shares the pcgs model (its Phi, its theta), so the CPU side has no state of its own for it
TOPIC_CASES = ([("ggs", K) for K in TOPICS if K <= TOPICS_GGS_MAX]
               + [(s, K) for s in ("pcgs", "spalias", "polyaurn") for K in TOPICS])
TOPIC_CASES_CPU = [c for c in TOPIC_CASES if c[0] != "spalias"] + [("ggs", BEYOND_FOUR_HISTOGRAMS)]


def huge_count_corpus():
    """50 documents of 40 000 tokens of word 0 and a handful of other words: with z = 2 on every word-0 token the cell
    (word 0, topic 2) counts 2 000 000.  Returns (corpus, z)."""
    D, n, V = 50, 40000, 5
    lens = np.full(D, n + 3, np.int64)
    tokens = np.zeros((D, n + 3), np.int32)
    tokens[:, n:] = [1, 2, 4]
    z = np.full((D, n + 3), 2, np.int32)
    z[:, n:] = [0, 3, 1]
    return Corpus(np.concatenate(([0], np.cumsum(lens))).astype(np.int64), tokens.ravel(), V), z.ravel()


# name -> (corpus builder, K, alpha, beta); alpha a scalar or "asym"
DOCUMENT_SHAPES = {
    "D=1": (lambda: _from_lens([37], 50, 1), 20, 0.1, 0.01),
    "D=2": (lambda: _from_lens([5, 90], 50, 2), 33, 0.1, 0.01),
    "D=3": (lambda: _from_lens([64, 1, 65], 50, 3), 33, 5.0, 7.0),
    "D=5": (lambda: _from_lens([12, 0, 128, 3, 129], 50, 5), 20, 0.1, 0.01),
    "all-empty": (lambda: _from_lens([0, 0, 0, 0, 0, 0], 7, 0), 9, 0.3, 0.2),
    "empty-every-4": (lambda: random_corpus(101, 80, 60, seed=3, empty_every=4), 33, 0.1, 0.01),
    "one-token-documents": (lambda: Corpus(np.arange(42, dtype=np.int64), (np.arange(41) % 6).astype(np.int32), 6), 9, 0.5, 0.1),
    "long-document": (lambda: _from_lens([7, 40000, 3, 0, 25], 300, 7), 130, 0.1, 0.01),
    "more-documents-than-types": (lambda: random_corpus(301, 20, 30, seed=9), 21, "asym", 0.05),
}
# V * K = 4100 * 257 = 1 053 700 cells: four full passes of the 262 144-thread grid and a fifth that ends inside block 19
GRID_PASSES = (lambda: random_corpus(61, 4100, 200, seed=12, empty_every=9), 257, 0.1, 0.01)


SHARD_CUTS = ((0, 33, 101), (0, 7, 7, 101), (0, 50, 99, 101))       # uneven cuts, two and three ways, an empty shard


def shard_corpus():
    return random_corpus(101, 80, 60, seed=21, empty_every=6)


def resolve_alpha(alpha, K):
    return asymmetric_alpha(K) if isinstance(alpha, str) else alpha


def plant_last_topic(z, doc_ptr, K):
    """z with the last token of the longest document moved to topic K - 1, so that a document has a non-zero count in
    the last topic of the last 64-group (the K % 64 tail of the document kernels' lane loop) whatever the chain drew.
    With it the tests' "topic K - 1 is hit" assertions hold by construction for every corpus with a token: they guard the
    planting, not the choice of corpus."""
    z = np.array(z, np.int32)
    lens = np.diff(doc_ptr)
    if z.size:
        z[int(doc_ptr[int(np.argmax(lens)) + 1]) - 1] = K - 1
    return z


def plant_phi_zeros(phi, z, tokens, doc_ptr):
    """phi with the cell under the first token of every third non-empty document set to exactly 0: the Poisson draw of
    scheme=polyaurn leaves such zeros under tokens wherever a cell counts one or two (see phi_zeros_under_tokens), which a
    narrow K on a small corpus has none of.  With it "a token sits on a zero of Phi" holds by construction; what depends
    on the corpus is the count of zeros the draw itself left, which the tests assert for K >= 63."""
    phi = np.array(phi, np.float64)
    doc_ptr = np.asarray(doc_ptr, np.int64)
    first = doc_ptr[:-1][np.diff(doc_ptr) > 0][::3]
    phi[np.asarray(z)[first], np.asarray(tokens)[first]] = 0.0
    return phi


def phi_zeros_under_tokens(phi, z, tokens):
    """how many tokens of the corpus sit on an exact zero of Phi: each contributes log(0 + 1e-12) to the log posterior"""
    return int((np.asarray(phi)[np.asarray(z), np.asarray(tokens)] == 0.0).sum())


def doc_side_terms_by_document(n_dk, doc_ptr, z, tokens, V):
    """Where each document's terms start in the two document sides the oracle exports (its loops run document by
    document): (offsets of the model log likelihood's terms, offsets of the log posterior's), each D + 1 long.  The model
    log likelihood adds one term per non-zero n_dk and one per document (and D * lgS(alphaSum) after the last document);
    the log posterior one per distinct (topic, type) cell of the document and K theta terms."""
    n_dk = np.asarray(n_dk)
    D, K = n_dk.shape
    doc_of = np.repeat(np.arange(D, dtype=np.int64), np.diff(doc_ptr))
    cells = np.unique((doc_of * K + np.asarray(z, np.int64)) * V + np.asarray(tokens, np.int64)) // (K * V)
    ll = np.concatenate(([0], np.cumsum((n_dk > 0).sum(axis=1) + 1)))
    lp = np.concatenate(([0], np.cumsum(np.bincount(cells, minlength=D) + K)))
    return ll.astype(np.int64), lp.astype(np.int64)
