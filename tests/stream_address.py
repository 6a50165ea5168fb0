"""The address of every random number of this library, stated once from the text of include/ggs_hip.h ("RNG stream
addressing"), and the corners at which the tests run it.  A test helper, not collected; it needs no device.

    Philox4x32-10,  key = (seed lo, seed hi),  counter = (elem lo, elem hi, purpose << 24 | block, iteration)

and a block's four words give two doubles the way java.util.Random.nextDouble builds one from next(26) and next(27):
((w0 >> 6) << 27 | w1 >> 5) * 2^-53 and the same of (w2, w3).  Nothing here calls the oracle's own draws (O.uniforms and
the like): only O.philox, which has Random123's known-answer vectors (tests/test_oracle_cpu.py).  So this file can decide
between the oracle and the device, should they ever part at a corner.

The corners: a seed whose two key words are non-zero and distinct with the top bit set; an iteration number with four
distinct non-zero bytes just below INT32_MAX; a tok_base that puts the global token index past 2^32 INSIDE a document and off
every multiple of 64 from the shard's start; a doc_base that puts the theta element (doc_base + d) * K + k past 2^32 INSIDE
a row.  MUTANTS are address functions that each get one word wrong, the way a narrowed Params field, a hoisted high word, an
int product or a 16-bit iteration would: tests/test_stream_address_model.py shows that the cases tell each of them from the
truth.  The device is never run with a mutant."""
import numpy as np

from oracle import oracle as O

M32 = 0xFFFFFFFF
TWO32 = 1 << 32
PURPOSE_Z, PURPOSE_THETA, PURPOSE_PHI, PURPOSE_INIT_PHI, PURPOSE_HELDOUT, PURPOSE_VS = 1, 2, 3, 4, 5, 6
PURPOSES = (PURPOSE_Z, PURPOSE_THETA, PURPOSE_PHI, PURPOSE_INIT_PHI, PURPOSE_HELDOUT, PURPOSE_VS)

SEED = 0xF1E2D3C4B5A69788
IT0 = 0x7F3A91C3
INT32_MAX = 2 ** 31 - 1
KS = (20, 200)                                           # 2^32 mod 20 = 16, 2^32 mod 200 = 96: the theta crossing is inside a row

assert (SEED & M32) != (SEED >> 32) and (SEED & M32) and SEED >> 63 == 1
assert len({(IT0 >> s) & 0xFF for s in (0, 8, 16, 24)} - {0}) == 4 and IT0 + 16 < INT32_MAX


# ---- the rule -------------------------------------------------------------------------------------------------------------
def key(seed):
    return (seed & M32, (seed >> 32) & M32)


def counter(purpose, iteration, elem, block=0):
    return (elem & M32, (elem >> 32) & M32, ((purpose << 24) | block) & M32, iteration & M32)


def true_address(seed, iteration, purpose, elem, block=0, base=0):
    """(counter, key) of one Philox block; `base` (the shard's first element) is what only a mutant looks at"""
    return counter(purpose, iteration, elem, block), key(seed)


def double_of(wa, wb):
    return float(((wa >> 6) << 27) + (wb >> 5)) * 2.0 ** -53


def uniform_pair(seed, iteration, purpose, elem, block=0, address=true_address, base=0):
    """the two doubles of one block of an element's stream: positions 2 * block and 2 * block + 1"""
    o = O.philox(*address(seed, iteration, purpose, elem, block, base))
    return double_of(o[0], o[1]), double_of(o[2], o[3])


def first_uniforms(seed, iteration, purpose, elem0, n, address=true_address, base=None):
    """each element's first draw (what a z step takes), elements elem0 ... elem0 + n - 1"""
    base = elem0 if base is None else base
    return np.array([uniform_pair(seed, iteration, purpose, elem0 + i, 0, address, base)[0] for i in range(n)], np.float64)


# ---- the mutants ----------------------------------------------------------------------------------------------------------
def _seed_hi_dropped(seed, iteration, purpose, elem, block=0, base=0):
    return counter(purpose, iteration, elem, block), (seed & M32, 0)


def _seed_lo_only_shifted(seed, iteration, purpose, elem, block=0, base=0):
    return counter(purpose, iteration, elem, block), ((seed >> 32) & M32, seed & M32)


def _elem_hi_dropped(seed, iteration, purpose, elem, block=0, base=0):
    return counter(purpose, iteration, elem & M32, block), key(seed)


def _elem_hi_from_base(seed, iteration, purpose, elem, block=0, base=0):
    """the high word hoisted to the shard's base, the low word added without a carry"""
    c = counter(purpose, iteration, elem, block)
    return (((base & M32) + (elem - base)) & M32, (base >> 32) & M32, c[2], c[3]), key(seed)


def _iteration_low16(seed, iteration, purpose, elem, block=0, base=0):
    return counter(purpose, iteration & 0xFFFF, elem, block), key(seed)


def _block_in_purpose_byte(seed, iteration, purpose, elem, block=0, base=0):
    """the two fields of the third word in each other's place: the block in the top byte, the purpose below it.  (A z step
    draws from block 0 only, so a mutant that misplaced the block alone would be the truth there.)"""
    c = counter(purpose, iteration, elem, block)
    return (c[0], c[1], (purpose | (block << 24)) & M32, c[3]), key(seed)


MUTANTS = {"seed_hi_dropped": _seed_hi_dropped, "seed_lo_only_shifted": _seed_lo_only_shifted, "elem_hi_dropped": _elem_hi_dropped,
           "elem_hi_from_base": _elem_hi_from_base, "iteration_low16": _iteration_low16, "block_in_purpose_byte": _block_in_purpose_byte}
ELEM_MUTANTS = ("elem_hi_dropped", "elem_hi_from_base")   # the truth below 2^32 (for a base below 2^32), wrong from there on


# ---- the corners ----------------------------------------------------------------------------------------------------------
def bases(corpus, K, doc, offset=5):
    """(doc_base, tok_base) of a shard holding `corpus` such that the global token index reaches 2^32 at position `offset` of
    document `doc`, and the theta element (doc_base + d) * K + k reaches 2^32 in row `doc` at k = 2^32 mod K."""
    ptr = corpus.doc_ptr
    first = int(ptr[doc]) + offset
    assert int(ptr[doc + 1]) - int(ptr[doc]) > 2 * offset, "document %d has %d tokens" % (doc, int(ptr[doc + 1] - ptr[doc]))
    assert first % 64 != 0, "the crossing is a multiple of 64 from the shard's start"
    assert 0 < TWO32 % K < K - 1, "2^32 mod K = %d: the theta crossing is at a row's edge" % (TWO32 % K)
    assert 0 < doc < corpus.num_docs - 1
    tok_base, doc_base = TWO32 - first, TWO32 // K - doc
    assert tok_base + first == TWO32 and (doc_base + doc) * K < TWO32 < (doc_base + doc + 1) * K
    assert (doc_base + doc) * K + TWO32 % K == TWO32
    return doc_base, tok_base


def crossing_token(corpus, doc, offset=5):
    """the shard-local index of the first token whose global index is >= 2^32"""
    return int(corpus.doc_ptr[doc]) + offset


def pick_doc(corpus, offset=5, start=None):
    """a document near the middle that bases() accepts"""
    ptr = corpus.doc_ptr
    for d in range(corpus.num_docs // 2 if start is None else start, corpus.num_docs - 1):
        if int(ptr[d + 1] - ptr[d]) > 2 * offset and (int(ptr[d]) + offset) % 64 != 0:
            return d
    raise AssertionError("no document fits")


def split_at_crossing(bad, cross):
    """(before, at, after) counts of a boolean mismatch vector around the crossing token: a lost carry reads as (0, x, y)"""
    bad = np.asarray(bad, bool)
    return int(bad[:cross].sum()), int(bad[cross]), int(bad[cross + 1:].sum())


# ---- a z step given Phi, walked directly ----------------------------------------------------------------------------------
def java_walk(scores, U):
    """GGS:96-113 / UPLDA:1509-1526: the scores summed in index order, sample = U * sum, then sample -= score[k] while > 0"""
    total = float(np.cumsum(scores)[-1])
    chain = np.cumsum(np.concatenate(([U * total], -scores)))
    assert chain[0] > 0
    past = np.flatnonzero(~(chain[1:] > 0))
    assert past.size
    return int(past[0])


def z_step_direct(scheme, corpus, z, phi, seed, iteration, tok_base, theta=None, alpha=None, address=true_address):
    """One z step given Phi over the whole shard, token by token, every uniform from uniform_pair: scheme "ggs" scores
    theta[d][k] * phi[k][w] (theta given), "pcgs" (n_dk + alpha) * phi[k][w] with the document's counts kept in step."""
    K = phi.shape[0]
    z = np.array(z, np.int64)
    ptr, tok = corpus.doc_ptr, corpus.tokens
    for d in range(corpus.num_docs):
        b, e = int(ptr[d]), int(ptr[d + 1])
        if scheme == "pcgs":
            cnt = np.bincount(z[b:e], minlength=K).astype(np.int64)
        for pos in range(b, e):
            w = int(tok[pos])
            U = uniform_pair(seed, iteration, PURPOSE_Z, tok_base + pos, 0, address, tok_base)[0]
            if scheme == "pcgs":
                cnt[z[pos]] -= 1
                new = java_walk((cnt.astype(np.float64) + alpha) * phi[:, w], U)
                cnt[new] += 1
            else:
                new = java_walk(theta[d] * phi[:, w], U)
            z[pos] = new
    return z.astype(np.int32)


# ---- a gamma draw that settles at its first try ---------------------------------------------------------------------------
def gamma_first_try(seed, iteration, purpose, elem, shape, address=true_address, base=0):
    """rgamma (oracle/ggs_oracle.c, ParallelRandoms.java:60-70,148-159) where its first Marsaglia-Tsang try is accepted by the
    squeeze: the element's draws 0 (the boost's uniform, taken for every shape), 1 and 2 (the polar pair) and 3 (the accept
    uniform) -- blocks 0 and 1.  None where the polar pair is rejected, v <= 0 or the squeeze does not settle it."""
    u0, a = uniform_pair(seed, iteration, purpose, elem, 0, address, base)
    b, u = uniform_pair(seed, iteration, purpose, elem, 1, address, base)
    v1, v2 = 2 * a - 1, 2 * b - 1
    s = v1 * v1 + v2 * v2
    if s >= 1 or s == 0:
        return None
    x = v1 * float(np.sqrt(-2 * float(O.log([s])[0]) / s))
    boosted = shape < 1
    d = ((1 + shape) if boosted else shape) - (1.0 / 3.0)
    c = 1.0 / float(np.sqrt(9.0 * d))
    v = 1.0 + c * x
    if v <= 0.0:
        return None
    v = v * v * v
    if not u < (1.0 - 0.0331 * (x * x) * (x * x)):
        return None
    g = d * v
    return g * float(O.pow([u0], [1.0 / shape])[0]) if boosted else g
