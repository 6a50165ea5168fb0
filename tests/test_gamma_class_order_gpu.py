"""The gamma draws in shape-class order: theta_kernel and phi_gamma_body against the oracle, bit for bit.

Both kernels draw their cells from a list with the count-0 cells (class A: constants from a per-document or per-column
table) at the front and the others (class B: constants per lane) at the back, 64 list positions per wave.  Which lane draws
a cell must change no bit of it, so every case compares get_theta() / get_phi() bit patterns with OracleSampler: after
set_z (the initial Phi draw from crafted counts), after one sweep (theta drawn from the crafted z) and after two.

The theta cases put an exact number of class-A cells into one workgroup: the seams between waves that hold one class and
the wave that holds both, and the two ends of the list.  A workgroup of 16 documents at K = 100 lists 1 600 cells; since a
non-empty document has a cell with a count, 16 documents give at most 1 584 class-A cells.  1 599 cannot be had in one
workgroup: the case takes 17 documents (1 700 cells listed, 101 of them class B; workgroups of 16 and 1), and 1 535 stands
for its seam, class A ending in the last lane of a wave.
"""
import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus
from tests.ranks import assert_bit_equal

pytestmark = pytest.mark.gpu

SEED = 4242


def pair(native, oracle, c, K, alpha, beta):
    g = native.GGSHandle(K, c.num_types, alpha, beta, SEED, flags=native.FLAG_PARANOID)
    o = oracle.OracleSampler(K, c.num_types, alpha, beta, SEED, threads=4)
    g.set_corpus(c.doc_ptr, c.tokens)
    o.set_corpus(c.doc_ptr, c.tokens)
    return g, o


def run_from(native, oracle, c, K, alpha, beta, z, tag, sweeps=2):
    g, o = pair(native, oracle, c, K, alpha, beta)
    z = np.ascontiguousarray(z, np.int32)
    g.set_z(z, redraw_phi=True)
    o.set_z(z, redraw_phi=True)
    assert_bit_equal(g.get_phi(), o.get_phi(), tag + ": initial phi")
    for s in range(sweeps):
        g.sweep(1)
        o.sweep(1)
        assert_bit_equal(g.get_theta(), o.get_theta(), "%s: theta after sweep %d" % (tag, s + 1))
        assert_bit_equal(g.get_phi(), o.get_phi(), "%s: phi after sweep %d" % (tag, s + 1))
        assert_bit_equal(g.get_z(), o.get_z(), "%s: z after sweep %d" % (tag, s + 1))
    g.close()


def crafted_docs(used, K, V, seed, extra=3):
    """One document per entry of `used`: it uses exactly that many distinct topics (0: an empty document), some of them
    `extra` times over.  Returns the corpus and z."""
    rng = np.random.default_rng(seed)
    zs, lens = [], []
    for u in used:
        t = rng.permutation(K)[:u].astype(np.int32)
        z = np.concatenate([t, rng.choice(t, extra)]) if u else t
        zs.append(rng.permutation(z))
        lens.append(z.size)
    z = np.concatenate(zs).astype(np.int32)
    doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    tokens = rng.integers(0, V, z.size).astype(np.int32)
    return Corpus(doc_ptr, tokens, V), z


def spread(total, docs, K):
    """`total` cells with a count over `docs` non-empty documents: at least one each, at most K"""
    used = np.ones(docs, np.int64)
    left = total - docs
    assert 0 <= left <= docs * (K - 1)
    for d in range(docs):
        take = min(K - 1, left)
        used[d] += take
        left -= take
    return used[::-1].copy()          # the fullest documents last


def class_a_cells(c, z, K):
    n = 0
    for d in range(c.num_docs):
        zd = z[c.doc_ptr[d]:c.doc_ptr[d + 1]]
        if zd.size:
            n += K - np.unique(zd).size
    return n


# ---------------------------------------------------------------- theta: the seams of the list
@pytest.mark.parametrize("n_a,docs", [(0, 16), (1, 16), (63, 16), (64, 16), (65, 16), (1535, 16), (1536, 16), (1584, 16), (1599, 17)])
def test_theta_class_a_count(native, oracle, n_a, docs):
    K = 100
    c, z = crafted_docs(spread(docs * K - n_a, docs, K), K, 50, seed=n_a, extra=0 if n_a == 1584 else 3)
    assert class_a_cells(c, z, K) == n_a and c.num_docs == docs
    if n_a == 1584:
        assert (np.diff(c.doc_ptr) == 1).all()                      # one token per document
    run_from(native, oracle, c, K, 0.1, 0.01, z, "class A = %d" % n_a)


@pytest.mark.parametrize("cap", [0, 3])
@pytest.mark.parametrize("n_a", [64, 65])
def test_theta_draws_on_the_spot_from_both_classes(native, oracle, monkeypatch, n_a, cap):
    """GGS_DEBUG_GAMMA_QUEUE: a queue of 0 or 3 entries sends the first try's leftovers of table waves, of the mixed wave
    and of per-lane waves down the general draw where they stand"""
    monkeypatch.setenv("GGS_DEBUG_GAMMA_QUEUE", str(cap))
    K = 100
    c, z = crafted_docs(spread(16 * K - n_a, 16, K), K, 50, seed=n_a)
    assert class_a_cells(c, z, K) == n_a
    run_from(native, oracle, c, K, 0.1, 0.01, z, "class A = %d, queue of %d" % (n_a, cap))


def test_theta_last_workgroup_is_short(native, oracle):
    """40 documents: workgroups of 16, 16 and 8"""
    K = 100
    rng = np.random.default_rng(40)
    c, z = crafted_docs(rng.integers(1, 60, 40), K, 80, seed=40)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "40 documents")


def test_theta_empty_documents(native, oracle):
    """empty documents in the middle and at the end of a workgroup: their cells are in no class and are not drawn"""
    K = 100
    used = [5, 0, 30, 100, 0, 0, 1, 77, 12, 0, 64, 3, 99, 50, 2, 0]
    c, z = crafted_docs(used, K, 60, seed=16)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "empty documents")
    assert c.num_docs == 16 and (np.diff(c.doc_ptr)[[1, 4, 5, 9, 15]] == 0).all()
    used = list(range(1, 33)) + [0, 9, 0]                            # ... and in a short last workgroup
    c, z = crafted_docs(used, K, 60, seed=17)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "empty documents, 35")


@pytest.mark.parametrize("K", [1, 3])
def test_theta_few_topics(native, oracle, K):
    rng = np.random.default_rng(K)
    c, z = crafted_docs(rng.integers(0, K + 1, 70), K, 20, seed=K, extra=2)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "K = %d" % K)


def test_theta_one_document_per_workgroup(native, oracle):
    """K = 1 024: a workgroup holds one document (two where the first sweep draws), the list K or 2 K entries"""
    K = 1024
    c, z = crafted_docs([1, 700, 1024], K, 90, seed=1024)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "K = 1024")


def test_theta_asymmetric_alpha_has_no_class_a(native, oracle):
    """alpha_k >= 1 beside tiny ones: count-0 cells of one document differ in shape, and those with alpha_k >= 1 do not boost"""
    K = 100
    alpha = np.where(np.arange(K) % 3 == 0, 1.0 + np.arange(K) / 10.0, 1e-3 * (1 + np.arange(K)))
    assert (alpha >= 1).any() and (alpha < 0.01).any()
    c, z = crafted_docs(spread(16 * K - 1000, 16, K), K, 50, seed=5)
    run_from(native, oracle, c, K, alpha, 0.01, z, "asymmetric alpha")
    # the same bits in every entry of an array: symmetric
    run_from(native, oracle, c, K, np.full(K, 0.1), 0.01, z, "alpha as an array of equal entries", sweeps=1)


@pytest.mark.parametrize("alpha", [1.0, 2.5])
def test_theta_class_a_that_does_not_boost(native, oracle, alpha):
    """symmetric alpha >= 1: the table's entries hold boost = false"""
    K = 100
    c, z = crafted_docs(spread(16 * K - 1200, 16, K), K, 50, seed=7)
    run_from(native, oracle, c, K, alpha, 0.01, z, "alpha = %g" % alpha)


# ---------------------------------------------------------------- Phi: tiles of 64 words x <= 6 topics
def every_pair_corpus(words, topics, V, docs=4, seed=0):
    """a token for every (word, topic) pair given, dealt over `docs` documents"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(words))
    tokens, z = np.asarray(words, np.int32)[order], np.asarray(topics, np.int32)[order]
    cuts = np.linspace(0, tokens.size, docs + 1).astype(np.int64)
    return Corpus(cuts, tokens, V), z


@pytest.mark.parametrize("K", [1, 6, 7, 13])
@pytest.mark.parametrize("V", [1, 63, 64, 65, 127])
def test_phi_ragged_tiles(native, oracle, V, K):
    """a last segment of 1, 63 or 64 rows and a last column group of 1 or 6 columns; V = 1: a list shorter than a wave"""
    c = random_corpus(12, V, 30, seed=V * 31 + K)
    z = np.random.default_rng(V + K).integers(0, K, c.num_tokens)
    run_from(native, oracle, c, K, 0.1, 0.01, z, "V = %d, K = %d" % (V, K))


def test_phi_tiles_of_one_class_and_a_split_at_64(native, oracle):
    """K = 6, V = 192: the tile of words 0-63 has a count in every cell (all class B), that of words 64-127 in none (all
    class A), that of words 128-191 in all but 64 (class A fills exactly the first wave)"""
    K, V = 6, 192
    pairs = [(w, k) for w in range(64) for k in range(K)]
    pairs += [(w, k) for w in range(128, 192) for k in range(K) if k != w % K]
    c, z = every_pair_corpus([p[0] for p in pairs], [p[1] for p in pairs], V)
    n = np.zeros((V, K), np.int64)
    np.add.at(n, (c.tokens, z), 1)
    assert (n[:64] > 0).all() and (n[64:128] == 0).all() and (n[128:] == 0).sum() == 64
    run_from(native, oracle, c, K, 0.1, 0.01, z, "one-class tiles")
    # and 63 / 65 class-A cells in the third tile
    for drop in (1, -1):
        q = list(pairs)
        if drop == 1:
            q.append((128, 128 % K))
        else:
            q.remove((129, (129 + 1) % K))
        c, z = every_pair_corpus([p[0] for p in q], [p[1] for p in q], V, seed=drop + 2)
        run_from(native, oracle, c, K, 0.1, 0.01, z, "third tile, class A = %d" % (64 - drop), sweeps=1)


# ---------------------------------------------------------------- the masked draws: a masked cell is in neither class
def test_spalias_priors_masked_cells_inside_a_tile(native, oracle):
    from tests import spalias_priors_restatement as PR
    from tests.test_spalias_priors_gpu import run_pair
    K, V = 7, 70
    c = random_corpus(20, V, 25, seed=3)
    cells = PR.random_cells(np.random.default_rng(3), K, V, 6, 12, np.bincount(c.tokens, minlength=V))
    g, m = run_pair(native, c, K, 0.1, 0.01, 2, cells, each_sweep=lambda g, m, s: assert_bit_equal(g.get_phi(), m.phi, "phi after sweep %d" % s))
    assert (m.P == 0.0).any()
    g.close()


def test_nzvsspalias_undrawn_cells_inside_a_tile(native, oracle):
    from tests.test_nzvs_gpu import run_pair
    g, m = run_pair(native, random_corpus(20, 70, 25, seed=4), 7, 0.1, 0.01, 2)   # compares phi after the initial draw and after every sweep
    undrawn = tuple(g.vs_stats())[0]
    assert 0 < undrawn < 7 * 70                                     # cells the indicator chain left undrawn, beside drawn ones
    phi = g.get_phi()
    assert_bit_equal(phi, m.phi, "phi after the last sweep")
    assert (phi == 0.0).sum() >= undrawn and not np.signbit(phi).any()   # an undrawn cell holds +0.0
    g.close()
