"""What tests/test_persistent_grid_gpu.py shares: the corpora whose length-sorted order hands a workgroup a long document,
then a short one, then a one-token one, then an empty one; and the arithmetic that says how many work items a workgroup
of a persistent grid takes (its loop trips) under a given CU count -- restated from the host code, with the caps named.

Every persistent launch goes through launch() (ggs_host_state.hpp): grid = min(ceil(items / waves), CUs x per_cu) workgroups
of `waves` waves, an item per wave and trip.  per_cu is what the plan allows at most (plan_launches, ggs_host_plan.hpp, but where
another function is named):

  CAP_WAVE      32   the single-wave document kernels: pcgs_wave (pl.wave), lightpc (pl.lightpc), spalias and
                     polyaurn_sparse (ggs_set_corpus, ggs_api.hip) -- min(what LDS and registers allow, 32)
  CAP_LANE       8   the lane-per-document kernels, one wave of 64 documents per workgroup (pl.lane); the ggs tile and
                     streaming kernels (pl.z)
  CAP_WORDLIST   8   word_list_build_kernel, workgroups of WORDLIST_WAVES = 4 waves, a word per wave (pl.wordlist)
  CAP_ALIAS     16   alias_build_kernel, alias_words_per_block(K) words per workgroup and trip (pl.alias, ggs_alias.hpp:39)
  CAP_POISSON    2   phi_poisson_kernel: tiles of rows_per_tile rows, two workgroups per CU (phi_slice_poisson, ggs_host_phi.hpp)
  CAP_SLICED     1   the ggs score-register kernels: one workgroup of SLICED_WAVES = 4 waves per CU (pl.cold, pl.hot, pl.warm)
  CAP_VSBITS    32   vs_bits_kernel (nzvsspalias): a wave per 32-cell word of 64 topics (plan_launches, pl.vsbits)
  CAP_WORDMASK   8   word_list_mask_kernel (nzvsspalias): as word_list_build_kernel, a word per wave (pl.wordmask)
nzvs_wave_kernel takes CAP_WAVE like the other sparse walks (resident_waves_per_cu: 32 at most).

A plan may give fewer than the cap (LDS, registers), never more: a bound computed with the cap holds for the real grid."""
import numpy as np

from ldagroupedgibbssampler_amd.corpus import Corpus

CAP_WAVE, CAP_LANE, CAP_WORDLIST, CAP_ALIAS, CAP_POISSON, CAP_SLICED = 32, 8, 8, 16, 2, 1
CAP_VSBITS, CAP_WORDMASK = 32, 8
WORDLIST_WAVES, SLICED_WAVES = 4, 4
POISSON_THREADS = 1024                  # kPoissonThreads (ggs_phi_poisson.hpp:23)
KNOB = "GGS_DEBUG_NUM_CUS"


def min_trips(items, cus, cap, waves=1):
    """trips of the busiest workgroup when the plan gives the entry its cap: ceil(ceil(items / waves) / (cus * cap))"""
    groups = -(-int(items) // waves)
    return -(-groups // (cus * cap))


def assert_trips(items, cus, cap, what, waves=1, trips=3):
    """some workgroup takes at least `trips` items: items >= trips x cus x cap (x waves)"""
    assert items >= trips * cus * cap * waves, "%s: %d items on %d CU(s) x %d x %d waves: no workgroup takes %d" % (what, items, cus, cap, waves, trips)
    assert min_trips(items, cus, cap, waves) >= trips


def alias_words_per_block(K):
    return max(1, min(64, 48 * 1024 // (12 * K)))                 # ggs_alias.hpp:38-39


def alias_items(V, K):
    return -(-V // alias_words_per_block(K))                      # launch_alias_build, ggs_host_phi.hpp


def vs_bits_items(V, K):
    return -(-V // 32) * -(-K // 64)                               # launch_vs_chain: vs_W words x ceil(Ks / 64) (ggs_host_phi.hpp)


def poisson_tiles(V, K, cus):
    """phi_slice_poisson (ggs_host_phi.hpp) for the whole vocabulary and all K topics"""
    cells = V * K
    want = max(POISSON_THREADS, cells // (cus * 8))
    rows_per_tile = max(1, min(V, -(-want // K)))
    return -(-V // rows_per_tile)


# (documents, shortest, longest) per kind; the documents are shuffled, the device sorts them by length
WAVE_KINDS = [(8, 260, 320), (32, 129, 180), (50, 2, 40), (70, 1, 1), (40, 0, 0)]          # 200 documents
LANE_KINDS = [(16, 130, 200), (496, 10, 40), (512, 2, 8), (512, 1, 1), (170, 0, 0)]        # 1706 documents: 27 groups of 64


def mixed_corpus(kinds, V, seed):
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.integers(lo, hi + 1, n) for n, lo, hi in kinds])
    rng.shuffle(lens)
    doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    p = 1.0 / np.arange(1, V + 1)
    tokens = rng.choice(V, int(doc_ptr[-1]), p=p / p.sum()).astype(np.int32)
    return Corpus(doc_ptr, tokens, int(V))


def assert_kinds(c):
    """over 128 tokens (the chunk look-ahead is live when the document ends), one-token and empty documents"""
    lens = np.diff(c.doc_ptr)
    assert (lens > 128).sum() >= 8 and (lens == 1).sum() >= 50 and (lens == 0).sum() >= 30 and ((lens > 1) & (lens <= 64)).sum() >= 40


def short_corpus(D, V, seed):
    """the real grid's: lengths 0..5"""
    return mixed_corpus([(D, 0, 5)], V, seed)


def doc_topic_counts(doc_ptr, z, K):
    doc_of = np.repeat(np.arange(len(doc_ptr) - 1), np.diff(doc_ptr))
    out = np.zeros((len(doc_ptr) - 1, K), np.int32)
    np.add.at(out, (doc_of, np.asarray(z, np.int64)), 1)
    return out
