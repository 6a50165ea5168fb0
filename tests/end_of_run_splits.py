"""What tests/test_end_of_run_splits_gpu.py and tests/test_end_of_run_splits_model.py share: how the host side of the end-of-run
features (ggs_host_end_of_run.hpp: the min distances, the topic diagnostics) cuts its work -- pieces of documents, groups of topics, bands
of tiles, pieces of a foreign block, grids that are capped so that a workgroup loops -- restated with the caps named, and the
inputs whose second piece, group, band and third trip the GPU cases compare.

  DOCS_GRID        4096   td_docs_kernel: grid min(nd, 4096), workgroup b takes documents b, b + 4096, ... of the piece (td_doc_launch)
  WTC_GRID         8192   td_wtc_kernel: grid min(V, 8192), a word per workgroup and trip (td_score_launch)
  SEG               256   kTdSegDocs: a piece of documents is whole waves of 256 documents, and at least one
  MIRROR_BLOCKS    2048   grid_for's cap (256 * 8 workgroups), MIRROR_BLOCK = 256 cells each: td_mirror_kernel strides beyond
  TD_PIECE_BYTES  64 MiB  kTdPieceBytes: DOC_CELL_BYTES = 12 per (document, topic) of a piece (TdDocPlan), SORT_CELL_BYTES = 16
                          per (topic, word) of a group (TdScorePlan)
  DIST_PIECE_BYTES 64 MiB kDistPieceBytes: 8 K bytes per row of a piece of the foreign block (ggs_min_doc_distances)
  DIST_BAND_TILES  2^30   kDistBandTiles: a launch covers whole tile rows, at most this many tiles (dist_band_rows)
  ROW_TILE, TOPIC_TILE  64, 16   the tile edges of min_row_dist_kernel and min_topic_dist_kernel

The three knobs replace the three byte / tile constants by clamp(value, 1, constant): knobbed(value,
constant) below.  Every function takes the knob's value (None: none set) and returns the list of piece, group or band sizes."""
import contextlib

import numpy as np

from tests import min_distances_restatement as MR
from tests import topic_diagnostics_restatement as R

DOCS_GRID, WTC_GRID, SEG = 4096, 8192, 256
MIRROR_BLOCKS, MIRROR_BLOCK = 2048, 256
TD_PIECE_BYTES, DOC_CELL_BYTES, SORT_CELL_BYTES = 64 << 20, 12, 16
DIST_PIECE_BYTES = 64 << 20
DIST_BAND_TILES = 1 << 30
ROW_TILE, TOPIC_TILE, TOPIC_CHUNK = 64, 16, 192                     # kDistRowR * 16, kDistTopR * 16, kDistTopKC
KNOB_TD, KNOB_DIST_PIECE, KNOB_DIST_BAND = "GGS_DEBUG_TD_PIECE_BYTES", "GGS_DEBUG_DIST_PIECE_BYTES", "GGS_DEBUG_DIST_BAND_TILES"


@contextlib.contextmanager
def knob(monkeypatch, name, value):
    """the knob around a call, gone after it (the library reads it at every call)"""
    monkeypatch.setenv(name, str(int(value)))
    try:
        yield
    finally:
        monkeypatch.delenv(name)


def knobbed(value, constant):
    """debug_shrunk: a knob can only make pieces smaller"""
    return constant if value is None else max(1, min(constant, int(value)))


def cut(total, size):
    """[size, size, ..., rest]: the loops `for (x0 = 0; x0 < total; x0 += size)`"""
    return [min(size, total - x) for x in range(0, total, size)]


def trips(items, grid_cap):
    """(trips of the busiest workgroup, workgroups that make that many) when item i goes to workgroup i % min(items, cap)"""
    grid = max(1, min(items, grid_cap))
    most = -(-items // grid)
    return most, items - (most - 1) * grid


def doc_pieces(D, K, piece_bytes=None):
    """TdDocPlan::piece and td_doc_launch's loop"""
    piece = knobbed(piece_bytes, TD_PIECE_BYTES) // (DOC_CELL_BYTES * K) // SEG * SEG
    piece = min(max(piece, SEG), max(D, 1))
    return cut(D, piece)


def topic_groups(V, K, piece_bytes=None):
    """TdScorePlan::group and td_score_launch's loop over k0"""
    return cut(K, min(K, max(1, knobbed(piece_bytes, TD_PIECE_BYTES) // (SORT_CELL_BYTES * V))))


def mirror_trips(K, n):
    """td_mirror_kernel: (trips of thread 0, cells of the last trip) over K n n cells on grid_for(cells, 256) workgroups"""
    cells = K * n * n
    grid = max(1, min(-(-cells // MIRROR_BLOCK), MIRROR_BLOCKS))
    return trips(cells, grid * MIRROR_BLOCK)


def dist_bands(n, m, tile, band_tiles=None):
    """launch_min_row_dist / launch_min_topic_dist: tile rows per launch over ceil(n / tile) rows of ceil(m / tile) tiles"""
    ta, tb = -(-n // tile), -(-m // tile)
    return cut(ta, max(1, knobbed(band_tiles, DIST_BAND_TILES) // max(tb, 1)))


def band_of(row, n, m, tile, band_tiles=None):
    """the launch whose tiles hold `row` as a row"""
    return int(np.searchsorted(np.cumsum(dist_bands(n, m, tile, band_tiles)), row // tile, side="right"))


def dist_pieces(n_other, K, piece_bytes=None):
    """ggs_min_doc_distances: rows of the foreign block per upload"""
    return cut(n_other, max(1, min(n_other, knobbed(piece_bytes, DIST_PIECE_BYTES) // (8 * K))))


# ---- the document pass on its second and third trip --------------------------------------------------------------------------
TRIP_D, TRIP_K, TRIP_N, TRIP_V = 2 * DOCS_GRID + 300, 130, 128, 300
TRIP_ALPHA = np.linspace(0.02, 0.9, TRIP_K)
TRIP_GROUP, TRIP_TOPIC = 150, TRIP_K - 1        # the workgroup of the hand-built triple; its topic, which no other document has
LONG, EMPTY, ONE, SHORT = "long", "empty", "one token", "short"


def trip_kinds(b):
    """the kinds of the documents workgroup b takes, in its order (b, b + 4096, b + 8192)"""
    if b < TRIP_D - 2 * DOCS_GRID:
        return (LONG, EMPTY, ONE) if b % 2 == 0 else (ONE, EMPTY, LONG)
    return [(SHORT, EMPTY), (EMPTY, SHORT), (ONE, SHORT), (SHORT, ONE)][b % 4]


_trip = []


def trip_corpus():
    """(doc_ptr, tokens, z, counts, idx): D = 2 x 4096 + 300 documents, so that workgroups 0..299 of td_docs_kernel make three
    trips and the others two, over documents that differ in kind (trip_kinds).  A long document has 300 to 400 tokens: half of
    them under one topic (b % 129: some seventy of its 128 top words, in all four mask words), the others over all of topics
    0..128.  Topic 129 -- the third round of lane 1 -- belongs to workgroup 150's hand-built triple alone: its first document has
    all 128 top words of the topic (words 236..299 twice, 172..235 once: every mask bit set), its second one exactly one of
    them (word 180, position 64 by its count of 2: the first bit of the third mask word) among tokens of other topics, its
    third one two of them in different mask words (words 298 and 173).  idx: the counts' own top words."""
    if _trip:
        return _trip[0]
    rng = np.random.default_rng(4096)
    D, K, V = TRIP_D, TRIP_K, TRIP_V
    docs = []
    for d in range(D):
        b = d % DOCS_GRID
        kind = trip_kinds(b)[d // DOCS_GRID]
        if kind == LONG:
            L = int(rng.integers(300, 401))
            zz = np.where(rng.random(L) < 0.5, b % (K - 1), rng.integers(0, K - 1, L))
        else:
            L = {EMPTY: 0, ONE: 1}.get(kind, int(rng.integers(2, 13)))
            zz = rng.integers(0, K - 1, L)
        docs.append((rng.integers(0, V, L), zz))
    b, k = TRIP_GROUP, TRIP_TOPIC
    all_words = np.concatenate([np.arange(236, 300), np.arange(236, 300), np.arange(172, 236)])
    docs[b] = (all_words, np.full(all_words.size, k))
    docs[b + DOCS_GRID] = (np.array([7, 180, 7, 9, 250]), np.array([3, k, 3, 64, 128]))
    docs[b + 2 * DOCS_GRID] = (np.array([298, 5, 173]), np.array([k, 0, k]))
    lens = np.array([len(w) for w, _ in docs], np.int64)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = np.concatenate([w for w, _ in docs]).astype(np.int32)
    z = np.concatenate([t for _, t in docs]).astype(np.int32)
    counts = np.zeros((V, K), np.int32)
    np.add.at(counts, (tokens, z), 1)
    _trip.append((doc_ptr, tokens, z, counts, R.top_words(counts, TRIP_N)))
    return _trip[0]


def triple_codoc(idx):
    """codoc[129] of trip_corpus(), by hand: 1 everywhere from the document with every top word; the second document adds its one
    word's diagonal cell, the third one the 2 x 2 block of its two words"""
    pos = {int(w): r for r, w in enumerate(idx[TRIP_TOPIC])}
    want = np.ones((TRIP_N, TRIP_N), np.int32)
    want[pos[180], pos[180]] += 1
    for i in (pos[298], pos[173]):
        for j in (pos[298], pos[173]):
            want[i, j] += 1
    return want, (pos[180], pos[298], pos[173])


# ---- pieces of documents -----------------------------------------------------------------------------------------------------
PIECE_DS, PIECE_KS, PIECE_V, PIECE_N = [255, 256, 257, 511, 512, 513, 769], [3, 65], 60, 5


def piece_knob(K):
    return DOC_CELL_BYTES * K * SEG                                   # a piece of exactly 256 documents


def piece_case(D, K):
    """(doc_ptr, tokens, z, counts): Poisson lengths, with the last document before and the first one behind every piece
    boundary empty at 256 and the two on either side of 512 holding tokens around an empty pair further out"""
    lens = np.random.default_rng([D, K, 5]).poisson(9, D)
    for d in (255, 256, 509, 514):
        if d < D:
            lens[d] = 0
    for d in (510, 511, 512, 513):
        if d < D:
            lens[d] = max(lens[d], 1)
    return R.random_case(D, PIECE_V, K, 6, lengths=lens)


# ---- groups of topics --------------------------------------------------------------------------------------------------------
GROUP_CASES = [(300, 1, 3), (300, 2, 5), (257, 64, 63), (257, 64, 64), (257, 64, 65), (257, 64, 129)]      # (V, g, K)
BIG_V, BIG_K, BIG_N = 70000, 61, 20                                  # no knob: 64 MiB / (16 x 70 000) = 59 topics per launch
DENSE, HOLED, EMPTY_COL, THIRD_DIGIT = "dense", "one zero cell", "empty", "third digit pass"


def group_knob(V, g):
    return SORT_CELL_BYTES * V * g


def sparse_tied_counts(V, K, seed):
    """test_sorted_chains_shapes' counts: sparse, many ties; column 0 without a zero"""
    rng = np.random.default_rng([V, K, seed])
    counts = (rng.integers(0, 4, (V, K)) * (rng.random((V, K)) < 0.4)).astype(np.int32)
    counts[:, 0] = rng.integers(1, 4, V)
    return counts


def group_counts(V, g, K):
    """(counts [V][K], {kind: column}): sparse tied counts, and behind the first group of g topics as many of the four built
    columns as there are columns (all four from K - g = 4 on): a dense one (finite uniform_dist and corpus_dist), the same
    column with exactly one zero cell (NaN, NaN, a finite eff_num_words), an empty one, one whose largest count (70 000) needs
    a third 8-bit digit pass.  Where fewer columns lie behind the first group, the dense column carries the large count and
    the later kinds are left out; with one column only, that column is the one-zero-cell copy of column 0.  A single group
    (K <= g) takes them in its last columns."""
    counts = sparse_tied_counts(V, K, g)
    rng = np.random.default_rng([V, K, g, 1])
    first = g if K > g else max(0, K - 4)
    slots = []
    for k in (first, K - 1, first + 1, K - 2):                       # a group's first and last topic, then their neighbours
        if first <= k < K and k not in slots and k != 0:
            slots.append(k)
    where = {}
    dense = rng.integers(1, 9, V).astype(np.int32)
    if len(slots) == 1:
        where[HOLED] = slots[0]
        counts[:, slots[0]] = counts[:, 0]
        counts[V // 2, slots[0]] = 0
    else:
        if len(slots) < 4:
            dense[V // 3] = 70000
        where[DENSE], where[HOLED] = slots[0], slots[1]
        counts[:, slots[0]] = dense
        counts[:, slots[1]] = dense
        counts[V // 2, slots[1]] = 0
        if len(slots) >= 3:
            where[EMPTY_COL] = slots[2]
            counts[:, slots[2]] = 0
        if len(slots) >= 4:
            where[THIRD_DIGIT] = slots[3]
            counts[V // 5, slots[3]] = 70000
            counts[V // 7, slots[3]] = 65536
    return counts, where


def columns_differ(counts):
    return len({counts[:, k].tobytes() for k in range(counts.shape[1])}) == counts.shape[1]


def big_counts():
    counts = sparse_tied_counts(BIG_V, BIG_K, 0)
    counts[:, BIG_K - 1] = counts[:, 0]
    counts[BIG_V // 2, BIG_K - 1] = 0
    return counts


WTC_V, WTC_KS = 2 * WTC_GRID + 5, [3, 65]
MIRROR_K, MIRROR_N, MIRROR_D, MIRROR_V = 33, 128, 60, 200


# ---- bands of distance tiles -------------------------------------------------------------------------------------------------
def band_knobs(m, tile):
    """less than one tile row (the floor: one row per launch), exactly one row, two rows and a tile more"""
    tb = -(-m // tile)
    return [1, tb, 2 * tb + 1]


BAND_ROW_SELF, BAND_ROW_FOREIGN, BAND_TOPIC = [129, 257], (129, 200), [(33, TOPIC_CHUNK + 1), (49, 2 * TOPIC_CHUNK + 1)]
BAND_ROW_LEN = 33                                                    # one more than kDistRowKC
TWIN, NEAR = 2, 5                                                    # row n - 2 is row 2 again; row n - 1 is the nearest partner of row 5


def band_rows(n, length, seed):
    """Dirichlet rows; row n - 2 equals row 2 (distance 0 across tiles) and row n - 1 is nearer to row 5 than any random row"""
    a = MR.dirichlet_rows(n, length, seed)
    a[n - 2] = a[TWIN]
    a[n - 1] = a[NEAR] * (1 - 2.0 ** -30)
    return a


def foreign_rows(a, m, seed):
    """a block whose last row is the nearest partner of row 5 of a and whose first row is a's row 2 (and n - 2) itself"""
    b = MR.dirichlet_rows(m, a.shape[1], seed)
    b[m - 1] = a[NEAR] * (1 - 2.0 ** -31)
    b[0] = a[TWIN]
    return b


# ---- pieces of the foreign block ---------------------------------------------------------------------------------------------
FOREIGN_RS = [1, 64, 65]
FIRST_DOC, LAST_DOC = 100, 3       # the documents whose nearest partners are the block's first and last row


def foreign_sizes(r):
    return [x for x in (r - 1, r, r + 1, 2 * r + 1) if x >= 1]


def foreign_knob(K, r):
    return 8 * K * r


def nan_row(n_other, r):
    """a row of a middle piece, where there are three pieces"""
    return r + r // 2 if len(cut(n_other, r)) >= 3 else None


def foreign_block(theta, n_other, r, seed):
    other = MR.dirichlet_rows(n_other, theta.shape[1], seed)
    other[n_other - 1] = theta[LAST_DOC] * (1 - 2.0 ** -30)
    if n_other > 1:
        other[0] = theta[FIRST_DOC] * (1 - 2.0 ** -30)
    if nan_row(n_other, r) is not None:
        other[nan_row(n_other, r)] = np.nan
    return other
