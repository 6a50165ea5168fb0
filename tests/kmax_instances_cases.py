"""What tests/test_kmax_instances_gpu.py and tests/test_kmax_instances_model.py share: the case list (nine legs x the 24
instances KMAX = 8, 16, .., 192 of the score-register z kernels x two K per instance), the two corpora, and the launch planner's
arithmetic for these kernels restated with the constants named -- which instance GGS_KMAX_SWITCH and collapsed_kernel_for
(csrc/ggs_host_plan.hpp) give a K, and the LDS layout functions of csrc/ggs_z_sliced.hpp and csrc/ggs_z_pcgs.hpp that size the
hot, pair and warm tables.

  MAX_LDS          160 KiB  kMaxLdsBytes: the LDS of a CU
  GRANULE          2048     kLdsGranule: LDS is handed out in granules
  SLICED_WAVES     4        kSlicedWaves: waves of a workgroup of the ggs kernels
  CHUNK_DOCS       2        kChunkDocs: theta rows of a cold / hot chunk;  HOT_PAIR_DOCS = 2 (kHotPairDocs): of a pair-chunk
  SLICE_TOPICS     16       kSliceTopics: fp64 topics of a ring slice;  SLICE32_TOPICS = 32 (kSlice32Topics): float32 topics
  RING_SLOTS       2        kRingSlots: slots of the ggs kernels' ring;  PCGS_RING_SLOTS = 3 (kPcgsRingSlots): of the lane kernels'
  SLICE_BYTES      8192     kSliceBytes: 64 rows x 128 bytes, one ring slot
  HOT_TAIL         64       kHotTailBytes: zeroed bytes behind a table
  WARM_THETA_PAD   16       kWarmThetaPad;  WARM_LANE_DOUBLES = 12 (GGS_WARM_LANE_DOUBLES): warm_docs_for's budget
  WARM_MIN_ROWS    16       plan_launches: a warm tier of fewer rows is no tier (warm_cap < 16 -> 0)
  TABLE_MAX_ROWS   255      a table row index is 8 bits of the chunk token word
  *_WAVE_FROM      176, 96, 168   kPcgsWaveFromTopics, kCollapsedWaveFromTopics, kPolyaurnWaveFromTopics: above them the
                            wave-per-document kernel serves unless GGS_DEBUG_PCGS_WAVE=0;  SLICED_DEFAULT = 160
                            (kSlicedDefaultTopics): above it the ggs kernels want GGS_DEBUG_ZKERNEL=1"""
import numpy as np

from ldagroupedgibbssampler_amd.corpus import Corpus

MAX_LDS, GRANULE = 160 * 1024, 2048
SLICED_WAVES, CHUNK_DOCS, HOT_PAIR_DOCS = 4, 2, 2
SLICE_TOPICS, SLICE32_TOPICS, RING_SLOTS, PCGS_RING_SLOTS, SLICE_BYTES = 16, 32, 2, 3, 8192
HOT_TAIL, WARM_THETA_PAD, WARM_LANE_DOUBLES, WARM_MIN_ROWS, TABLE_MAX_ROWS = 64, 16, 12, 16, 255
SLICED_MAX, SLICED_DEFAULT = 192, 160
PCGS_WAVE_FROM, COLLAPSED_WAVE_FROM, POLYAURN_WAVE_FROM = 176, 96, 168

KMAXES = tuple(range(8, 193, 8))
GGS_LEGS = ("cold32", "cold64", "fused", "hot", "pairs", "warm")
LANE_LEGS = ("pcgs", "collapsed", "polyaurn")
LEGS = GGS_LEGS + LANE_LEGS
KERNEL_OF = {"cold32": "z_sliced32_kernel", "cold64": "z_sliced_kernel", "fused": "z_sliced32_kernel (hot chunks)", "hot": "z_hot_kernel",
             "pairs": "z_pairs_kernel", "warm": "z_warm_kernel", "pcgs": "pcgs_sliced_kernel<KMAX>", "collapsed": "pcgs_sliced_kernel<KMAX, true>",
             "polyaurn": "polyaurn_sliced_kernel"}

# GGS_KMAX_SWITCH and collapsed_kernel_for: `switch ((K + 7) / 8)`, case -> the template argument; every other value: DEFAULT
SWITCH = {1: 8, 2: 16, 3: 24, 4: 32, 5: 40, 6: 48, 7: 56, 8: 64, 9: 72, 10: 80, 11: 88, 12: 96, 13: 104, 14: 112, 15: 120, 16: 128,
          17: 136, 18: 144, 19: 152, 20: 160, 21: 168, 22: 176, 23: 184}
SWITCH_DEFAULT = 192


def instance_for(K):
    """the KMAX of the instance the planner launches for K topics"""
    return SWITCH.get((K + 7) // 8, SWITCH_DEFAULT)


def ks_of(kmax):
    """the two K of an instance: a full row, and its smallest K (odd, seven padding topics)"""
    return (kmax, kmax - 7)


CASES = tuple((leg, kmax, K) for leg in LEGS for kmax in KMAXES for K in ks_of(kmax))          # 9 x 24 x 2 = 432


def case_id(case):
    return "%s-KMAX%d-K%d" % case


# ---------------------------------------------------------------- the layout functions (bytes)
def round_up(x, unit):
    return (x + unit - 1) // unit * unit


def sliced_kmax(K):
    return (K + 7) // 8 * 8


def sliced_slices(K):
    return (sliced_kmax(K) + SLICE_TOPICS - 1) // SLICE_TOPICS


def sliced_ring_base(K):
    return round_up(max(CHUNK_DOCS * sliced_kmax(K) * 8, sliced_slices(K) * 128), 256)


def sliced_cold_lds(K):
    return SLICED_WAVES * (sliced_ring_base(K) + RING_SLOTS * SLICE_BYTES)


def table_row_pitch(K):
    return sliced_kmax(K) // 8 * 64 + 16


def sliced_fused_lds(K, rows):
    """what launch_info()["lds_bytes_z"] reports for the score-register ggs kernels: the cold workgroup and a table of `rows`"""
    return sliced_cold_lds(K) + rows * table_row_pitch(K)


def hot_wave_lds(K):
    return round_up(CHUNK_DOCS * sliced_slices(K) * SLICE_TOPICS * 8, 256)


def warm_docs_for(kmax):
    rowd = round_up(kmax, SLICE_TOPICS)
    d = WARM_LANE_DOUBLES // 2 if rowd <= 112 else WARM_LANE_DOUBLES // 2 - 1 if rowd <= 128 else 2
    return min(8, max(2, d))


def warm_wave_lds(K):
    return round_up(warm_docs_for(sliced_kmax(K)) * (sliced_slices(K) * SLICE_TOPICS * 8 + WARM_THETA_PAD), 256)


def pairs_record_pitch(K):
    return (sliced_slices(K) | 1) * 8


def pairs_wave_lds(K):
    return round_up(HOT_PAIR_DOCS * sliced_slices(K) * SLICE_TOPICS * 8 + 64 * pairs_record_pitch(K), 256)


def table_rows_beside_cold(K, wave_lds):
    room = (MAX_LDS - round_up(sliced_cold_lds(K), GRANULE) - SLICED_WAVES * wave_lds) // GRANULE * GRANULE - HOT_TAIL
    return max(0, min(TABLE_MAX_ROWS, room // table_row_pitch(K)))      # room >= -HOT_TAIL > -pitch: floor and truncation agree


def table_rows_fused(K):
    return max(0, min(TABLE_MAX_ROWS, (MAX_LDS - sliced_cold_lds(K)) // table_row_pitch(K)))


def lane_lds(K):
    """pcgs_sliced_lds_bytes, as tests/test_scheme_plan_gpu.py restates it"""
    kmax = sliced_kmax(K)
    return (kmax * 8 + kmax * 128 + 255) // 256 * 256 + PCGS_RING_SLOTS * SLICE_BYTES


# ---------------------------------------------------------------- the knobs of a leg and the table they leave it
HOT = 64            # GGS_DEBUG_HOT of the table legs: the planner's capacity where that is smaller (KMAX >= 112 for the pair-chunks)
WARM_HOT, WARM_ROWS, WARM_TIERS = 8, 16, 8          # the "warmsparse" settings of tests/test_parity_gpu.py
SLICED = {"GGS_DEBUG_ZKERNEL": "1"}
ENV = {
    "cold32": dict(SLICED, GGS_DEBUG_HOT="0", GGS_DEBUG_WARM="0", GGS_DEBUG_PHI64="0", GGS_DEBUG_REPLAYS="1"),
    "cold64": dict(SLICED, GGS_DEBUG_HOT="0", GGS_DEBUG_WARM="0", GGS_DEBUG_PHI64="1", GGS_DEBUG_REPLAYS="1"),
    "fused": dict(SLICED, GGS_DEBUG_SPLIT="0", GGS_DEBUG_HOT=str(HOT), GGS_DEBUG_WARM="0"),
    "hot": dict(SLICED, GGS_DEBUG_SPLIT="2", GGS_DEBUG_HOT=str(HOT), GGS_DEBUG_HOT_PAIRS="0", GGS_DEBUG_WARM="0"),
    "pairs": dict(SLICED, GGS_DEBUG_SPLIT="2", GGS_DEBUG_HOT=str(HOT), GGS_DEBUG_WARM="0"),
    "warm": dict(SLICED, GGS_DEBUG_WARM=str(WARM_TIERS), GGS_DEBUG_WARM_ROWS=str(WARM_ROWS), GGS_DEBUG_WARM_FILL="1", GGS_DEBUG_HOT=str(WARM_HOT),
                 GGS_DEBUG_WARM_CPW="0"),
    "pcgs": {"GGS_DEBUG_PCGS_WAVE": "0"}, "collapsed": {"GGS_DEBUG_PCGS_WAVE": "0"}, "polyaurn": {"GGS_DEBUG_PCGS_WAVE": "0"},
}


def hot_rows(leg, K):
    """rows of the hot table plan_launches gives the leg (LaunchPlan::hot_cap)"""
    if leg in ("cold32", "cold64"):
        return 0
    if leg == "fused":
        return min(HOT, table_rows_fused(K))
    if leg == "hot":
        return min(HOT, table_rows_beside_cold(K, hot_wave_lds(K)))
    if leg == "pairs":
        return min(HOT, table_rows_beside_cold(K, max(hot_wave_lds(K), pairs_wave_lds(K))))
    assert leg == "warm"                                # the split form is possible, so the hot table leaves room for the pairs' records
    return min(WARM_HOT, table_rows_beside_cold(K, max(hot_wave_lds(K), pairs_wave_lds(K))))


def warm_rows(K):
    """rows of a warm tier (LaunchPlan::warm_cap) under the warm leg's knobs: 0 where the planner refuses the tiers"""
    cap = table_rows_beside_cold(K, warm_wave_lds(K))
    return 0 if cap < WARM_MIN_ROWS else min(cap, WARM_ROWS)


# ---------------------------------------------------------------- the corpora
GGS_V, GGS_SEED = 400, 20261
GGS_EDGE_LENGTHS = (0, 1, 63, 64, 65, 150)
MIN_TABLE_SHARE = 0.30


def ggs_corpus():
    """One corpus for the six ggs legs, about 2 400 tokens over V = 400 words: documents of 0, 1, 63, 64, 65 and 150 tokens, then
    ragged ones (0 .. 47 tokens, every ninth empty); words Zipf-like by id (p ~ 1 / (w + 1): word 0 the most frequent, the 30
    most frequent words take more than half of the tokens); word V - 1, the last phiT row, is the one-token document's token
    and occurs in the documents of 65 and 150 tokens."""
    rng = np.random.default_rng(GGS_SEED)
    lengths = list(GGS_EDGE_LENGTHS) + [0 if j % 9 == 4 else 3 + (j * 29) % 45 for j in range(75)]
    p = 1.0 / (1.0 + np.arange(GGS_V))
    docs = [rng.choice(GGS_V, n, p=p / p.sum()).astype(np.int32) for n in lengths]
    docs[1][0] = GGS_V - 1
    docs[4][0] = GGS_V - 1
    docs[5][[7, 70, 149]] = GGS_V - 1
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return Corpus(ptr, np.concatenate(docs).astype(np.int32), GGS_V)


def table_share(c, rows, skip=0):
    """the share of the corpus' tokens that belong to the words of ranks skip .. skip + rows - 1 by frequency (ties at either end
    change which words those are, not the sum)"""
    counts = np.sort(np.bincount(c.tokens, minlength=c.num_types))[::-1]
    return counts[skip:skip + rows].sum() / c.num_tokens


LANE_V, LANE_SEED = 120, 20262
LANE_MIN_STEPS = 3


def lane_lengths():
    """70 documents: a full group of 64 and a ragged one of 6.  The kernels take the documents longest first, a group steps as
    often as its longest document is long: no more than five documents are shorter than LANE_MIN_STEPS tokens, so that the
    ragged group -- the six shortest -- still makes that many steps."""
    return np.array([0, 1, 0, 1, 2] + [3 + (j * 11) % 28 for j in range(65)], np.int64)


def lane_corpus():
    rng = np.random.default_rng(LANE_SEED)
    lengths = rng.permutation(lane_lengths())
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return Corpus(ptr, rng.integers(0, LANE_V, int(ptr[-1])).astype(np.int32), LANE_V)


def lane_group_steps(c):
    """steps of each group of 64 documents in the lane-per-document kernels' order (pcgs_order: longest first, stable)"""
    lens = np.sort(np.diff(c.doc_ptr))[::-1]
    return [int(lens[g]) for g in range(0, lens.size, 64)]


# ---------------------------------------------------------------- the float32 cold path's decided share
SEED, ZSEED, ALPHA, BETA, SWEEPS = 4242, 11, 0.1, 0.01, 2
REPLAY_CAP = 0.03                                        # cold32: at most this share of the sampled tokens replayed


def oracle_run(oracle, scheme, c, K, record=None):
    """the CPU authority's run of a leg's scheme over corpus c: SWEEPS sweeps from the Java-LCG start; `record(o, Phi before the
    sweep)` is called after every sweep"""
    o = oracle.OracleSampler(K, c.num_types, ALPHA, BETA, SEED, threads=4)
    if scheme == "pcgs":
        o.set_scheme("pcgs")
    o.set_corpus(c.doc_ptr, c.tokens)
    o.init_z_java_lcg(ZSEED)
    o.init_phi()
    for _ in range(SWEEPS):
        before = o.get_phi() if record else None
        if scheme == "collapsed":
            o.collapsed_parallel_sweep(1)
        else:
            o.sweep(1)
        if record:
            record(o, before)
    return o
