"""tests/test_kmax_instances_gpu.py reaches what it claims, shown on the CPU from the constants restated in
tests/kmax_instances_cases.py: the case list covers each of the 24 instances of each of the nine legs, both K of a case
select that instance in the planner's switch, the hot, pair and warm tables have rows at every KMAX and take at least 30 % of
the shared corpus' tokens at the capacity each KMAX gets, the lane corpus gives each of its groups three steps and more, and
the float32 cold path decides all but a sliver of the corpus' draws (the numpy model of tests/test_margin32_model.py on the
oracle's theta, Phi and uniforms of both sweeps)."""
import numpy as np
import pytest

from tests import kmax_instances_cases as C
from tests.test_margin32_model import kernel_rule


# ---------------------------------------------------------------- the case list and the switch
def test_case_list_covers_every_instance_of_every_leg():
    assert len(C.CASES) == len(set(C.CASES)) == 9 * 24 * 2 == 432
    assert C.KMAXES == tuple(range(8, 193, 8)) and len(C.KMAXES) == 24
    assert len(C.LEGS) == len(set(C.LEGS)) == 9 and set(C.KERNEL_OF) == set(C.ENV) == set(C.LEGS)
    for leg in C.LEGS:
        reached = {}
        for l, kmax, K in C.CASES:
            if l == leg:
                reached.setdefault(C.instance_for(K), []).append(K)
        assert sorted(reached) == list(C.KMAXES), (leg, sorted(reached))
        assert all(len(ks) == 2 for ks in reached.values()), leg


@pytest.mark.parametrize("kmax", C.KMAXES)
def test_both_k_of_a_case_select_its_instance(kmax):
    full, smallest = C.ks_of(kmax)
    assert full == kmax and smallest == kmax - 7 and smallest % 2 == 1 and 1 <= smallest
    for K in (full, smallest):
        assert (K + 7) // 8 * 8 == kmax == C.sliced_kmax(K)
        assert C.instance_for(K) == kmax, "the restated switch sends K = %d to KMAX = %d" % (K, C.instance_for(K))
        assert K <= C.SLICED_MAX
    assert C.instance_for(smallest - 1) != kmax or smallest == 1          # the instance's smallest K
    assert C.instance_for(full + 1) != kmax or full == C.SLICED_MAX       # ... and its largest
    # Kp = K + 1 at the odd K; the float32 rows are whole 32-topic slices, which can reach past KMAX (K = 33: KMAX 40, Kp32 64)
    assert (smallest + 1) & ~1 == smallest + 1
    assert C.round_up(smallest, C.SLICE32_TOPICS) >= kmax - 7


def test_the_switch_is_the_rounding_up_to_eight_topics():
    assert sorted(C.SWITCH) == list(range(1, 24)) and C.SWITCH_DEFAULT == 192
    for K in range(1, C.SLICED_MAX + 1):
        assert C.instance_for(K) == (K + 7) // 8 * 8, K
    assert C.round_up(33, C.SLICE32_TOPICS) == 64 > C.instance_for(33) == 40


def test_instances_reachable_only_through_a_knob():
    """what DESIGN.md's coverage table says of the defaults: above these K the planner gives the work to another kernel"""
    knob_only = {"ggs": [k for k in C.KMAXES if k - 7 > C.SLICED_DEFAULT], "pcgs": [k for k in C.KMAXES if k - 7 > C.PCGS_WAVE_FROM],
                 "collapsed": [k for k in C.KMAXES if k - 7 > C.COLLAPSED_WAVE_FROM], "polyaurn": [k for k in C.KMAXES if k - 7 > C.POLYAURN_WAVE_FROM]}
    assert knob_only == {"ggs": [168, 176, 184, 192], "pcgs": [184, 192], "collapsed": list(range(104, 193, 8)), "polyaurn": [176, 184, 192]}
    for leg in C.GGS_LEGS:
        assert C.ENV[leg]["GGS_DEBUG_ZKERNEL"] == "1"
    for leg in C.LANE_LEGS:
        assert C.ENV[leg]["GGS_DEBUG_PCGS_WAVE"] == "0"


# ---------------------------------------------------------------- the tables
def test_layout_restatement_at_known_points():
    """figures the sources state: 96 hot rows beside the cold kernel and 79 with the pair-chunks at K = 100, about 30 rows for the
    pairs at 192, six documents per warm chunk up to KMAX 112, five up to 128, two beyond"""
    assert C.table_rows_beside_cold(100, C.hot_wave_lds(100)) == 96
    assert C.table_rows_beside_cold(100, max(C.hot_wave_lds(100), C.pairs_wave_lds(100))) == 79
    assert C.table_rows_beside_cold(192, max(C.hot_wave_lds(192), C.pairs_wave_lds(192))) == 30
    assert [C.warm_docs_for(k) for k in (8, 104, 112, 120, 128, 136, 192)] == [6, 6, 6, 5, 5, 2, 2]
    assert C.table_row_pitch(100) == 104 * 8 + 16 and C.pairs_record_pitch(100) == 7 * 8 and C.pairs_record_pitch(128) == 9 * 8
    assert C.sliced_ring_base(8) == 256 and C.sliced_ring_base(192) == 2 * 192 * 8
    assert C.lane_lds(8) == 1280 + 3 * 8192 and C.lane_lds(185) == 192 * 136 + 3 * 8192


@pytest.mark.parametrize("kmax", C.KMAXES)
def test_every_table_leg_has_a_table_at_every_kmax(kmax):
    c = C.ggs_corpus()
    for K in C.ks_of(kmax):
        assert C.table_rows_fused(K) > 0 and C.table_rows_beside_cold(K, C.hot_wave_lds(K)) > 0
        assert C.table_rows_beside_cold(K, max(C.hot_wave_lds(K), C.pairs_wave_lds(K))) > 0
        for leg in ("fused", "hot", "pairs"):
            rows = C.hot_rows(leg, K)
            assert 0 < rows <= C.HOT
            assert C.table_share(c, rows) >= C.MIN_TABLE_SHARE, (leg, K, rows, C.table_share(c, rows))
            assert rows < np.count_nonzero(np.bincount(c.tokens)), "cold words remain: the split form wants cold and hot chunks"
        # the warm leg: the planner keeps the tiers at every KMAX (a capacity below WARM_MIN_ROWS would mean none: the GPU case
        # then asserts their absence), the hot table is full, so the tiers are built, and they take the share
        cap = C.table_rows_beside_cold(K, C.warm_wave_lds(K))
        assert cap >= C.WARM_MIN_ROWS and C.warm_rows(K) == C.WARM_ROWS, (K, cap)
        assert C.hot_rows("warm", K) == C.WARM_HOT
        warm_words = min(C.WARM_TIERS * C.warm_rows(K), np.count_nonzero(np.bincount(c.tokens)) - C.WARM_HOT)
        assert warm_words == C.WARM_TIERS * C.WARM_ROWS
        assert C.table_share(c, warm_words, skip=C.WARM_HOT) >= C.MIN_TABLE_SHARE
        assert C.table_share(c, warm_words) >= C.MIN_TABLE_SHARE
    assert C.hot_rows("cold32", kmax) == C.hot_rows("cold64", kmax) == 0


def test_table_capacity_shrinks_with_kmax_and_the_pairs_take_rows():
    for wave_lds in (C.hot_wave_lds, lambda K: max(C.hot_wave_lds(K), C.pairs_wave_lds(K)), C.warm_wave_lds):
        rows = [C.table_rows_beside_cold(k, wave_lds(k)) for k in C.KMAXES if k <= 128]       # beyond 128 a warm chunk has fewer theta rows
        assert rows == sorted(rows, reverse=True)
    for k in C.KMAXES:
        assert C.hot_rows("pairs", k) <= C.hot_rows("hot", k) <= C.hot_rows("fused", k)
    assert C.hot_rows("pairs", 192) < C.HOT                         # the planner's capacity, not the knob, at the large instances


# ---------------------------------------------------------------- the corpora
def test_shared_corpus_has_the_edge_documents_and_words():
    c = C.ggs_corpus()
    lens = np.diff(c.doc_ptr)
    assert c.num_tokens <= 2500 and c.num_types == C.GGS_V
    for n in C.GGS_EDGE_LENGTHS:
        assert (lens == n).any(), n
    counts = np.bincount(c.tokens, minlength=c.num_types)
    assert counts[0] == counts.max() > 0 and counts[c.num_types - 1] > 0
    assert c.tokens[c.doc_ptr[1]] == c.num_types - 1 and lens[1] == 1
    assert C.table_share(c, 30) > 0.5                                # a Zipf-like head
    assert c.num_tokens // 64 >= 2 * C.SLICED_WAVES                  # cold chunks for every wave of a workgroup, and a second one


def test_lane_corpus_gives_each_group_three_steps():
    c = C.lane_corpus()
    lens = np.diff(c.doc_ptr)
    assert c.num_docs == 70 and lens.min() == 0 and (lens == 1).any() and lens.max() == 30 and 900 <= c.num_tokens <= 1200
    steps = C.lane_group_steps(c)
    assert len(steps) == 2 and min(steps) >= C.LANE_MIN_STEPS, steps
    # a step moves the ring's start slot by NS slices: three steps and more visit every slot the instance can start at
    for kmax in C.KMAXES:
        ns = (kmax + C.SLICE_TOPICS - 1) // C.SLICE_TOPICS
        starts = {(t * ns) % C.PCGS_RING_SLOTS for t in range(min(steps))}
        assert starts == {(t * ns) % C.PCGS_RING_SLOTS for t in range(3 * C.PCGS_RING_SLOTS)}, kmax


# ---------------------------------------------------------------- the float32 cold path
@pytest.mark.parametrize("kmax", C.KMAXES)
def test_float32_cold_path_decides_the_corpus(oracle, kmax):
    """The cold32 GPU cases cap the replayed tokens at REPLAY_CAP of those sampled, so that they test the decided path: here the
    rule of z_sliced32_kernel on the oracle's own theta, Phi and uniforms leaves at most half the cap undecided (0.2 % at the most,
    K = 176).  A bound on the inputs; the device's count is asserted by the GPU case."""
    c = C.ggs_corpus()
    doc_of = np.repeat(np.arange(c.num_docs), np.diff(c.doc_ptr))
    for K in C.ks_of(kmax):
        undecided = []

        def record(o, phi_before):
            U = oracle.uniforms(C.SEED, o.iteration, oracle.PURPOSE_Z, 0, c.num_tokens)
            decided, _ = kernel_rule(o.get_theta()[doc_of], np.ascontiguousarray(phi_before[:, c.tokens].T), U, K, kmax, False)
            undecided.append(int((~decided).sum()))

        C.oracle_run(oracle, "ggs", c, K, record).close()
        assert len(undecided) == C.SWEEPS
        share = sum(undecided) / (C.SWEEPS * c.num_tokens)
        print("K=%d: %d of %d draws undecided" % (K, sum(undecided), C.SWEEPS * c.num_tokens))
        assert share <= C.REPLAY_CAP / 2, (K, share)
