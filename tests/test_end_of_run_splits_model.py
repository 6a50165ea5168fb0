"""tests/end_of_run_splits.py without a device: from the constants alone, every case of tests/test_end_of_run_splits_gpu.py
reaches what it claims -- a second piece, group or band, a third trip, a ragged last one -- and the inputs hold the document
and column kinds where a workgroup or a later launch meets them."""
import numpy as np

from tests import end_of_run_splits as S
from tests import topic_diagnostics_restatement as R


def test_the_arithmetic_itself():
    assert S.cut(7, 3) == [3, 3, 1] and S.cut(6, 3) == [3, 3] and S.cut(0, 3) == []
    assert S.knobbed(None, 10) == 10 and S.knobbed(0, 10) == 1 and S.knobbed(-5, 10) == 1 and S.knobbed(11, 10) == 10 and S.knobbed(4, 10) == 4
    assert S.trips(8492, 4096) == (3, 300) and S.trips(4096, 4096) == (1, 4096) and S.trips(4097, 4096) == (2, 1) and S.trips(5, 8) == (1, 5)
    # the built-in sizes: the benchmark-sized shapes the constants were chosen for stay in one piece
    assert S.doc_pieces(10000, 100) == [10000] and S.topic_groups(5000, 100) == [100] and S.dist_bands(10000, 10000, 64) == [157]
    assert S.doc_pieces(1792 + 263, 3072) == [1792, 263]              # test_second_piece_of_documents_at_the_largest_k
    assert S.dist_pieces(200, 7) == [200] and S.dist_pieces(0, 7) == []
    assert S.dist_bands(1 << 22, 1 << 22, 64) == [1 << 14] * 4        # 2^16 tile rows of 2^16 tiles: 2^14 rows per launch


def test_document_pass_trips_and_kinds():
    most, groups = S.trips(S.TRIP_D, S.DOCS_GRID)
    assert S.doc_pieces(S.TRIP_D, S.TRIP_K) == [S.TRIP_D] and most == 3 and groups == 300 < S.DOCS_GRID     # one piece, a ragged third round
    assert -(-S.TRIP_K // 64) == 3 and S.TRIP_K % 64 == 2 and -(-S.TRIP_N // 32) == 4                   # three rounds of topics, four mask words
    doc_ptr, tokens, z, counts, idx = S.trip_corpus()
    lens = np.diff(doc_ptr)
    assert len(lens) == S.TRIP_D and len(set(S.TRIP_ALPHA.tolist())) == S.TRIP_K
    ok = {S.LONG: lambda n: 300 <= n <= 400, S.EMPTY: lambda n: n == 0, S.ONE: lambda n: n == 1, S.SHORT: lambda n: 2 <= n <= 12}
    orders = set()
    for b in range(S.DOCS_GRID):
        if b == S.TRIP_GROUP:
            continue
        kinds = S.trip_kinds(b)
        assert len(kinds) == (3 if b < groups else 2)
        assert len(set(kinds)) == len(kinds)                          # a workgroup's consecutive documents differ in kind
        for trip, kind in enumerate(kinds):
            assert ok[kind](int(lens[b + trip * S.DOCS_GRID])), (b, trip, kind)
        orders.add(tuple(kinds))
    assert {(S.LONG, S.EMPTY, S.ONE), (S.ONE, S.EMPTY, S.LONG)} <= orders
    # a long document: most topics, and under its main topic top words in all four mask words
    where = np.full((S.TRIP_K, S.TRIP_V), -1)
    where[np.arange(S.TRIP_K)[:, None], idx] = np.arange(S.TRIP_N)[None, :]
    for b in (0, 1, 128, 299):
        d = b if b % 2 == 0 else b + 2 * S.DOCS_GRID
        zz, ww = z[doc_ptr[d]:doc_ptr[d + 1]], tokens[doc_ptr[d]:doc_ptr[d + 1]]
        assert len(np.unique(zz)) > S.TRIP_K // 2
        pos = where[b % (S.TRIP_K - 1), ww[zz == b % (S.TRIP_K - 1)]]
        pos = np.unique(pos[pos >= 0])
        assert len(pos) > S.TRIP_N // 3 and set((pos // 32).tolist()) == {0, 1, 2, 3}, (b, pos)


def test_the_hand_built_triple():
    doc_ptr, tokens, z, counts, idx = S.trip_corpus()
    b, k = S.TRIP_GROUP, S.TRIP_TOPIC
    assert k // 64 == 2 and k % 64 == 1                               # lane 1 on its third round
    docs = [(tokens[doc_ptr[d]:doc_ptr[d + 1]], z[doc_ptr[d]:doc_ptr[d + 1]]) for d in (b, b + S.DOCS_GRID, b + 2 * S.DOCS_GRID)]
    top = set(idx[k].tolist())
    assert counts[:, k].sum() == sum(int((zz == k).sum()) for _, zz in docs)            # no other document has the topic
    assert {int(w) for w, t in zip(*docs[0]) if t == k} == top and len(top) == S.TRIP_N   # trip 1: every mask bit
    assert [int(w) for w, t in zip(*docs[1]) if t == k] == [180] and (docs[1][1] != k).sum() >= 3
    assert sorted(int(w) for w, t in zip(*docs[2]) if t == k) == [173, 298]
    want, (p1, p2, p3) = S.triple_codoc(idx)
    assert p1 == 64 and p2 // 32 != p3 // 32                          # the first bit of the third mask word; two words in different ones
    assert want.sum() == S.TRIP_N * S.TRIP_N + 1 + 4 and np.array_equal(want, want.T)
    # and the restatement agrees with the hand count
    sel = np.isin(np.arange(S.TRIP_D), (b, b + S.DOCS_GRID, b + 2 * S.DOCS_GRID))
    lens = np.where(sel, np.diff(doc_ptr), 0)
    keep = np.repeat(sel, np.diff(doc_ptr))
    got = R.doc_statistics(np.concatenate([[0], np.cumsum(lens)]), tokens[keep], z[keep], S.TRIP_V, S.TRIP_K, S.TRIP_ALPHA, S.TRIP_N, idx)[0]
    assert np.array_equal(got[k], want)


def test_document_pieces():
    for K in S.PIECE_KS:
        bytes_ = S.piece_knob(K)
        assert bytes_ < S.TD_PIECE_BYTES and S.knobbed(bytes_, S.TD_PIECE_BYTES) == bytes_
        want = {255: [255], 256: [256], 257: [256, 1], 511: [256, 255], 512: [256, 256], 513: [256, 256, 1], 769: [256, 256, 256, 1]}
        for D in S.PIECE_DS:
            assert S.doc_pieces(D, K, bytes_) == want[D] and S.doc_pieces(D, K) == [D]
            assert S.doc_pieces(D, K, bytes_ - 1) == want[D]          # the 256-document floor
            lens = np.diff(S.piece_case(D, K)[0])
            for d in (255, 256):                                      # empty on both sides of the first boundary
                assert d >= D or lens[d] == 0
            for d in (510, 511, 512, 513):                            # tokens on both sides of the second
                assert d >= D or lens[d] > 0
        assert S.PIECE_DS == sorted(want) and max(len(v) for v in want.values()) == 4


def test_topic_groups():
    all_kinds = {S.DENSE, S.HOLED, S.EMPTY_COL, S.THIRD_DIGIT}
    want = {(300, 1, 3): [1, 1, 1], (300, 2, 5): [2, 2, 1], (257, 64, 63): [63], (257, 64, 64): [64], (257, 64, 65): [64, 1], (257, 64, 129): [64, 64, 1]}
    for V, g, K in S.GROUP_CASES:
        groups = S.topic_groups(V, K, S.group_knob(V, g))
        assert groups == want[(V, g, K)] and S.topic_groups(V, K) == [K]
        counts, where = S.group_counts(V, g, K)
        assert S.columns_differ(counts) and (counts >= 0).all()
        if len(groups) > 1:
            assert all(k >= g for k in where.values())                # every built column in a launch with k0 > 0
            behind = min(K - g, 4)                                    # columns behind the first group
            assert set(where) == [None, {S.HOLED}, {S.DENSE, S.HOLED}, {S.DENSE, S.HOLED, S.EMPTY_COL}, all_kinds][behind]
        else:
            assert set(where) == all_kinds
        for kind, k in where.items():
            col = counts[:, k]
            if kind == S.DENSE:
                assert (col > 0).all()
            if kind == S.HOLED:
                assert (col == 0).sum() == 1
                twin = where.get(S.DENSE, 0)
                assert (counts[:, twin] > 0).all() and (counts[:, twin] != col).sum() == 1
            if kind == S.EMPTY_COL:
                assert not col.any()
            if kind == S.THIRD_DIGIT:
                assert (1 << 16) <= col.max() < (1 << 24) and (col == 0).any()
        if S.THIRD_DIGIT not in where and S.DENSE in where:           # fewer than four columns: the dense one carries the large count
            assert counts[:, where[S.DENSE]].max() >= 1 << 16
    assert {len(want[c]) for c in S.GROUP_CASES} == {1, 2, 3}
    # (257, 64, 129): the four kinds at a group's first and last topic, and in the last group of one topic
    assert sorted(S.group_counts(257, 64, 129)[1].values()) == [64, 65, 127, 128]
    # the built-in group
    assert S.topic_groups(S.BIG_V, S.BIG_K) == [59, 2]
    big = S.big_counts()
    assert (big[:, 0] > 0).all() and (big[:, S.BIG_K - 1] == 0).sum() == 1 and S.BIG_K - 1 >= 59


def test_wtc_and_mirror_trips():
    assert S.trips(S.WTC_V, S.WTC_GRID) == (3, 5)
    for K in S.WTC_KS:
        assert S.topic_groups(S.WTC_V, K) == [K]
    assert S.MIRROR_K * S.MIRROR_N * S.MIRROR_N == 540672 > S.MIRROR_BLOCKS * S.MIRROR_BLOCK == 524288
    assert S.mirror_trips(S.MIRROR_K, S.MIRROR_N) == (2, 540672 - 524288)
    assert S.mirror_trips(32, 128) == (1, 524288)                     # one topic fewer: no second trip


def test_distance_bands():
    def check(n, m, tile, diag):
        tb = -(-m // tile)
        ta = -(-n // tile)
        assert ta >= 3 and S.band_knobs(m, tile) == [1, tb, 2 * tb + 1] and S.dist_bands(n, m, tile) == [ta]
        assert S.dist_bands(n, m, tile, 1) == [1] * ta and S.dist_bands(n, m, tile, tb) == [1] * ta
        assert S.dist_bands(n, m, tile, tb - 1) == [1] * ta          # the max(1, ...) floor
        two = S.dist_bands(n, m, tile, 2 * tb + 1)
        assert two == S.cut(ta, 2) and len(two) >= 2
        for v in S.band_knobs(m, tile):
            if diag:                                                  # the nearest partner of row 5 lies in another band than row 5
                assert S.band_of(n - 1, n, m, tile, v) != S.band_of(S.NEAR, n, m, tile, v)
            assert S.band_of(n - 1, n, m, tile, v) == len(S.dist_bands(n, m, tile, v)) - 1
        if diag:
            for v in (1, tb):                                         # the identical rows in two bands
                assert S.band_of(n - 2, n, m, tile, v) != S.band_of(S.TWIN, n, m, tile, v)
        return two

    assert check(129, 129, S.ROW_TILE, True) == [2, 1] and check(257, 257, S.ROW_TILE, True) == [2, 2, 1]
    assert S.band_of(255, 257, 257, S.ROW_TILE, 11) != S.band_of(S.TWIN, 257, 257, S.ROW_TILE, 11)      # n = 257: identical rows apart also two rows a band
    assert check(*S.BAND_ROW_FOREIGN, S.ROW_TILE, False) == [2, 1]
    assert check(33, 33, S.TOPIC_TILE, True) == [2, 1] and check(49, 49, S.TOPIC_TILE, True) == [2, 2]
    assert S.band_of(47, 49, 49, S.TOPIC_TILE, 9) != S.band_of(S.TWIN, 49, 49, S.TOPIC_TILE, 9)
    for n, length in S.BAND_TOPIC:
        assert length % S.TOPIC_CHUNK == 1 and length > S.TOPIC_CHUNK    # one element behind a chunk end
    a = S.band_rows(129, S.BAND_ROW_LEN, 1)
    assert np.array_equal(a[127], a[S.TWIN]) and S.BAND_ROW_LEN == 33
    from tests import min_distances_restatement as MR
    d5 = MR.pair_sums(a[S.NEAR:S.NEAR + 1], a)[0]
    d5[S.NEAR] = np.inf
    assert int(np.argmin(d5)) == 128
    b = S.foreign_rows(a, 200, 2)
    assert int(np.argmin(MR.pair_sums(a[S.NEAR:S.NEAR + 1], b)[0])) == 199 and np.array_equal(b[0], a[S.TWIN])


def test_foreign_block_pieces():
    K = 7
    assert S.foreign_sizes(1) == [1, 2, 3] and S.foreign_sizes(64) == [63, 64, 65, 129] and S.foreign_sizes(65) == [64, 65, 66, 131]
    seen = set()
    for r in S.FOREIGN_RS:
        for n_other in S.foreign_sizes(r):
            pieces = S.dist_pieces(n_other, K, S.foreign_knob(K, r))
            assert pieces == S.cut(n_other, min(r, n_other)) and S.dist_pieces(n_other, K) == [n_other]
            assert S.dist_pieces(n_other, K, S.foreign_knob(K, r) + 8 * K - 1) == pieces         # bytes that hold no further row
            seen.add(len(pieces))
            row = S.nan_row(n_other, r)
            if n_other == 2 * r + 1:
                assert pieces == [r, r, 1] and r <= row < 2 * r       # a NaN row in the middle piece
            else:
                assert row is None and len(pieces) <= 2
            theta = np.random.default_rng(r).dirichlet(np.full(K, 0.3), 130)
            other = S.foreign_block(theta, n_other, r, 1)
            assert other.shape == (n_other, K) and (row is None) == (not np.isnan(other).any())
    assert seen == {1, 2, 3}
