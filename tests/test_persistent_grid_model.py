"""tests/persistent_grid.py without a device: the corpora hold the kinds of documents the GPU cases rely on, in the order a
one-CU grid hands them out, and the trip arithmetic of the rows holds for the caps it names."""
import numpy as np

from tests import persistent_grid as PG
from tests import test_persistent_grid_gpu as T


def test_a_workgroup_meets_long_short_one_token_and_empty_documents():
    for kind, per_item, cap in (("wave", 1, PG.CAP_WAVE), ("lane", 64, PG.CAP_LANE)):
        c = T.corpus_of(kind, 210 if kind == "wave" else 500)
        lens = np.sort(np.diff(c.doc_ptr))[::-1]                    # the device's order: longest first
        items = -(-lens.size // per_item)
        PG.assert_trips(items, 1, cap, kind)
        first = lens[::per_item][:items]                            # the longest document of every item
        mine = first[0::cap]                                        # the items of workgroup 0 on one CU
        assert mine[0] > 128 and mine[-1] == 0 and (mine == 1).any() and ((mine > 1) & (mine <= 64)).any(), mine
        assert (np.diff(mine) <= 0).all()


def test_trip_arithmetic():
    assert PG.min_trips(96, 1, 32) == 3 and PG.min_trips(95, 1, 32) == 3 and PG.min_trips(64, 1, 32) == 2
    assert PG.min_trips(200, 2, 32) == 4 and PG.min_trips(27, 1, 8) == 4 and PG.min_trips(210, 1, 8, waves=4) == 7
    assert PG.alias_words_per_block(1024) == 4 and PG.alias_words_per_block(100) == 40 and PG.alias_words_per_block(8) == 64
    assert PG.alias_items(210, 1024) == 53
    # the Poisson tiles: ceil(1024 / K) rows at least, about eight per CU otherwise
    assert PG.poisson_tiles(210, 8, 1) == 2 and PG.poisson_tiles(800, 8, 1) == 7 and PG.poisson_tiles(500, 20, 1) == 8
    assert PG.poisson_tiles(210, 200, 1) == 8 and PG.poisson_tiles(900, 100, 1) == 8 and PG.poisson_tiles(210, 160, 1) == 8
    for r in T.ROWS:
        if "poisson" in r.phases:
            PG.assert_trips(PG.poisson_tiles(r.V, r.K, 1), 1, PG.CAP_POISSON, r.id)
        if "wordlist" in r.phases:
            PG.assert_trips(r.V, 1, PG.CAP_WORDLIST, r.id, waves=PG.WORDLIST_WAVES)
        if "alias" in r.phases:
            PG.assert_trips(PG.alias_items(r.V, r.K), 1, PG.CAP_ALIAS, r.id)
        if "vsbits" in r.phases:
            PG.assert_trips(PG.vs_bits_items(r.V, r.K), 1, PG.CAP_VSBITS, r.id)
            assert PG.vs_bits_items(r.V, r.K) % PG.CAP_VSBITS != 0    # a ragged last trip
        if "wordmask" in r.phases:
            PG.assert_trips(r.V, 1, PG.CAP_WORDMASK, r.id, waves=PG.WORDLIST_WAVES)
            assert -(-r.V // PG.WORDLIST_WAVES) % PG.CAP_WORDMASK != 0
    assert PG.vs_bits_items(1030, 130) == 99 and PG.vs_bits_items(210, 8) == 7 and PG.min_trips(99, 1, PG.CAP_VSBITS) == 4
    assert sum("vsbits" in r.phases and "wordmask" in r.phases for r in T.ROWS) == 1
