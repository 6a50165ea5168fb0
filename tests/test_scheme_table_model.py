"""ggs_create's argument check over every combination of the nine scheme flags, against the classes recorded from the library
before the scheme table (tests/golden/scheme_flag_codes.json).  The check is answered before a device is asked for, so it
runs anywhere."""
from tests.scheme_table_cases import SCHEME_BITS, flag_classes, golden, same_class


def test_every_flag_combination_is_classed_as_before(native):
    want, got = golden("scheme_flag_codes.json"), flag_classes(native)
    assert sorted(want) == sorted(got)
    # the golden is what the issue counted on the parent: 16 combinations accepted at K = 5, 6 accepted and 10 unsupported at 4097
    assert [want["5/0"].count(c) for c in ("accepted", "UNSUPPORTED", "BAD_ARG")] == [16, 0, 496]
    assert [want["4097/0"].count(c) for c in ("accepted", "UNSUPPORTED", "BAD_ARG")] == [6, 10, 496]
    wrong = []
    for key in want:
        K = int(key.split("/")[0])
        assert len(want[key]) == len(got[key]) == 1 << len(SCHEME_BITS)
        wrong += ["K/threshold %s flags %#x: %s, was %s" % (key, sum(b for j, b in enumerate(SCHEME_BITS) if i >> j & 1), g, w)
                  for i, (w, g) in enumerate(zip(want[key], got[key])) if not same_class(K, w, g)]
    assert not wrong, "\n".join(wrong[:20])
