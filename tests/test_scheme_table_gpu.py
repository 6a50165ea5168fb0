"""What each of the ten schemes' handles answers to the getters that only some schemes have, and the kernel number it
reports, against the answers recorded on the device from the library before the scheme table
(tests/golden/scheme_capabilities.json)."""
import pytest

from tests.scheme_table_cases import capabilities, golden

pytestmark = pytest.mark.gpu


def test_every_scheme_answers_every_capability_call_as_before(native):
    want, got = golden("scheme_capabilities.json"), capabilities(native)
    assert len(want) == 10
    assert got == want, "\n".join("%s %s: %s, was %s" % (s, k, got.get(s, {}).get(k), v) for s in want for k, v in want[s].items() if got.get(s, {}).get(k) != v)
