"""The knife-edge rows of scheme=lightpcldaw2 (tests/lightpcldaw2_knife_edge.py) on the device: each row is a handle of its
own -- ggs_set_z, ggs_set_phi, one ggs_sample_z_given_phi -- whose z and Metropolis-Hastings counters must be the
restatement's, bit for bit.  What the rows aim at and that they reach it: tests/test_lightpcldaw2_knife_edge_model.py."""
import functools

import pytest

from tests import lightpcldaw2_knife_edge as KE
from tests.ranks import assert_bit_equal, z_kernel

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def rows():
    return {r.name: r for r in KE.build()}


@pytest.mark.parametrize("name", KE.NAMES)
def test_row(native, oracle, name):
    r = rows()[name]
    g = native.GGSHandle(KE.K, KE.V, r.alpha, r.beta, r.seed, flags=native.FLAG_LIGHTPCLDAW2)
    g.set_corpus(KE.DOC_PTR, KE.TOKENS)
    g.set_z(r.z, redraw_phi=False)
    g.set_phi(r.phi)
    g.sample_z_given_phi(1)
    assert z_kernel(g).startswith("lightpcw2_wave_kernel")
    assert_bit_equal(g.get_z(), r.want_z, "z of row %s (%s)" % (name, r.note))
    assert_bit_equal(g.mh_stats(), r.want_stats, "MH counters of row %s" % name)
    g.close()
