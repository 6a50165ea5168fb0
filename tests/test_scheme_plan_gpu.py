"""A handle plans, allocates and reports the z step of ITS scheme: for all six schemes, at a K the lane-per-document and
score-register kernels take (8) and one they do not (200), launch_info() names the kernel the handle launches and gives
that launch's dynamic LDS and work items -- for the pcgs family written out here from the layout functions beside the
kernels (ggs_z_pcgs.hpp, ggs_z_pcgs_wave.hpp, ggs_z_spalias.hpp, ggs_z_lightpc.hpp) -- before a corpus, with one, and
with a second one on the same handle; the sweeps run with GGS_FLAG_PARANOID.  The bits of the results are pinned by the
parity, posterior and knife-edge files; the bits of a REUSED handle -- a second and a third corpus against a fresh handle and
the oracle, for every scheme -- by tests/test_handle_lifecycle_gpu.py."""
import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus

pytestmark = pytest.mark.gpu

SEED, ALPHA, BETA, V = 4242, 0.1, 0.01, 40
SCHEMES = ("ggs", "pcgs", "collapsed", "polyaurn", "spalias", "lightpclda")
LANE, WAVE = "pcgs_sliced_kernel (lane per document)", "pcgs_wave_kernel (wave per document)"
KERNEL = {   # (scheme, K) -> what launch_info()["z_kernel"] starts with
    ("ggs", 8): "z_sliced_kernel + z_hot_kernel (score registers)", ("ggs", 200): "z_stream1_kernel (one pass)",
    ("pcgs", 8): LANE, ("collapsed", 8): LANE, ("polyaurn", 8): LANE,
    ("pcgs", 200): WAVE, ("collapsed", 200): WAVE, ("polyaurn", 200): WAVE,       # beyond 176 / 96 / 168 topics: a wave per document
    ("spalias", 8): "spalias_wave_kernel (wave per document)", ("spalias", 200): "spalias_wave_kernel (wave per document)",
    ("lightpclda", 8): "lightpc_wave_kernel (wave per document)", ("lightpclda", 200): "lightpc_wave_kernel (wave per document)",
}


def corpus(lens, seed):
    rng = np.random.default_rng(seed)
    doc_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return Corpus(doc_ptr, rng.integers(0, V, int(doc_ptr[-1])).astype(np.int32), V)


def ragged(D, seed):
    """D documents of 0 .. 30 tokens: every length occurs, so there are empty documents and one of 30."""
    return corpus(np.random.default_rng(seed).permutation(np.arange(D) % 31), seed)


def lane_lds(K):                       # pcgs_sliced_lds_bytes: alpha row + int16 counts [KMAX][64] in whole 256 bytes, a ring of three 8 KiB slices
    kmax = (K + 7) // 8 * 8
    return (kmax * 8 + kmax * 128 + 255) // 256 * 256 + 3 * 8192


def wave_lds(K):                       # pcgs_wave_lds_bytes: blocks of 128 topics, a power of two of them; int32 counts and the alpha row
    nb = 1
    while nb * 128 < K + (K & 1):
        nb *= 2
    return nb * 128 * 4 + nb * 128 * 8


def spalias_lds(K, cap):               # spalias_lds_bytes: [cap] doubles, [K] int32, [K] int16, [cap rounded up to 4] int16
    return cap * 8 + K * 4 + K * 2 + ((cap + 3) & ~3) * 2


def expected(scheme, K, c, kernel):
    """lds_bytes_z and num_chunks of a pcgs-family handle over corpus c (None: before a corpus)."""
    longest = 0 if c is None else int(np.diff(c.doc_ptr).max())
    D = 0 if c is None else c.num_docs             # the document order: one entry per document (fewer groups of 64 than resident waves)
    if scheme == "lightpclda":
        return 4 * K, D
    if scheme == "spalias":
        return (0 if c is None else spalias_lds(K, max(1, min(K, longest)))), D
    if kernel == WAVE:
        return wave_lds(K), D
    return lane_lds(K), (D + 63) // 64


def make(native, scheme, K):
    flags = {"ggs": 0, "pcgs": native.FLAG_PCGS, "collapsed": native.FLAG_COLLAPSED, "polyaurn": native.FLAG_POLYAURN, "spalias": native.FLAG_SPALIAS,
             "lightpclda": native.FLAG_LIGHTPCLDA}[scheme]
    return native.GGSHandle(K, V, ALPHA, BETA, SEED, flags=flags | native.FLAG_PARANOID)


def run_and_check(g, scheme, K, c, kernel):
    g.set_corpus(c.doc_ptr, c.tokens)
    g.init_z_java_lcg(SEED)
    z0 = g.get_z()
    g.init_phi()
    g.sweep(2)
    g.check_invariants()
    z = g.get_z()
    assert z.shape == (c.num_tokens,) and int(g.get_topic_totals().sum()) == c.num_tokens
    assert (z != z0).mean() > 0.25, "the z step ran"        # two sweeps redraw every token: at K = 8 one in eight keeps its topic by chance
    info = g.launch_info()
    assert info["z_kernel"].startswith(kernel)
    if scheme != "ggs":
        assert (info["lds_bytes_z"], info["num_chunks"]) == expected(scheme, K, c, kernel)
        assert info["num_hot"] == 0 and info["warm_tiers"] == 0 and info["z_parts"] == 1 and info["z_form"] == "n/a"
    return info


@pytest.mark.parametrize("K", [8, 200])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_launch_info_is_the_scheme_s_own(native, scheme, K):
    kernel = KERNEL[scheme, K]
    a, b = ragged(130, seed=1), ragged(77, seed=2)         # three groups of 64 documents, the last one ragged; then two
    assert a.num_docs == 130 and (np.diff(a.doc_ptr) == 0).any() and np.diff(a.doc_ptr).max() == 30 and a.num_tokens != b.num_tokens
    g = make(native, scheme, K)
    try:
        before = g.launch_info()
        if scheme != "ggs":
            assert (before["lds_bytes_z"], before["num_chunks"]) == expected(scheme, K, None, kernel)
            assert before["num_hot"] == 0 and before["warm_tiers"] == 0 and before["z_parts"] == 1 and before["z_form"] == "n/a"
        first = run_and_check(g, scheme, K, a, kernel)
        second = run_and_check(g, scheme, K, b, kernel)     # a second corpus on the same handle
        if scheme != "ggs":                                 # the diagnostic theta draw's: not the corpus' choice
            assert first["docs_per_block_theta"] == second["docs_per_block_theta"] == before["docs_per_block_theta"] > 0
    finally:
        g.close()


def test_a_long_document_switches_pcgs_to_the_wave_kernel(native):
    K = 8
    g = make(native, "pcgs", K)
    try:
        run_and_check(g, "pcgs", K, ragged(130, seed=1), LANE)
        long_doc = corpus(np.array([5, 33000, 0, 12]), seed=3)          # more tokens than the lane kernels' int16 counts hold
        info = run_and_check(g, "pcgs", K, long_doc, WAVE)
        assert (info["lds_bytes_z"], info["num_chunks"]) == (1536, 4)
        run_and_check(g, "pcgs", K, ragged(77, seed=2), LANE)           # and back
    finally:
        g.close()
