"""The arms of the cold chunk loop (cold_chunk_loop, ggs_z_sliced.hpp) at their smallest, for both forms of the kernel.

One workgroup of four waves (GGS_DEBUG_NUM_CUS=1: the stride is 4) and every chunk a cold one (GGS_DEBUG_HOT=0,
GGS_DEBUG_WARM=0), so launch_info()["num_chunks"] is the cold chunk count C and wave w takes chunks w, w + 4, ...:

  C   3        4          5        8          9        12         13
      0 or 1   exactly 1  1 or 2   exactly 2  2 or 3   exactly 3  3 or 4   chunks per wave

-- each value of has1 and has2 in the prologue, in the steady state and at the last chunk, and (C = 3) a wave that leaves
at once.  K = 8, 24, 40, 72 give the float32 form (GGS_DEBUG_PHI64=0) 1, 1, 2, 3 slices per chunk and the fp64 form
(GGS_DEBUG_PHI64=1) 1, 2, 3, 5: with the ring's two slots, both forms meet "the only slice in flight is the next
chunk's", "as many slices as slots" and "more slices than slots".  Two corpora per C over V = 50 words: documents of
exactly 64 tokens (every chunk full, one document per chunk) and a ragged one (documents of 0, 1, a few and about 100
tokens: chunks that span a document boundary, idle lanes); the document counts were found with the CPU list builder
(tests/corpus_lists_driver.cpp, hot_cap = 0, sliced_waves = 4) and every case asserts the count it got.  At most 832
tokens per case, two sweeps, z, n_wk, phi and theta bit for bit against the oracle.

The float32 rows must test the decided path, not the exact replay behind it: they run with GGS_DEBUG_REPLAYS=1 and assert
that at most 2 % of the sampled tokens were replayed.  The margin of ggs_z_sliced.hpp leaves about 2 K (2K + 8) 2^-24 of
the tokens undecided, below 0.2 % at K = 72; for these corpora and seeds the numpy model of tests/test_margin32_model.py
(kernel_rule on the oracle's theta, Phi and uniforms of both sweeps) was run on the CPU: at most 1 token undecided in any
case, so every case stays well under the cap."""
import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus
from tests.test_phi32_gpu import compare_state, make_pair, replays_reported

pytestmark = pytest.mark.gpu

V, SWEEPS = 50, 2
COUNTS = (3, 4, 5, 8, 9, 12, 13)
PATTERN = (0, 1, 5, 100, 3, 0, 97, 1, 7, 103, 2)                        # the ragged corpus' document lengths, repeated
RAGGED = {3: (0, 4), 4: (2, 6), 5: (0, 7), 8: (0, 13), 9: (2, 13), 12: (0, 18), 13: (0, 20)}   # C -> (first length, documents)


def corpus_of(lengths, seed):
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    return Corpus(ptr, np.random.default_rng(seed).integers(0, V, int(ptr[-1])).astype(np.int32), V)


def make_corpus(kind, C):
    if kind == "full":
        return corpus_of([64] * C, 100 + C)
    rot, n = RAGGED[C]
    return corpus_of([PATTERN[(i + rot) % len(PATTERN)] for i in range(n)], 200 + C)


@pytest.mark.parametrize("phi64", ["0", "1"], ids=["float32", "fp64"])
@pytest.mark.parametrize("K", [8, 24, 40, 72])
@pytest.mark.parametrize("kind", ["full", "ragged"])
@pytest.mark.parametrize("C", COUNTS)
def test_cold_chunk_loop_arms(native, oracle, monkeypatch, capfd, C, kind, K, phi64):
    for k, v in {"GGS_DEBUG": "1", "GGS_DEBUG_NUM_CUS": "1", "GGS_DEBUG_ZKERNEL": "1", "GGS_DEBUG_HOT": "0", "GGS_DEBUG_WARM": "0",
                 "GGS_DEBUG_PHI64": phi64, "GGS_DEBUG_REPLAYS": "1"}.items():
        monkeypatch.setenv(k, v)
    c = make_corpus(kind, C)
    assert c.num_tokens <= 13 * 64
    g, o = make_pair(native, oracle, c, K, 40 + K, K + C)
    try:
        info = g.launch_info()
        assert info["num_chunks"] == C and info["num_hot"] == 0 and info["z_kernel"].startswith("z_sliced_kernel"), info
        g.sweep(SWEEPS)
        o.sweep(SWEEPS)
        compare_state(g, o, "cold chunk loop C=%d %s K=%d phi64=%s" % (C, kind, K, phi64))
    finally:
        g.close()
        o.close()
    if phi64 == "0":
        n, launches = replays_reported(capfd.readouterr().err)
        print("C=%d %s K=%d: %d of %d sampled tokens replayed in %d launches" % (C, kind, K, n, SWEEPS * c.num_tokens, launches))
        assert launches >= SWEEPS
        assert n <= 0.02 * SWEEPS * c.num_tokens, (n, c.num_tokens)
