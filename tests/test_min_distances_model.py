"""The document and topic distances of the diagnostics loop (compute_doc_topic_distances; UPLDA:723-753, 778-806) without a
GPU: the numpy restatement against its scalar twin, the power of the bit-for-bit comparison the GPU tests make
(tests/test_min_distances_gpu.py), the file writers in Python and C++, the block-wise combine of
ShardedGGS.min_doc_distances, and the configuration key."""
import os
import subprocess

import numpy as np
import pytest

from ldagroupedgibbssampler_amd import formats as F
from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import min_distances_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ----------------------------------------------------------------------------------------------------
def test_numpy_form_equals_the_scalar_loops():
    a = R.dirichlet_rows(5, 4, 1)
    b = R.dirichlet_rows(3, 4, 2)
    for got, want in ((R.min_distances(a), R.scalar_min_distances(a)), (R.min_distances(a, b), R.scalar_min_distances(a, b))):
        assert np.array_equal(R.bits(got[0]), R.bits(want[0])) and np.array_equal(R.bits(got[1]), R.bits(want[1]))
    assert R.min_topic_distance(a) == min(R.scalar_min_distances(a)[0])


def test_edges_of_the_reference_loop():
    one = R.dirichlet_rows(1, 7, 3)
    d, sq = R.min_distances(one)
    assert d.tolist() == [1e20] and np.isinf(sq[0])                       # no partner: the initial minimum, not a square root
    assert R.min_topic_distance(one) == 1e20
    a = R.dirichlet_rows(6, 5, 4)
    a[2] = np.nan
    d, sq = R.min_distances(a)
    clean = R.min_distances(np.delete(a, 2, axis=0))[0]
    assert d[2] == 1e20 and np.array_equal(np.delete(d, 2), clean)        # a NaN row reports 1e20 and lowers nobody
    a = R.dirichlet_rows(4, 5, 5)
    a[3] = a[0]
    assert R.min_distances(a)[0][[0, 3]].tolist() == [0.0, 0.0]
    big = np.array([[1e200, 0.0], [0.0, 0.0], [-1e200, 0.0]])              # sums overflow to +inf: sqrt(inf) < 1e20 is false
    d, sq = R.min_distances(big)
    assert d.tolist() == [1e20, 1e20, 1e20] and np.isinf(sq).all()
    far = np.array([[3e20, 0.0], [0.0, 0.0]])                              # a finite sum whose root is not below 1e20
    d, sq = R.min_distances(far)
    assert d.tolist() == [1e20, 1e20] and sq.tolist() == [9e40, 9e40]


def test_blockwise_minimum_is_the_whole_minimum():
    a = R.dirichlet_rows(23, 9, 6)
    whole = R.min_distances(a)[0]
    top, bottom = a[:10], a[10:]
    got = np.concatenate([np.minimum(R.min_distances(top)[0], R.min_distances(top, bottom)[0]),
                          np.minimum(R.min_distances(bottom)[0], R.min_distances(bottom, top)[0])])
    assert np.array_equal(R.bits(got), R.bits(whole))


# ---- the power of the comparison -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [7, 100])
def test_wrong_accumulations_differ_on_the_gpu_cases_inputs(length):
    """A kernel that fused the multiply-add, summed in another order or forgot to skip the diagonal must fail the GPU tests'
    bit-for-bit comparison on the inputs those tests use (dirichlet_rows(65, L, seed=0)).  After sqrt and min an FMA changes
    only a few rows, which is why the GPU tests compare the minimal sums as well and use at least 65 rows."""
    a = R.dirichlet_rows(65, length, 0)
    true = R.pair_sums(a)
    t_dist, t_sq = R.minima(true, skip_diagonal=True)
    # (a) FMA, through exact rationals, on the first 12 rows
    head = a[:12]
    fused, plain = R.fma_pair_sums(head), R.pair_sums(head)
    frac = float((R.bits(fused) != R.bits(plain)).mean())
    print("FMA changes %.0f %% of the pair sums at L = %d" % (100 * frac, length))
    assert frac > 0.1
    f_dist, f_sq = R.minima(fused, skip_diagonal=True)
    p_dist, p_sq = R.minima(plain, skip_diagonal=True)
    print("... and %d of 12 minimal sums, %d of 12 distances" % ((R.bits(f_sq) != R.bits(p_sq)).sum(), (R.bits(f_dist) != R.bits(p_dist)).sum()))
    assert (R.bits(f_sq) != R.bits(p_sq)).any()
    # (b) reversed index order, all 65 rows
    rev = R.pair_sums(a, reverse=True)
    assert float((R.bits(rev) != R.bits(true)).mean()) > 0.1
    assert (R.bits(R.minima(rev, skip_diagonal=True)[1]) != R.bits(t_sq)).any()
    # (c) the diagonal included: every row is nearest to itself
    w_dist, w_sq = R.minima(true, skip_diagonal=False)
    assert (w_dist == 0.0).all() and (t_dist > 0.0).all()


# ---- the writers -----------------------------------------------------------------------------------------------------------
VALUES = [1e20, 0.00012345, 0.0, 0.25, 1.4142135623730951, 5e-324, 12345678.5]
LINE = "7,1.0E20,1.2345E-4,0.0,0.25,1.4142135623730951,4.9E-324,1.23456785E7"


def test_writers_against_hand_written_lines(tmp_path):
    d = str(tmp_path)
    F.append_min_doc_distances(d, 7, VALUES)
    F.append_min_doc_distances(d, 8, np.array([0.5]))
    F.append_min_doc_distances(d, 9, [])
    F.append_min_topic_distance(d, 7, 1e20)
    F.append_min_topic_distance(d, 8, 0.00012345)
    F.append_min_topic_distance(d, 9, 0.0)
    assert open(os.path.join(d, "min_doc_distances.csv"), newline="").read() == LINE + os.linesep + "8,0.5" + os.linesep + "9" + os.linesep
    assert open(os.path.join(d, "min_topic_distances.csv"), newline="").read() == "7,1.0E20%s8,1.2345E-4%s9,0.0%s" % ((os.linesep,) * 3)


def test_cpp_writers_equal_the_python_ones(tmp_path):
    exe = str(tmp_path / "driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "min_distances_formats_driver.cpp"), "-o", exe])
    rng = np.random.default_rng(11)
    rows = [np.array(VALUES), R.min_distances(R.dirichlet_rows(40, 6, 1))[0], 10.0 ** rng.uniform(-8, 8, 30), np.zeros(0)]
    topics = [1e20, 0.0, 3.3e-5, float(rows[1].min())]
    pdir, cdir = tmp_path / "py", tmp_path / "cpp"
    pdir.mkdir()
    cdir.mkdir()
    feed = []
    for it, (r, t) in enumerate(zip(rows, topics), start=3):
        F.append_min_doc_distances(str(pdir), it, r)
        F.append_min_topic_distance(str(pdir), it, t)
        feed.append("D %d %d %s" % (it, r.size, " ".join("%x" % b for b in r.view(np.uint64).tolist())))
        feed.append("T %d %x" % (it, int(np.float64(t).view(np.uint64))))
    subprocess.run([exe, str(cdir)], input="\n".join(feed) + "\n", text=True, check=True)
    for name in ("min_doc_distances.csv", "min_topic_distances.csv"):
        assert open(str(cdir / name), "rb").read() == open(str(pdir / name), "rb").read(), name


# ---- ShardedGGS.min_doc_distances over a numpy engine -------------------------------------------------------------------
class NumpyEngine:
    """The GGSHandle methods ShardedGGS touches, over a fixed theta block."""

    def __init__(self, theta_of_global_doc):
        self._all = theta_of_global_doc

    def set_corpus(self, doc_ptr, tokens, doc_base=0, tok_base=0):
        self.theta = self._all[doc_base:doc_base + len(doc_ptr) - 1]

    def set_global_token_count(self, n):
        pass

    def get_theta(self):
        return self.theta

    def min_doc_distances(self, other=None):
        return R.min_distances(self.theta, other)[0]


def test_sharded_combine_equals_the_whole_corpus():
    from ldagroupedgibbssampler_amd.sharded import NativeExchange, ShardedGGS
    D = 3 * 29 + 1
    theta = R.dirichlet_rows(D, 10, 8)
    sizes = [(57, 570), (1, 10), (30, 300)]                                # uneven, one shard a single document
    bounds = np.concatenate([[0], np.cumsum([d for d, _ in sizes])])
    whole = random_corpus(D, 20, 10, seed=1)
    whole.doc_ptr[:] = np.arange(D + 1) * 10                               # 10 tokens per document, so that sizes is exact
    ranks = []
    for r in range(3):
        sub, _, _ = whole.shard(int(bounds[r]), int(bounds[r + 1]))
        ranks.append(ShardedGGS.from_local_shard(NumpyEngine(theta), NativeExchange, sub, sizes, r, 3))
    gather = lambda a: [s.engine.get_theta() for s in ranks]               # noqa: E731
    got = np.concatenate([s.min_doc_distances(gather=gather) for s in ranks])
    assert np.array_equal(R.bits(got), R.bits(R.min_distances(theta)[0]))
    assert [s.min_doc_distances(gather=gather).size for s in ranks] == [57, 1, 30]


# ---- the configuration key ----------------------------------------------------------------------------------------------------
def test_config_key_default_and_wiring():
    from ldagroupedgibbssampler_amd.sampler import LDAGroupedGibbsSampler, SimpleLDAConfiguration
    assert SimpleLDAConfiguration().compute_doc_topic_distances is False   # COMPUTE_DOC_TOPIC_DISTANCES_DEFAULT
    cfg = SimpleLDAConfiguration(compute_doc_topic_distances=True, start_diagnostic=2)
    assert cfg.compute_doc_topic_distances is True
    m = LDAGroupedGibbsSampler(cfg)
    assert m.minDocDistances == [] and m.minTopicDistances == []
    calls = []
    m.minDocumentDistances = lambda: calls.append("doc") or np.array([0.5, 1e20])
    m.minTopicDistance = lambda: calls.append("topic") or 0.25
    m.computeLogPosterior = lambda: calls.append("posterior") or -1.0
    m._diagnostics(1)
    assert calls == []                                                      # before start_diagnostic
    m._diagnostics(2)
    assert calls == ["doc", "topic", "posterior"]                           # the Java order: theta, distances, log posterior
    assert m.minDocDistances[0].tolist() == [0.5, 1e20] and m.minTopicDistances == [0.25] and m.logPosterior == [-1.0]
    off = LDAGroupedGibbsSampler(SimpleLDAConfiguration(start_diagnostic=1))
    off.minDocumentDistances = lambda: calls.append("never")
    off.computeLogPosterior = lambda: -2.0
    off._diagnostics(1)
    assert "never" not in calls and off.minDocDistances == []


def test_reference_names_the_default():
    import json
    with open(os.path.join(ROOT, "tests", "golden", "reference_signatures.json")) as f:
        assert "COMPUTE_DOC_TOPIC_DISTANCES_DEFAULT" in json.load(f)["LDAConfiguration"]["fields"]
