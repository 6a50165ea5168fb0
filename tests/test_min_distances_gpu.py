"""The distance kernels (csrc/ggs_distances.hpp) against the restated reference loops (tests/min_distances_restatement.py),
bit for bit: the distances AND the minimal sums they are the square roots of -- an FMA or another summation order changes a
third of the pair sums but only a few of the minima after sqrt (tests/test_min_distances_model.py measures it).

Shapes: the tile edges are 64 rows (row-major: min_row_dist_kernel) and 16 (element-major: min_topic_dist_kernel), the
k-chunks 32 and 192; every shape list holds the edges -1, +0, +1 and more than one tile."""
import os

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import random_corpus
from tests import min_distances_restatement as R

pytestmark = pytest.mark.gpu

ROW_TILE, ROW_CHUNK, TOPIC_TILE, TOPIC_CHUNK = 64, 32, 16, 192     # kDistRowR * 16, kDistRowKC, kDistTopR * 16, kDistTopKC
SEED, ZSEED = 17, 23
MIN_VALUE = 5e-324                                                  # Double.MIN_VALUE, the clamp of the theta and Phi draws


def check(native, a, b=None, element_major=False, tag=""):
    """the debug entry on rows `a` (always given row-major here; transposed for the element-major kernel) == the restatement"""
    dev_in = np.ascontiguousarray(a.T) if element_major else a
    dist, sq = native.debug_min_distances(dev_in, b, element_major=element_major)
    want_dist, want_sq = R.min_distances(a, b)
    bad = np.flatnonzero(R.bits(sq) != R.bits(want_sq))
    assert bad.size == 0, "%s min_sq differs in %d of %d rows, first %d: %r vs %r" % (tag, bad.size, sq.size, bad[0], sq[bad[0]], want_sq[bad[0]])
    assert np.array_equal(R.bits(dist), R.bits(want_dist)), tag
    return dist, sq


# ---- row-major: the document kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 2, 3, 7, 100])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129, 257])
def test_row_major_shapes(native, n, length):
    check(native, R.dirichlet_rows(n, length, 0), tag="n=%d L=%d" % (n, length))


@pytest.mark.parametrize("length", [1024, 1030, ROW_CHUNK - 1, ROW_CHUNK, ROW_CHUNK + 1])
@pytest.mark.parametrize("n", [65, 129])
def test_row_major_long_rows_and_chunk_edges(native, n, length):
    check(native, R.dirichlet_rows(n, length, 0), tag="n=%d L=%d" % (n, length))


@pytest.mark.parametrize("m", [1, 64, 65, 200])
@pytest.mark.parametrize("n", [1, 65, 129])
def test_against_a_foreign_block(native, n, m):
    a, b = R.dirichlet_rows(n, 33, 1), R.dirichlet_rows(m, 33, 2)
    b[m // 2] = a[n // 2]                                            # no diagonal with a block: an equal row counts, distance 0
    dist, _ = check(native, a, b, tag="n=%d m=%d" % (n, m))
    assert dist[n // 2] == 0.0


# ---- element-major: the topic kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 5, 303, 5000, TOPIC_CHUNK - 1, TOPIC_CHUNK, TOPIC_CHUNK + 1])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 100, TOPIC_TILE - 1, TOPIC_TILE, TOPIC_TILE + 1, 2 * TOPIC_TILE + 1])
def test_element_major_shapes(native, n, length):
    check(native, R.dirichlet_rows(n, length, 0), element_major=True, tag="n=%d L=%d" % (n, length))


# ---- built rows, both layouts ---------------------------------------------------------------------------------------------
LAYOUTS = pytest.mark.parametrize("element_major", [False, True], ids=["row-major", "element-major"])


@LAYOUTS
def test_identical_rows_in_different_tiles(native, element_major):
    a = R.dirichlet_rows(201, 40, 3)
    a[197] = a[2]                                                    # tiles 0 and 3 (rows), 0 and 12 (topics)
    dist, sq = check(native, a, element_major=element_major)
    assert dist[2] == 0.0 and dist[197] == 0.0 and sq[2] == 0.0 and (np.delete(dist, [2, 197]) > 0).all()


@LAYOUTS
def test_all_zero_row(native, element_major):
    a = R.dirichlet_rows(70, 12, 4)
    a[33] = 0.0                                                      # theta when the gammas sum to zero
    check(native, a, element_major=element_major)


@LAYOUTS
def test_min_value_entries_underflow_alike(native, element_major):
    """Rows holding Double.MIN_VALUE entries: their differences are subnormal, the squares underflow to 0 -- nothing may
    flush differently on the device."""
    a = R.dirichlet_rows(70, 12, 5)
    a[a < 0.01] = MIN_VALUE
    a[7] = MIN_VALUE
    a[8] = MIN_VALUE
    a[8, 3] = 0.0
    a[9] = 2 * MIN_VALUE
    dist, sq = check(native, a, element_major=element_major)
    assert sq[7] == 0.0 and sq[8] == 0.0 and sq[9] == 0.0             # subnormal differences, squares that underflow


@LAYOUTS
def test_nan_row_reports_no_partner_and_lowers_nobody(native, element_major):
    a = R.dirichlet_rows(131, 9, 6)
    clean = R.min_distances(np.delete(a, 66, axis=0))[0]
    a[66] = np.nan
    dist, sq = check(native, a, element_major=element_major)
    assert dist[66] == 1e20 and np.isinf(sq[66])
    assert np.array_equal(R.bits(np.delete(dist, 66)), R.bits(clean))


@LAYOUTS
def test_nearest_partner_is_the_last_row_of_the_ragged_tile(native, element_major):
    n = 2 * ROW_TILE + 3                                             # 131: ragged for both tile edges (131 = 8 * 16 + 3)
    a = R.dirichlet_rows(n, 20, 7)
    a[n - 1] = a[5] * (1 - 2.0 ** -30)                               # nearer to row 5 than any random row
    dist, _ = check(native, a, element_major=element_major)
    d5 = R.pair_sums(a[5:6], a)[0]
    d5[5] = np.inf
    assert int(np.argmin(d5)) == n - 1 and dist[5] == np.sqrt(d5[n - 1])


def test_no_partner_at_all(native):
    for em in (False, True):
        dist, sq = native.debug_min_distances(np.array([[0.25, 0.75]]).T if em else np.array([[0.25, 0.75]]), element_major=em)
        assert dist.tolist() == [1e20] and np.isinf(sq[0])


def test_bad_arguments(native):
    L = native._lib.load()
    out = np.zeros(4)
    a = np.zeros((4, 3))
    p = native._dp
    assert L.ggs_debug_min_distances(0, None, 4, None, 0, 3, 0, p(out), None) == native.ERR_BAD_ARG
    assert L.ggs_debug_min_distances(0, p(a), 4, None, 0, 3, 0, None, None) == native.ERR_BAD_ARG
    assert L.ggs_debug_min_distances(0, p(a), -1, None, 0, 3, 0, p(out), None) == native.ERR_BAD_ARG
    assert L.ggs_debug_min_distances(0, p(a), 4, p(a), 4, 3, 1, p(out), None) == native.ERR_BAD_ARG   # element-major takes no block


# ---- handle level ---------------------------------------------------------------------------------------------------------
def synthetic():
    return random_corpus(130, 300, 40, seed=31, empty_every=13)


def flags_of(native, scheme):
    return native.SCHEME_FLAGS["spalias" if scheme == "spalias_priors" else scheme]


def make(native, scheme, corpus, K, sweeps=2):
    h = native.GGSHandle(K, corpus.num_types, 0.1, 0.01, SEED, flags=flags_of(native, scheme))
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    if scheme == "spalias_priors":
        h.set_topic_priors(np.array([0, 1], np.int32), np.array([3, 4], np.int32))
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    h.sweep(sweeps)
    return h


def corpora(cats):
    return [("cats", cats, 3), ("cats", cats, 20), ("synthetic", synthetic(), 7)]


def test_ggs_document_distances_are_those_of_the_last_theta(native, cats):
    for name, corpus, K in corpora(cats):
        h = make(native, "ggs", corpus, K)
        theta = h.get_theta()
        got = h.min_doc_distances()
        assert np.array_equal(R.bits(got), R.bits(R.min_distances(theta)[0])), (name, K)
        assert np.array_equal(R.bits(h.get_theta()), R.bits(theta))          # the call leaves the thetaMatrix alone
        h.close()


@pytest.mark.parametrize("first", ["distances", "posterior"])
def test_pcgs_document_distances_use_the_diagnostic_theta(native, cats, first):
    for name, corpus, K in corpora(cats):
        h = make(native, "pcgs", corpus, K)
        if first == "distances":
            got = h.min_doc_distances()
            theta = h.get_theta()
            h.log_posterior()
            assert np.array_equal(R.bits(h.get_theta()), R.bits(theta)), "the log posterior drew another theta"
        else:
            h.log_posterior()
            theta = h.get_theta()
            got = h.min_doc_distances()
            assert np.array_equal(R.bits(h.get_theta()), R.bits(theta)), "the distances drew another theta"
        assert np.array_equal(R.bits(got), R.bits(R.min_distances(theta)[0])), (name, K)
        h.close()


@pytest.mark.parametrize("scheme", ["ggs", "polyaurn", "spalias_priors"])
def test_topic_distance_is_that_of_phi(native, cats, scheme):
    for name, corpus, K in corpora(cats):
        h = make(native, scheme, corpus, K)
        phi = h.get_phi()
        if scheme != "ggs":
            assert (phi == 0.0).any(), "no exact zero in Phi"
        got = h.min_topic_distance()
        assert np.float64(got).view(np.int64) == np.float64(R.min_topic_distance(phi)).view(np.int64), (name, K, got)
        h.close()


def test_one_topic_and_one_document(native):
    c = random_corpus(1, 30, 25, seed=2)
    h = make(native, "ggs", c, 1)
    assert h.min_topic_distance() == 1e20 and h.min_doc_distances().tolist() == [1e20]
    h.close()


@pytest.mark.parametrize("scheme", ["collapsed", "lightcollapsed", "adlda"])
def test_count_form_schemes_are_unsupported(native, scheme):
    c = synthetic()
    h = native.GGSHandle(5, c.num_types, 0.1, 0.01, SEED, flags=flags_of(native, scheme))
    h.set_corpus(c.doc_ptr, c.tokens)
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    for call in (h.min_doc_distances, h.min_topic_distance):
        with pytest.raises(native.GGSError) as e:
            call()
        assert e.value.code == native.ERR_UNSUPPORTED
    h.close()


def test_state_and_argument_errors(native):
    c = synthetic()
    h = native.GGSHandle(5, c.num_types, 0.1, 0.01, SEED)
    L, p = native._lib.load(), native._dp
    out, v = np.zeros(c.num_docs), np.zeros(1)
    assert L.ggs_min_doc_distances(h._h, None, 0, p(out)) == native.ERR_STATE         # no corpus
    h.set_corpus(c.doc_ptr, c.tokens)
    assert L.ggs_min_doc_distances(h._h, None, 0, p(out)) == native.ERR_STATE         # no Phi
    assert L.ggs_min_topic_distance(h._h, p(v)) == native.ERR_STATE
    h.init_z_java_lcg(ZSEED)
    h.init_phi()
    h.sweep(1)
    assert L.ggs_min_doc_distances(h._h, None, 0, None) == native.ERR_BAD_ARG
    assert L.ggs_min_doc_distances(h._h, p(out), -1, p(out)) == native.ERR_BAD_ARG
    assert L.ggs_min_topic_distance(h._h, None) == native.ERR_BAD_ARG
    assert L.ggs_min_doc_distances(h._h, None, 0, p(out)) == 0
    h.close()


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_diagnostics_leave_the_chain_alone(native, scheme):
    c = synthetic()
    plain, probed = make(native, scheme, c, 7), make(native, scheme, c, 7)
    probed.min_doc_distances()
    probed.min_topic_distance()
    probed.min_doc_distances(R.dirichlet_rows(9, 7, 1))
    for what in ("get_z", "get_type_topic_counts", "get_phi"):
        assert np.array_equal(getattr(plain, what)(), getattr(probed, what)()), what
    plain.sweep(1)
    probed.sweep(1)
    for what in ("get_z", "get_type_topic_counts", "get_phi") + (("get_theta",) if scheme == "ggs" else ()):
        assert np.array_equal(getattr(plain, what)().view(np.int64 if what in ("get_phi", "get_theta") else np.int32),
                              getattr(probed, what)().view(np.int64 if what in ("get_phi", "get_theta") else np.int32)), what
    plain.close()
    probed.close()


class _Lockstep:
    """exchange of ShardedGGS for handles driven in lockstep from one thread: the test sums the count buffers itself"""

    def __init__(self, engine=None):
        pass

    def allreduce_startup(self):
        pass

    allreduce_sweep = allreduce_startup


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_three_handles_equal_one(native, scheme):
    torch = pytest.importorskip("torch")
    from ldagroupedgibbssampler_amd.sharded import ShardedGGS, java_lcg_initial_z, wrap_device_int32
    c = synthetic()
    K = 7
    one = native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=flags_of(native, scheme))
    one.set_corpus(c.doc_ptr, c.tokens)
    z0 = java_lcg_initial_z(c.num_tokens, K, ZSEED)
    one.set_z(z0, redraw_phi=False)
    one.init_phi()
    one.sweep(2)
    want = one.min_doc_distances()
    one.close()

    ranks = [ShardedGGS(native.GGSHandle(K, c.num_types, 0.1, 0.01, SEED, flags=flags_of(native, scheme)), _Lockstep, c, r, 3) for r in range(3)]

    def allreduce():
        counts = [wrap_device_int32(*s.engine.counts_device_ptr()) for s in ranks]
        tot = torch.stack(counts).sum(0, dtype=torch.int32)
        for t in counts:
            t.copy_(tot)
        torch.cuda.synchronize()

    for s in ranks:
        s.engine.set_z(z0[s.tok_base:s.tok_base + s.local.num_tokens], redraw_phi=False)
    allreduce()
    for s in ranks:
        s.engine.init_phi()
    for _ in range(2):
        for s in ranks:
            s.engine.sweep_begin()
        allreduce()
        for s in ranks:
            s.engine.sweep_end()
    for s in ranks:
        s.engine.min_doc_distances()                                  # pcgs: every rank's diagnostic theta exists before the gather
    gather = lambda a: [s.engine.get_theta() for s in ranks]          # noqa: E731
    got = np.concatenate([s.min_doc_distances(gather=gather) for s in ranks])
    assert np.array_equal(R.bits(got), R.bits(want))
    topic = {s.engine.min_topic_distance() for s in ranks}
    assert len(topic) == 1                                            # Phi is replicated
    for s in ranks:
        s.engine.close()


@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_sample_writes_both_files(native, cats, scheme, tmp_path):
    from ldagroupedgibbssampler_amd import formats as F
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    cfg = SimpleLDAConfiguration(scheme=scheme, topics=5, alpha=0.1, beta=0.01, seed=SEED, exec_time=None, iterations=4,
                                 compute_doc_topic_distances=True, start_diagnostic=2, log_dir=str(tmp_path))
    m = create_model(cfg)
    m.setRandomSeed(SEED)
    m.addInstances(cats)
    m.sample(4)
    assert len(m.minDocDistances) == 3 and len(m.minTopicDistances) == 3 and len(m.logPosterior) == 3
    assert np.array_equal(R.bits(m.minDocDistances[-1]), R.bits(m.minDocumentDistances()))     # the getters, same state
    assert m.minTopicDistances[-1] == m.minTopicDistance()
    doc_lines = open(os.path.join(str(tmp_path), "min_doc_distances.csv")).read().splitlines()
    topic_lines = open(os.path.join(str(tmp_path), "min_topic_distances.csv")).read().splitlines()
    assert len(doc_lines) == 3 and len(topic_lines) == 3
    for i, it in enumerate((2, 3, 4)):
        assert doc_lines[i] == ",".join([str(it)] + [F.java_double_to_string(v) for v in m.minDocDistances[i]])
        assert topic_lines[i] == "%d,%s" % (it, F.java_double_to_string(m.minTopicDistances[i]))
    assert len(doc_lines[0].split(",")) == cats.num_docs + 1


def test_diagnostics_off_by_default(native, cats, tmp_path):
    from ldagroupedgibbssampler_amd.sampler import SimpleLDAConfiguration, create_model
    cfg = SimpleLDAConfiguration(topics=5, seed=SEED, exec_time=None, iterations=2, start_diagnostic=1, log_dir=str(tmp_path))
    m = create_model(cfg)
    m.setRandomSeed(SEED)
    m.addInstances(cats)
    m.sample(2)
    assert m.minDocDistances == [] and not os.path.exists(os.path.join(str(tmp_path), "min_doc_distances.csv"))
