"""Every KMAX instance of the score-register z kernels against the CPU authority of its scheme, bit for bit.

The kernels for K <= 192 are templates on KMAX = K rounded up to 8 topics; GGS_KMAX_SWITCH and collapsed_kernel_for
(csrc/ggs_host_plan.hpp) instantiate each for KMAX = 8, 16, .., 192: 24 instances of eight kernels, each a fully unrolled function
with its own registers, spills, slice count and LDS layout.  Here each instance runs at two K -- KMAX (a full row) and KMAX - 7
(its smallest K: odd, so Kp = K + 1, seven padding topics, a float32 row that can reach past KMAX) -- in nine legs:

  cold32     z_sliced32_kernel              every chunk cold, the float32 form     OracleSampler
  cold64     z_sliced_kernel                the same, GGS_DEBUG_PHI64=1            OracleSampler
  fused      the cold kernel's hot chunks   GGS_DEBUG_SPLIT=0, a hot table         OracleSampler
  hot        z_hot_kernel                   GGS_DEBUG_SPLIT=2, no pair-chunks      OracleSampler
  pairs      z_pairs_kernel                 GGS_DEBUG_SPLIT=2                      OracleSampler
  warm       z_warm_kernel                  eight tiers of 16 rows                 OracleSampler
  pcgs       pcgs_sliced_kernel<KMAX>       GGS_FLAG_PCGS                          OracleSampler, scheme pcgs
  collapsed  pcgs_sliced_kernel<KMAX, true> GGS_FLAG_COLLAPSED, parallel schedule  collapsed_parallel_sweep
  polyaurn   polyaurn_sliced_kernel<KMAX>   GGS_FLAG_POLYAURN                      tests/polyaurn_restatement.Model

-- GGS_DEBUG_ZKERNEL=1 and GGS_DEBUG_PCGS_WAVE=0 at every K, so that the instances the planner leaves to other kernels by
default (ggs from 161 topics, pcgs from 177, collapsed from 97, polyaurn from 169) run too.  Two sweeps; z, n_wk and phi, and
theta where the scheme has one.  The six ggs legs share one corpus of 1 998 tokens (tests/kmax_instances_cases.ggs_corpus:
documents of 0, 1, 63, 64, 65 and 150 tokens, a Zipf-like head, word V - 1) and one oracle run per K; the lane-per-document
legs one of 70 documents (a full group and a ragged one, three steps and more each).

Every case asserts from launch_info() that it ran what it names: the kernel family and form, the LDS of that instance's layout
(restated in tests/kmax_instances_cases.py; the lane kernels' as in tests/test_scheme_plan_gpu.py), a table of the rows the
planner's arithmetic gives that holds at least 30 % of the tokens.  cold32 also asserts, from GGS_DEBUG_REPLAYS, that at most
3 % of the sampled tokens were replayed: the decided path is what is tested (tests/test_kmax_instances_model.py runs the
decision rule on the oracle's draws: at most 0.2 % undecided in any case, K = 176); cold64 that no float32 launch was made."""
import re

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import kmax_instances_cases as C
from tests import polyaurn_restatement as R
from tests.ranks import assert_bit_equal
from tests.test_phi32_gpu import replays_reported

pytestmark = pytest.mark.gpu

SLICED_NAME = {False: "z_sliced_kernel + z_hot_kernel (score registers)", True: "z_sliced_kernel + z_pairs_kernel (score registers)"}
LANE_NAME = "pcgs_sliced_kernel (lane per document)"

_corpus = {}
_ggs_oracle = {}


def corpus(kind):
    if kind not in _corpus:
        _corpus[kind] = C.ggs_corpus() if kind == "ggs" else C.lane_corpus()
    return _corpus[kind]


def frozen(state):
    for v in state.values():
        v.setflags(write=False)
    return state


def ggs_authority(oracle, K):
    """the oracle's state after SWEEPS sweeps over the shared corpus: once per K for the six ggs legs"""
    if K not in _ggs_oracle:
        o = C.oracle_run(oracle, "ggs", corpus("ggs"), K)
        _ggs_oracle[K] = frozen(dict(z=o.get_z(), n_wk=o.get_type_topic_counts(), phi=o.get_phi(), theta=o.get_theta()))
        o.close()
    return _ggs_oracle[K]


def lane_authority(oracle, leg, K, z0):
    c = corpus("lane")
    if leg == "polyaurn":
        start = java_lcg_initial_z(c.num_tokens, K, C.ZSEED)
        assert_bit_equal(z0, start.astype(np.int32), "the Java-LCG start")
        m = R.Model(K, c.num_types, C.ALPHA, C.BETA, C.SEED, c.doc_ptr, c.tokens, start)
        m.init_phi()
        m.sweep(C.SWEEPS)
        return dict(z=m.z.astype(np.int32), n_wk=m.counts().T.astype(np.int32), phi=m.phi)
    o = C.oracle_run(oracle, leg, c, K)
    s = dict(z=o.get_z(), n_wk=o.get_type_topic_counts())
    if leg == "collapsed":                                           # no Phi is drawn: the point estimate of the counts
        s["phi"] = ((C.BETA + s["n_wk"].astype(np.float64)) / (C.BETA * c.num_types + o.get_topic_totals().astype(np.float64))).T
    else:
        s["phi"] = o.get_phi()
    o.close()
    return s


def check_ggs_launch(leg, kmax, K, c, info):
    """the handle launches the leg's kernel, of this KMAX's layout, over a table that matters"""
    rows = C.hot_rows(leg, K)
    assert info["lds_bytes_z"] == C.sliced_fused_lds(K, rows), (info, rows)
    assert info["z_parts"] == 1
    if leg in ("cold32", "cold64"):
        assert info["z_kernel"] == SLICED_NAME[False] and info["z_form"] == "fused", info     # every chunk a cold one: nothing to split
        assert info["num_hot"] == 0 and info["num_warm"] == 0 and info["warm_tiers"] == 0 and not info["hot_pairs"], info
        assert info["num_chunks"] >= c.num_tokens // 64 >= 2 * C.SLICED_WAVES, info
        return
    if leg == "warm":
        if C.warm_rows(K) == 0:                                      # the planner refuses the tiers at this KMAX (none does: the model file)
            assert info["warm_tiers"] == 0 and info["num_warm"] == 0 and "z_warm_kernel" not in info["z_kernel"], info
            return
        assert info["warm_tiers"] == C.WARM_TIERS and info["num_warm"] == C.WARM_TIERS * C.warm_rows(K) > 0, info
        assert info["z_kernel"].endswith(" + z_warm_kernel (%d tiers)" % C.WARM_TIERS), info
        assert info["warm_docs_per_chunk"] == C.warm_docs_for(kmax), info
        assert info["num_hot"] == rows + info["num_warm"], info        # launch_info counts the table words of both kinds
        assert C.table_share(c, info["num_warm"], skip=rows) >= C.MIN_TABLE_SHARE
        assert C.table_share(c, info["num_warm"]) >= C.MIN_TABLE_SHARE
        return
    assert rows > 0 and info["num_hot"] == rows and info["num_warm"] == 0 and info["warm_tiers"] == 0, (info, rows)
    assert C.table_share(c, info["num_hot"]) >= C.MIN_TABLE_SHARE
    assert info["z_form"] == ("fused" if leg == "fused" else "split"), info
    assert info["hot_pairs"] == (leg == "pairs") and info["z_kernel"] == SLICED_NAME[leg == "pairs"], info
    if leg == "pairs":
        assert info["hot_pair_chunks"] > 0 and 0 < info["hot_pairs_per_token"] <= 1, info
    else:
        assert info["hot_pair_chunks"] == 0, info


def check_lane_launch(K, c, info):
    assert info["z_kernel"] == LANE_NAME and info["z_form"] == "n/a", info
    assert info["lds_bytes_z"] == C.lane_lds(K) and info["num_chunks"] == (c.num_docs + 63) // 64 == 2, info
    assert info["num_hot"] == 0 and info["warm_tiers"] == 0 and info["z_parts"] == 1, info


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_instance_matches_its_authority(native, oracle, monkeypatch, capfd, case):
    leg, kmax, K = case
    assert C.instance_for(K) == kmax == (K + 7) // 8 * 8
    ggs = leg in C.GGS_LEGS
    c = corpus("ggs" if ggs else "lane")
    for k in [k for e in C.ENV.values() for k in e] + ["GGS_DEBUG_NUM_CUS", "GGS_DEBUG_MARGIN"]:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("GGS_DEBUG", "1")
    for k, v in C.ENV[leg].items():
        monkeypatch.setenv(k, v)
    flags = {"pcgs": native.FLAG_PCGS, "collapsed": native.FLAG_COLLAPSED, "polyaurn": native.FLAG_POLYAURN}.get(leg, 0)
    capfd.readouterr()
    g = native.GGSHandle(K, c.num_types, C.ALPHA, C.BETA, C.SEED, flags=flags | native.FLAG_PARANOID)
    try:
        g.set_corpus(c.doc_ptr, c.tokens)
        g.init_z_java_lcg(C.ZSEED)
        z0 = g.get_z()
        g.init_phi()
        g.sweep(C.SWEEPS)
        info = g.launch_info()                                       # after the sweeps: the form the z step took
        got = dict(z=g.get_z(), n_wk=g.get_type_topic_counts(), phi=g.get_phi())
        if ggs:
            got["theta"] = g.get_theta()
        g.check_invariants()
    finally:
        g.close()
    err = capfd.readouterr().err
    if ggs:
        check_ggs_launch(leg, kmax, K, c, info)
        want = ggs_authority(oracle, K)
    else:
        check_lane_launch(K, c, info)
        want = lane_authority(oracle, leg, K, z0)
    assert sorted(got) == sorted(want)
    for k in ("z", "n_wk", "phi", "theta")[:len(got)]:
        assert_bit_equal(got[k], want[k], "%s KMAX=%d K=%d (%s): %s" % (leg, kmax, K, C.KERNEL_OF[leg], k))
    if leg == "cold32":
        n, launches = replays_reported(err)
        sampled = C.SWEEPS * c.num_tokens
        print("K=%d: %d of %d sampled tokens replayed in %d launches" % (K, n, sampled, launches))
        assert "launches of z_sliced32_kernel" in err and launches >= C.SWEEPS >= 2
        assert n <= C.REPLAY_CAP * sampled, (n, sampled)
    elif leg == "cold64":                                            # asked to count them, the float32 form would have reported
        assert not re.search(r"\[ggs\] z replays", err), err[-500:]
