"""The knife-edge rows of scheme=lightpcldaw2 (tests/lightpcldaw2_knife_edge.py) on the CPU: every row exists and reaches the
comparison it aims at -- the builder asserts that while it builds, from the restatement -- and the rows have the power they
claim: the rewrite an order row names decides its comparison the other way, and so does one double more or less."""
import functools

import numpy as np

from tests import lightpcldaw2_knife_edge as KE
from tests import lightpcldaw2_restatement as R


@functools.lru_cache(maxsize=None)
def rows():
    return {r.name: r for r in KE.build()}


def test_every_row_is_built(oracle):
    got = rows()
    assert tuple(got) == KE.NAMES                                   # no row is left out
    for r in got.values():
        assert r.want_stats.sum() == KE.TOKENS.size and r.want_z.shape == KE.Z.shape
        assert (R.count(KE.TOKENS, r.z, KE.V, KE.K)[0][0] == [0, 2, 0, 0, 2, 0, 2, 0]).all()     # the word's row the rows are planned on
        print("%-22s seed %4d beta %-22r %s" % (r.name, r.seed, r.beta, r.note))


def target_ratio_inputs(r, which):
    n, G, bh = KE.quantities(r.alpha, r.beta)
    phi_w = r.phi[:, 0]
    if which == "w":
        t, s = r.det["word"], 1
        return (float(phi_w[t]), float(phi_w[s]), r.alpha, n[t], n[s] - 1, r.beta, G[s], G[t], bh[t], bh[s])
    t, s = r.det["doc"], 1
    return (float(phi_w[t]), float(phi_w[s]), r.alpha, n[t], n[s] - 1, n[t], n[s])


def test_order_rows_separate_the_rewrites(oracle):
    for v in KE.ORDERS_W:
        r = rows()["order_w:" + v]
        q, u = target_ratio_inputs(r, "w"), KE.uniforms(r.seed)[1]
        ours, other = R.word_ratio(*q), KE.pi_w_as(v, *q)
        assert ours == r.det["pi_w"] and other != ours
        assert R.accepts(ours, u) == r.det["acc_w"] and R.accepts(other, u) != r.det["acc_w"], (v, ours, other, u)
    for v in KE.ORDERS_D:
        r = rows()["order_d:" + v]
        q, u = target_ratio_inputs(r, "d"), KE.uniforms(r.seed)[3]
        ours, other = R.doc_ratio(*q), KE.pi_d_as(v, *q)
        assert ours == r.det["pi_d"] and other != ours and "pi_w" not in r.det
        assert R.accepts(ours, u) == r.det["acc_d"] and R.accepts(other, u) != r.det["acc_d"], (v, ours, other, u)
    for r in rows().values():                                       # a flipped comparison is a different new topic for the target
        if r.name.startswith("order_w") or r.name.startswith("edge_w"):
            f = KE.flips(r.seed, r.alpha, r.beta, r.phi, "w")
            assert f[0] != f[1] and r.want_z[0] == f[0 if r.det["acc_w"] else 1]
        if r.name.startswith("order_d"):
            f = KE.flips(r.seed, r.alpha, r.beta, r.phi, "d")
            assert f[0] != f[1] and r.want_z[0] == f[0 if r.det["acc_d"] else 1]


def test_value_rows_stand_on_their_doubles(oracle):
    got = rows()
    assert got["one_w"].det["pi_w"] == 1.0 and got["one_w"].det["acc_w"]          # `> 1` is false; U2 < 1.0 accepts
    for tag, k in zip(KE.TAGS, (-1, 0, 1)):
        r = got["edge_w:" + tag]
        u = KE.uniforms(r.seed)[1]
        assert r.det["pi_w"] == KE.moved(u, k) and r.det["acc_w"] == (k == 1)
        r = got["branch:" + tag]
        u_w = KE.uniforms(r.seed)[0] * (6.0 + r.beta * float(KE.K))
        assert u_w == KE.moved(6.0, k) and r.det["branch"] == (R.TABLE if k < 0 else R.BETA)
    r = got["last_entry"]
    u_w = KE.uniforms(r.seed)[0] * (6.0 + r.beta * float(KE.K))
    assert u_w < 6.0 and int((u_w / 6.0) * 3.0) == 2 and r.det["word"] == KE.LIST_W[-1] and r.det["branch"] == R.TABLE
    assert got["beta_last"].det["word"] == KE.K - 1 and got["beta_last"].det["branch"] == R.BETA
    assert got["inf_w"].det["pi_w"] == np.inf and got["inf_w"].det["acc_w"] and got["inf_w"].phi[1, 0] == 0.0
    assert np.isnan(got["nan_w"].det["pi_w"]) and not got["nan_w"].det["acc_w"]
    r = got["back_to_z0"]
    assert r.det["acc_w"] and r.det["doc"] == r.det["s"] == r.det["word"] != 1 and r.det["new"] == 1 and r.want_z[0] == 1 and r.det["idx"] > 0
