"""Knife-edge rows for the token step of scheme=lightpcldaw2 (a test helper, not collected; in the manner of
tests/lightpclda_knife_edge.py and tests/lightcollapsed_knife_edge.py, with simpler means: the scheme has a Phi that
ggs_set_phi sets cell by cell, so most comparisons are aimed through one cell of Phi instead of through alpha).

A row is a whole tiny model of its own -- K = 8 topics, V = 3 words, two documents, one handle -- whose TARGET is token 0:
document 0, position 0, word 0.  Its uniforms are those of (seed, iteration 1, token 0), so the seed is searched until the
proposals fall where the row wants them; the document's histogram and the word's count row come from the z that ggs_set_z
sets (document 1 is ballast: more tokens of word 0 on chosen topics); then ONE cell of Phi (or, for the branch of the word
proposal, beta -- fixed at ggs_create, so every value is a handle) is moved ulp by ulp until the comparison stands where the
row aims.  The z step is ggs_sample_z_given_phi(1).

The comparisons (LightPCLDAtypeTopicProposal.java:148-225, tests/lightpcldaw2_restatement.token_step):
  order_w:<v>   U2 < pi_w, where the left-to-right pi_w and the rewrite <v> decide differently.  Rewrites: "rtl" (each product
                right to left), "pairs" ((p * x) * (y * z)), "mid_left" ((p * (x * y)) * z), "mid_right" (p * ((x * y) * z))
                -- with left to right the five ways to bracket four factors -- "bhat_across" (bhat[s] divides the
                numerator, bhat[t] the denominator), "bg_across" ((beta + G) likewise)
  order_d:<v>   U4 < pi_d likewise: "rtl" (the other way to bracket three factors), "quotients" (the product of three quotients)
  one_w         pi_w == 1.0 exactly: `pi_w > 1` is false, U2 < 1 accepts
  edge_w:<tag>  pi_w == the double below U2, U2 itself, the double above: only the last accepts
  branch:<tag>  u_w == the double below tokensPerType[w] (the table), tokensPerType[w] itself and the double above (the beta
                branch), through beta
  last_entry    u_w / tokensPerType[w] so close to 1 that the cell is nnz_w - 1: the last list entry, not an invalid topic
  beta_last     a beta-branch topic of K - 1
  inf_w, nan_w  phi[s][w] == 0 with a non-zero numerator (+inf: accepted whatever U2 is) and with phi[t][w] == 0 too (NaN:
                accepts nothing)
  back_to_z0    the word proposal is accepted and the document proposal, read from the array, equals it: the token returns to z0

build() asserts from the restatement that every row reaches the comparison it aims at, with the values it aims at, and
raises if one cannot be built: no row is left out."""
import struct
from collections import namedtuple

import numpy as np

from tests import lightpcldaw2_restatement as R

K, V = 8, 3
ITERATION = 1
SCAN = 400                                                          # ulps of the aimed cell to either side of the solution
MAX_SEEDS = 4000
ORDERS_W = ("rtl", "pairs", "mid_left", "mid_right", "bhat_across", "bg_across")
ORDERS_D = ("rtl", "quotients")
TAGS = ("below", "tie", "above")
NAMES = tuple(["order_w:" + v for v in ORDERS_W] + ["order_d:" + v for v in ORDERS_D] + ["one_w"] + ["edge_w:" + t for t in TAGS] +
              ["branch:" + t for t in TAGS] + ["last_entry", "beta_last", "inf_w", "nan_w", "back_to_z0"])

# document 0: the target (word 0, topic 1) and four tokens of word 1; document 1: five more tokens of word 0.  Word 0's row is
# 2, 2, 2 on topics 1, 4, 6 (tokensPerType 6, three equal table entries: ps = 1.0, a = i), every one of those topics holds 3
# tokens in all and the document without the target holds one token of each: pi_w is symmetric in them.
DOC_PTR = np.array([0, 5, 10], np.int64)
TOKENS = np.array([0, 1, 1, 1, 1, 0, 0, 0, 0, 0], np.int32)
Z = np.array([1, 1, 4, 6, 2, 1, 4, 4, 6, 6], np.int32)
LIST_W = [1, 4, 6]

Row = namedtuple("Row", "name seed alpha beta phi z want_z want_stats det note")


def _bits(x):
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _dbl(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def moved(x, k):
    """x moved by k doubles (x > 0)"""
    return _dbl(_bits(x) + k)


def scan(x):
    """x, then its neighbours outwards"""
    yield x
    for k in range(1, SCAN + 1):
        yield moved(x, k)
        yield moved(x, -k)


def uniforms(seed):
    return R.token_uniforms(seed, ITERATION, 0)


def base_phi(seed):
    """positive, no special values: every product of the ratios rounds"""
    return 0.05 + 0.9 * np.random.default_rng(seed).random((K, V))


def run(seed, alpha, beta, phi, z=Z):
    """the restatement's z step of the row: (z after it, the three counters, the target's detail)"""
    n_wk, n_k = R.count(TOKENS, z, V, K)
    out = np.array(z, np.int64)
    dets = {}
    stats = R.z_step(DOC_PTR, TOKENS, out, phi, n_wk, n_k, alpha, beta, R.build_tables(n_wk, n_k, beta), seed, ITERATION,
                     on_token=lambda d, pos, det: dets.setdefault((d, pos), det))
    return out.astype(np.int32), np.array(stats, np.int64), dets[(0, 0)]


def quantities(alpha, beta, z=Z):
    """what the target's two ratios read besides Phi: the document's histogram with the token, the word's row, bhat"""
    n_wk, n_k = R.count(TOKENS, z, V, K)
    n = np.bincount(z[:5], minlength=K).tolist()
    return n, [int(x) for x in n_wk[0]], R.bhat(n_k, beta * float(V))


def pi_w_as(order, phi_t, phi_s, a, ni_t, ni_s, beta, G_s, G_t, bh_t, bh_s):
    """pi_w under a rewrite of the kernel's arithmetic (plain Python floats: IEEE doubles)"""
    x, y, bs, bt = a + float(ni_t), a + float(ni_s), beta + float(G_s), beta + float(G_t)
    with np.errstate(all="ignore"):
        if order == "rtl":
            return float(np.float64(phi_t * (x * (bs * bh_t))) / np.float64(phi_s * (y * (bt * bh_s))))
        if order == "pairs":
            return float(np.float64((phi_t * x) * (bs * bh_t)) / np.float64((phi_s * y) * (bt * bh_s)))
        if order == "mid_left":
            return float(np.float64((phi_t * (x * bs)) * bh_t) / np.float64((phi_s * (y * bt)) * bh_s))
        if order == "mid_right":
            return float(np.float64(phi_t * ((x * bs) * bh_t)) / np.float64(phi_s * ((y * bt) * bh_s)))
        if order == "bhat_across":
            return float(np.float64(phi_t * x * bs / bh_s) / np.float64(phi_s * y * bt / bh_t))
        if order == "bg_across":
            return float(np.float64(phi_t * x / bt * bh_t) / np.float64(phi_s * y / bs * bh_s))
    raise KeyError(order)


def pi_d_as(order, phi_t, phi_s, a, ni_t, ni_s, n_t, n_s):
    x, y, u, v = a + float(ni_t), a + float(ni_s), a + float(n_s), a + float(n_t)
    if order == "rtl":
        return (phi_t * (x * u)) / (phi_s * (y * v))
    if order == "quotients":
        return (phi_t / phi_s) * (x / y) * (u / v)
    raise KeyError(order)


def finish(name, seed, alpha, beta, phi, note, z=Z):
    want_z, stats, det = run(seed, alpha, beta, phi, z)
    return Row(name, seed, alpha, beta, phi, np.array(z, np.int32), want_z, stats, det, note)


def _seeds(start):
    return range(start, start + MAX_SEEDS)


def flips(seed, alpha, beta, phi, which):
    """the target's new topic with the comparison `which` ("w": U2 < pi_w, "d": U4 < pi_d) forced to accept and to reject, on a
    ratio below 1: a row is useful only if the two differ"""
    out = []
    for u in (0.0, 1.0 - 2.0 ** -53):
        U = list(uniforms(seed))
        U[1 if which == "w" else 3] = u
        n, G, bh = quantities(alpha, beta)
        zdoc = [int(k) for k in Z[:5]]
        n_wk, n_k = R.count(TOKENS, Z, V, K)
        ps, a, _, nw, lists, tpt = R.build_tables(n_wk, n_k, beta)
        al = np.full(K, alpha)
        R.token_step(n, zdoc, 0, phi[:, 0].tolist(), G, bh, al, R.alpha_sum(al, K), beta, (ps[0], a[0], lists[0], int(nw[0]), int(tpt[0])), tuple(U))
        out.append(zdoc[0])
    return out


def word_row(name, alpha, beta, accept, start=1):
    """accept(pi_w, U2, q) -> note or None decides whether a value of phi[t][0] makes the row; q = the ratio's other inputs"""
    for seed in _seeds(start):
        U = uniforms(seed)
        phi = base_phi(seed)
        _, _, det = run(seed, alpha, beta, phi)
        t, s = det["word"], 1
        if t == s or det["branch"] != R.TABLE or not 0.2 < U[1] < 0.8:
            continue
        n, G, bh = quantities(alpha, beta)
        q = (float(phi[s, 0]), alpha, n[t], n[s] - 1, beta, G[s], G[t], bh[t], bh[s])
        den = q[0] * (alpha + float(q[3])) * (beta + float(G[t])) * bh[s]
        guess = U[1] * den / ((alpha + float(n[t])) * (beta + float(G[s])) * bh[t])
        for x in scan(guess):
            note = accept(R.word_ratio(x, *q), U[1], (x,) + q)
            if note is None:
                continue
            phi[t, 0] = x
            f = flips(seed, alpha, beta, phi, "w")
            if f[0] == f[1]:
                break                                               # accepting or not gives the same topic here: another seed
            row = finish(name, seed, alpha, beta, phi, note)
            assert row.det["word"] == t and row.det["pi_w"] == R.word_ratio(x, *q)
            return row
    raise AssertionError("no row %s in %d seeds" % (name, MAX_SEEDS))


def doc_row(name, alpha, beta, accept, start=1):
    """the same through phi[dt][0], on tokens whose word proposal is their own topic (no word step)"""
    for seed in _seeds(start):
        U = uniforms(seed)
        phi = base_phi(seed)
        _, _, det = run(seed, alpha, beta, phi)
        t, s = det["doc"], 1
        if det["word"] != s or t == s or not 0.2 < U[3] < 0.8:
            continue
        n, _, _ = quantities(alpha, beta)
        q = (float(phi[s, 0]), alpha, n[t], n[s] - 1, n[t], n[s])
        guess = U[3] * (q[0] * (alpha + float(n[s] - 1)) * (alpha + float(n[t]))) / ((alpha + float(n[t])) * (alpha + float(n[s])))
        for x in scan(guess):
            note = accept(R.doc_ratio(x, *q), U[3], (x,) + q)
            if note is None:
                continue
            phi[t, 0] = x
            f = flips(seed, alpha, beta, phi, "d")
            if f[0] == f[1]:
                break
            row = finish(name, seed, alpha, beta, phi, note)
            assert row.det["doc"] == t and row.det["pi_d"] == R.doc_ratio(x, *q) and "pi_w" not in row.det
            return row
    raise AssertionError("no row %s in %d seeds" % (name, MAX_SEEDS))


def branch_row(tag, alpha=0.1):
    """u_w = U1 * (6 + beta * 8) on the double below 6, on 6 and on the double above, through beta"""
    want = {"below": moved(6.0, -1), "tie": 6.0, "above": moved(6.0, 1)}[tag]
    for seed in _seeds(1):
        U1 = uniforms(seed)[0]
        if not 0.5 < U1 < 0.95:
            continue
        guess = (6.0 / U1 - 6.0) / float(K)
        for beta in scan(guess):
            if U1 * (6.0 + beta * float(K)) != want:
                continue
            row = finish("branch:" + tag, seed, alpha, beta, base_phi(seed), "u_w = %r against tokensPerType 6" % want)
            assert row.det["branch"] == (R.TABLE if tag == "below" else R.BETA)
            assert row.det["word"] == (LIST_W[-1] if tag == "below" else 0)     # cell nnz - 1 of three equal entries; beta cell 0
            return row
    raise AssertionError("no row branch:%s" % tag)


def search_row(name, alpha, beta, make_phi, ok, note, z=Z):
    for seed in _seeds(1):
        phi = make_phi(seed)
        with np.errstate(all="ignore"):
            row = finish(name, seed, alpha, beta, phi, note, z)
        if ok(row.det, row):
            return row
    raise AssertionError("no row %s in %d seeds" % (name, MAX_SEEDS))


def build():
    """every row of NAMES, in that order"""
    rows = []
    a, b = 0.1, 0.01

    def differs(order, pi_as):
        def accept(pi, u, q):
            other = pi_as(order, *q)
            if other != pi and R.accepts(pi, u) != R.accepts(other, u):
                return "left to right %r, %s %r, U %r" % (pi, order, other, u)
            return None
        return accept

    for v in ORDERS_W:
        rows.append(word_row("order_w:" + v, a, b, differs(v, pi_w_as)))
    for v in ORDERS_D:
        rows.append(doc_row("order_d:" + v, a, b, differs(v, pi_d_as)))

    # pi_w == 1.0: equal Phi cells on the word's three topics, everything else symmetric by construction
    def sym_phi(seed):
        phi = base_phi(seed)
        phi[LIST_W, 0] = phi[1, 0]
        return phi
    rows.append(search_row("one_w", a, b, sym_phi, lambda det, row: det.get("pi_w") == 1.0 and det["acc_w"] and det["word"] != 1, "pi_w == 1.0"))

    for tag, k in zip(TAGS, (-1, 0, 1)):
        rows.append(word_row("edge_w:" + tag, a, b, lambda pi, u, q, k=k: ("pi_w %r, U2 %r" % (pi, u)) if pi == moved(u, k) else None, start=50))
        assert rows[-1].det["acc_w"] == (tag == "above")
    for tag in TAGS:
        rows.append(branch_row(tag))
    last = branch_row("below")
    rows.append(last._replace(name="last_entry", note="(u_w / 6) * 3 = %r: cell 2" % ((moved(6.0, -1) / 6.0) * 3.0)))
    assert int((moved(6.0, -1) / 6.0) * 3.0) == 2 and last.det["word"] == LIST_W[-1]

    rows.append(search_row("beta_last", a, 0.5, base_phi, lambda det, row: det["branch"] == R.BETA and det["word"] == K - 1, "beta-branch topic K - 1"))

    def zero_s(both):
        def make(seed):
            phi = base_phi(seed)
            phi[1, 0] = 0.0
            if both:
                phi[:, 0] = 0.0
            return phi
        return make
    rows.append(search_row("inf_w", a, b, zero_s(False), lambda det, row: det.get("pi_w") == np.inf and det["acc_w"] and uniforms(row.seed)[1] > 0.9,
                           "phi[s][w] == 0, numerator > 0: +inf, accepted at U2 > 0.9"))
    rows.append(search_row("nan_w", a, b, zero_s(True), lambda det, row: "pi_w" in det and np.isnan(det["pi_w"]) and not det["acc_w"] and uniforms(row.seed)[1] < 0.1,
                           "phi[s][w] == phi[t][w] == 0: NaN, refused at U2 < 0.1"))

    def eager(seed):
        phi = base_phi(seed)
        phi[1, 0] = 1e-3                                            # every word proposal away from topic 1 is accepted
        return phi
    rows.append(search_row("back_to_z0", a, b, eager, lambda det, row: det["acc_w"] and det["idx"] not in (None, 0) and det["doc"] == det["word"] and det["new"] == 1
                           and row.want_z[0] == 1, "accepted word proposal, document proposal equal to it: back on z0"))
    assert tuple(r.name for r in rows) == NAMES
    return rows
