"""tests/stream_address.py without a device: the oracle's draws and its z step against the rule stated directly from
include/ggs_hip.h, every restatement model against its own step under that statement, and the sensitivity of the corner cases
-- each mutant address moves z and the theta rows at the corner, and the two that lose the element's high word move nothing
before the crossing and something from it on.  Without the last a corner that tests nothing could pass unnoticed."""
import importlib

import numpy as np
import pytest

from tests import handle_lifecycle as H
from tests import stream_address as S

ALPHA = H.ALPHA


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def corner(K):
    c = H.corpus("A")
    doc = S.pick_doc(c)
    return (c, doc) + S.bases(c, K, doc)


def test_rule_is_the_header_s():
    assert S.key(S.SEED) == (0xB5A69788, 0xF1E2D3C4)
    assert S.counter(S.PURPOSE_THETA, S.IT0, (7 << 32) | 9, 3) == (9, 7, (2 << 24) | 3, 0x7F3A91C3)
    assert S.double_of(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and S.double_of(0, 0) == 0.0 and S.double_of(1 << 6, 0) == 2.0 ** -26
    for name, m in S.MUTANTS.items():                                    # each mutant gets one word of (counter, key) wrong (the swap: both key words)
        elem, base = S.TWO32 + 11, S.TWO32 - 50
        (c, k), (tc, tk) = m(S.SEED, S.IT0, S.PURPOSE_THETA, elem, 1, base), S.true_address(S.SEED, S.IT0, S.PURPOSE_THETA, elem, 1, base)
        wrong = [i for i in range(4) if c[i] != tc[i]] + [4 + i for i in range(2) if k[i] != tk[i]]
        expect = {"seed_hi_dropped": [5], "seed_lo_only_shifted": [4, 5], "elem_hi_dropped": [1], "elem_hi_from_base": [1], "iteration_low16": [3],
                  "block_in_purpose_byte": [2]}[name]
        assert wrong == expect, (name, wrong)
        below = S.TWO32 - 7                                              # the element mutants are the truth below 2^32
        assert (m(S.SEED, S.IT0, 1, below, 0, base) == S.true_address(S.SEED, S.IT0, 1, below, 0, base)) == (name in S.ELEM_MUTANTS), name


def test_corner_helper_accepts_every_corpus_and_K_the_device_tests_use():
    from tests import test_stream_address_gpu as G
    seen = 0
    for c, K, doc, offset in G.corner_cases():
        doc_base, tok_base = S.bases(c, K, doc, offset)
        cross = S.crossing_token(c, doc, offset)
        assert tok_base + cross == S.TWO32 and c.doc_ptr[doc] < cross < c.doc_ptr[doc + 1] - 1
        seen += 1
    assert seen >= 2 + len(G.FORMS)
    with pytest.raises(AssertionError):
        S.bases(H.corpus("A"), 8, S.pick_doc(H.corpus("A")))            # 2^32 mod 8 == 0: the crossing would be a row's edge
    with pytest.raises(AssertionError):
        S.bases(H.corpus("A"), 20, S.pick_doc(H.corpus("A")), offset=25)  # no document of corpus A has more than 50 tokens


@pytest.mark.parametrize("purpose", S.PURPOSES)
def test_oracle_draws_equal_the_direct_statement(oracle, purpose):
    elem0, n = S.TWO32 - 100, 200
    want = S.first_uniforms(S.SEED, S.IT0, purpose, elem0, n)
    assert np.array_equal(bits(oracle.uniforms(S.SEED, S.IT0, purpose, elem0, n)), bits(want))
    assert len(set(want.tolist())) == n
    # gaussians: the polar pair is the element's draws 0 and 1; where it is accepted at once the first value is v1 * multiplier
    g = oracle.gaussians(S.SEED, S.IT0, purpose, elem0, n)
    settled = 0
    for i in range(n):
        a, b = S.uniform_pair(S.SEED, S.IT0, purpose, elem0 + i, 0)
        v1, v2 = 2 * a - 1, 2 * b - 1
        s = v1 * v1 + v2 * v2
        if 0 < s < 1:
            assert bits([g[i]])[0] == bits([v1 * float(np.sqrt(-2 * float(oracle.log([s])[0]) / s))])[0], i
            settled += 1
    assert settled > n // 2
    # gammas: shapes on both sides of 1; the first-try subset is predicted by uniform_pair alone
    shape = np.where(np.arange(n) % 2 == 0, 0.1, 3.1) + (np.arange(n) % 5)
    gam = oracle.gammas(S.SEED, S.IT0, purpose, elem0, shape)
    first = [S.gamma_first_try(S.SEED, S.IT0, purpose, elem0 + i, float(shape[i])) for i in range(n)]
    idx = [i for i in range(n) if first[i] is not None]
    assert len(idx) > n // 2 and min(idx) < 100 <= max(idx) and any(shape[i] < 1 for i in idx) and any(shape[i] > 1 for i in idx)
    assert np.array_equal(bits(gam[idx]), bits([first[i] for i in idx])), purpose
    # the Dirichlet draw: the same gammas at the same elements, normalised (ParallelDirichlet.java:46-70)
    p = shape
    mag = float(np.cumsum(p)[-1])
    a = p / mag * mag
    ga = oracle.gammas(S.SEED, S.IT0, purpose, elem0, a)
    assert np.array_equal(bits(oracle.dirichlet(S.SEED, S.IT0, purpose, elem0, p)), bits(ga / float(np.cumsum(ga)[-1])))


def oracle_before_step(oracle, scheme, K):
    c, doc, doc_base, tok_base = corner(K)
    o = oracle.OracleSampler(K, H.V, ALPHA, 0.05, S.SEED, threads=4)
    o.set_scheme(scheme)
    o.set_corpus(c.doc_ptr, c.tokens, doc_base, tok_base)
    o.set_iteration(S.IT0)
    o.set_z(H.initial_z(c, K), redraw_phi=False)
    o.init_phi()
    return o, c, doc, doc_base, tok_base


@pytest.fixture(scope="module")
def stepped():
    """per (scheme, K): the oracle's z before and after one z step given Phi at the corner, its Phi and theta -- computed once"""
    from oracle import oracle as O
    out = {}
    for scheme in ("ggs", "pcgs"):
        for K in S.KS:
            o, c, doc, doc_base, tok_base = oracle_before_step(O, scheme, K)
            z0 = o.get_z()
            o.set_iteration(S.IT0 + 1)
            o.z_step()
            out[scheme, K] = dict(c=c, doc=doc, doc_base=doc_base, tok_base=tok_base, z0=z0, z1=o.get_z(), phi=o.get_phi(),
                                  theta=o.get_theta() if scheme == "ggs" else None, n_dk0=H_doc_counts(c, z0, K))
            o.close()
    return out


def H_doc_counts(c, z, K):
    n = np.zeros((c.num_docs, K), np.int64)
    np.add.at(n, (np.repeat(np.arange(c.num_docs), np.diff(c.doc_ptr)), np.asarray(z, np.int64)), 1)
    return n


def direct(s, scheme, address=S.true_address):
    return S.z_step_direct(scheme, s["c"], s["z0"], s["phi"], S.SEED, S.IT0 + 1, s["tok_base"], theta=s["theta"], alpha=ALPHA, address=address)


@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("scheme", ["ggs", "pcgs"])
def test_oracle_z_step_equals_a_direct_walk(stepped, scheme, K):
    s = stepped[scheme, K]
    z = direct(s, scheme)
    bad = z != s["z1"]
    assert not bad.any(), "%s K=%d: %d tokens differ; before / at / after the crossing: %s" % (
        scheme, K, bad.sum(), S.split_at_crossing(bad, S.crossing_token(s["c"], s["doc"])))
    assert (s["z1"] != s["z0"]).mean() > 0.5


@pytest.mark.parametrize("K", S.KS)
def test_oracle_theta_rows_equal_the_direct_statement(oracle, stepped, K):
    """GGS:57-72 at the corner: element (doc_base + d) * K + k, shape n_dk + alpha; the first-try gammas of rows doc - 1 ... doc + 1,
    normalised by the oracle's own row sum, are the oracle's theta cells -- and the row sum is recovered from any settled cell."""
    s = stepped["ggs", K]
    doc, settled = s["doc"], 0
    for d in (doc - 1, doc, doc + 1):
        p = s["n_dk0"][d].astype(np.float64) + ALPHA
        mag = float(np.cumsum(p)[-1])
        shapes = p / mag * mag                                           # Dirichlet(p): partition * magnitude (ParallelDirichlet.java:46-70)
        gam = oracle.gammas(S.SEED, S.IT0 + 1, S.PURPOSE_THETA, (s["doc_base"] + d) * K, shapes)
        total = float(np.cumsum(gam)[-1])
        assert np.array_equal(bits(gam / total), bits(s["theta"][d])), d
        for k in range(K):
            g = S.gamma_first_try(S.SEED, S.IT0 + 1, S.PURPOSE_THETA, (s["doc_base"] + d) * K + k, float(shapes[k]))
            if g is not None:
                assert bits([g])[0] == bits([gam[k]])[0], (d, k)
                settled += 1
    assert settled > K


@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("name", [r.name for r in H.ROWS if r.oracle != "c"])
def test_restatement_models_equal_their_own_step_under_the_direct_statement(monkeypatch, oracle, name, K):
    """The models take their z uniforms from O.uniforms (or, the two LightLDA ones, from Philox blocks addressed in their own
    words).  One step of each at the corner, once as it is and once with O.uniforms replaced by the direct statement: the same z;
    and not the z of tok_base = 0, so the constructor's tok_base reaches the step."""
    row = H.ROW[name]
    c, doc, doc_base, tok_base = corner(K)
    step = (("zgiven", 1),) if row.z_given_phi else (("sweep", 1),)
    z0 = H.initial_z(c, K)

    def chain(tb):
        return H.Chain(row, K, c, z0, S.IT0, seed=S.SEED, doc_base=doc_base, tok_base=tb)

    plain = chain(tok_base).run(step)
    patched = chain(tok_base)
    calls = []

    def direct_uniforms(seed, it, purpose, elem0, n):
        calls.append((purpose, elem0, n))
        return S.first_uniforms(seed, it, purpose, elem0, n)

    mod = importlib.import_module("tests." + row.oracle)
    if name in ("lightpclda", "lightcollapsed"):
        for gtok in (S.TWO32 - 1, S.TWO32, S.TWO32 + 1):
            want = S.uniform_pair(S.SEED, S.IT0 + 1, S.PURPOSE_Z, gtok, 0) + S.uniform_pair(S.SEED, S.IT0 + 1, S.PURPOSE_Z, gtok, 1)
            assert mod.token_uniforms(S.SEED, S.IT0 + 1, gtok) == want
    else:
        with monkeypatch.context() as m:
            m.setattr(oracle, "uniforms", direct_uniforms)
            patched.run(step)                                                # adlda: the sweep is its z step, no Phi draw behind it
        assert (S.PURPOSE_Z, tok_base, c.num_tokens) in calls, calls[:4]
        assert np.array_equal(plain.state()["z"], patched.state()["z"]), name
    assert plain.iteration == S.IT0 + 1
    at_zero = chain(0).run(step)
    bad = plain.state()["z"] != at_zero.state()["z"]
    assert bad.mean() > 0.1, "%s: tok_base does not reach the z step (%d tokens differ)" % (name, bad.sum())


@pytest.mark.parametrize("K", S.KS)
@pytest.mark.parametrize("mutant", list(S.MUTANTS))
def test_every_mutant_address_moves_z_and_theta_at_the_corner(stepped, mutant, K):
    address = S.MUTANTS[mutant]
    for scheme in ("ggs", "pcgs"):
        s = stepped[scheme, K]
        cross = S.crossing_token(s["c"], s["doc"])
        bad = direct(s, scheme, address) != s["z1"]
        before, at, after = S.split_at_crossing(bad, cross)
        n_after = bad.size - cross
        print("%s %s K=%d: z differs in %d tokens before the crossing, %d of %d from it on (%.0f %%)" % (
            mutant, scheme, K, before, at + after, n_after, 100.0 * (at + after) / n_after))
        assert at + after > 0.3 * n_after, (mutant, scheme, K)
        if mutant in S.ELEM_MUTANTS:
            assert before == 0
        else:
            assert before > 0.3 * cross
    # the theta rows around row doc: the first-try gammas, cell by cell
    s = stepped["ggs", K]
    doc, base = s["doc"], s["doc_base"] * K
    kx = S.TWO32 % K
    moved = {"before": [0, 0], "after": [0, 0]}
    for d in (doc - 1, doc, doc + 1):
        shapes = s["n_dk0"][d].astype(np.float64) + ALPHA
        for k in range(K):
            elem = (s["doc_base"] + d) * K + k
            t = S.gamma_first_try(S.SEED, S.IT0 + 1, S.PURPOSE_THETA, elem, float(shapes[k]), base=base)
            m = S.gamma_first_try(S.SEED, S.IT0 + 1, S.PURPOSE_THETA, elem, float(shapes[k]), address, base)
            side = moved["before" if elem < S.TWO32 else "after"]
            side[0] += (t is None) != (m is None) or (t is not None and bits([t])[0] != bits([m])[0])
            side[1] += 1
    assert moved["before"][1] == K + kx and moved["after"][1] == 2 * K - kx
    print("%s K=%d: theta cells moved: %d of %d before the crossing, %d of %d from it on" % (mutant, K, *moved["before"], *moved["after"]))
    assert moved["after"][0] > 0.5 * moved["after"][1]
    if mutant in S.ELEM_MUTANTS:
        assert moved["before"][0] == 0
    else:
        assert moved["before"][0] > 0.5 * moved["before"][1]
