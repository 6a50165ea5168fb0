"""scheme=lightpcldaw2 without a device: the public surface (class, flag, header, Java constant, refused combinations,
create_model's refusal, no scratch), the restatement (tests/lightpcldaw2_restatement.py) against a line-by-line transcription
of LightPCLDAtypeTopicProposal.java:101-274 on explicit arrays, the target the word step leaves invariant, and the distance
of the restatement's chain from the enumerated posterior of tests/lda_posterior.py.

The chain is approximate as the reference writes it: the last test prints chi-square and total variation
against the enumerated posterior and asserts no p-value."""
import os
import re

import numpy as np
import pytest

from tests import lda_posterior as LP
from tests import lightpcldaw2_restatement as R
from tests import spalias_restatement as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the public surface (the first test: it fails on a build without the scheme) --------------------------------------
def test_class_flag_header_and_java_constant_agree():
    from ldagroupedgibbssampler_amd import _lib, native, sampler
    m = sampler.LightPCLDAtypeTopicProposal(sampler.SimpleLDAConfiguration(topics=4, seed=1))
    assert isinstance(m, sampler.LDAPartiallyCollapsedGibbsSampler)
    assert sampler.LightPCLDAtypeTopicProposal._scheme_flags == native.FLAG_LIGHTPCLDAW2 == 2048
    for name in ("getAliasTables", "getWordTopicLists", "getMHStats", "sampleZGivenPhi", "getPhi", "computeLogPosterior"):
        assert callable(getattr(m, name))
    with pytest.raises(NotImplementedError):
        m.getTheta()
    for fn in ("ggs_get_mh_stats", "ggs_get_alias_tables", "ggs_get_word_topic_lists", "ggs_sample_z_given_phi", "ggs_get_theta"):
        assert fn in _lib.SIGNATURES
    header = open(_lib.HEADER_PATH).read()
    bits = {name: int(bit) for name, bit in re.findall(r"\bGGS_FLAG_(\w+)\s*=\s*1\s*<<\s*(\d+)", header)}
    assert bits["LIGHTPCLDAW2"] == 11 and bits["LIGHTPCLDAW2"] == max(bits.values())      # the next free bit
    assert sorted(bits.values()) == list(range(12))                 # and no bit twice
    assert "#define GGS_ABI_VERSION 6" in header                    # a new bit, not a new ABI version
    java = open(os.path.join(ROOT, "integration", "java", "cc", "mallet", "topics", "GGSNative.java")).read()
    assert "FLAG_LIGHTPCLDAW2 = 2048" in java
    assert native.Z_KERNEL_NAMES[12] == "lightpcw2_wave_kernel (wave per document)"
    api = open(os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc", "ggs_host_state.hpp")).read()
    assert re.search(r'\{"lightpcldaw2", GGS_FLAG_LIGHTPCLDAW2, [^}]*?, 12, &LaunchPlan::lightpcw2,', api)   # its row of the scheme table


def test_create_model_still_refuses_the_name():
    from ldagroupedgibbssampler_amd import sampler
    with pytest.raises(ValueError, match="not provided by this build"):
        sampler.create_model(sampler.SimpleLDAConfiguration(topics=4, seed=1), "lightpcldaw2")


def test_flag_combinations_are_refused():
    """GGS_FLAG_LIGHTPCLDAW2 with any other scheme's flag but GGS_FLAG_PCGS is GGS_ERR_BAD_ARG: an argument check, answered
    before ggs_create asks for a device -- so it can be seen here.  Alone and beside GGS_FLAG_PCGS it passes the check (what
    comes then is GGS_OK, or GGS_ERR_HIP where no device is)."""
    from ldagroupedgibbssampler_amd import native
    for other in (native.FLAG_COLLAPSED, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA, native.FLAG_POLYAURN_SPARSE,
                  native.FLAG_LIGHTCOLLAPSED, native.FLAG_NZVSSPALIAS, native.FLAG_ADLDA, native.FLAG_LIGHTPCLDA | native.FLAG_PCGS):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_LIGHTPCLDAW2 | other)
        assert e.value.code == native.ERR_BAD_ARG, other
    for flags in (native.FLAG_LIGHTPCLDAW2, native.FLAG_LIGHTPCLDAW2 | native.FLAG_PCGS, native.FLAG_LIGHTPCLDAW2 | native.FLAG_SAVE_PHI_MEAN):
        try:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=flags).close()
        except native.GGSError as e:
            assert e.code == native.ERR_HIP, (flags, e)
    with pytest.raises(native.GGSError) as e:                       # a wave-per-document kernel: 4096 topics at most
        native.GGSHandle(4097, 10, 0.1, 0.01, 1, flags=native.FLAG_LIGHTPCLDAW2)
    assert e.value.code == native.ERR_UNSUPPORTED


def test_the_kernel_uses_no_scratch():
    path = os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc", "ggs_resource_summary.txt")
    if not os.path.exists(path):
        from ldagroupedgibbssampler_amd import _lib
        _lib.build()
    rows = {}
    for line in open(path):
        if line.startswith("#"):
            continue
        f = line.split()
        rows[" ".join(f[:-6])] = [int(x) for x in f[-6:]]
    for k in ("ggs::lightpcw2_wave_kernel", "ggs::count_alias_build_kernel"):
        assert k in rows, "%s is not in the build" % k
        assert rows[k][3] == 0, "%s spills %d bytes per lane" % (k, rows[k][3])


# ---- the token step against the Java text -----------------------------------------------------------------------------
def java_token(phi, typeTopicCounts, topicCountBetaHat, tokensPerType, nonZeroTypeTopics, aliasTables, localTopicCounts, localTopicCounts_not_i,
               oneDocTopics, position, type_, alpha, alphaSum, beta, numTopics, U):
    """LightPCLDAtypeTopicProposal.java:128-241 for one position, line by line.  phi [K][V], typeTopicCounts [V][K],
    aliasTables[type] = (ps, a) of the DECLARED builder (TypeTopicParallelTableBuilder); U the four uniforms in the order the
    Java code asks ThreadLocalRandom for them when every branch runs.  decrement / increment (:136, :227) only queue updates
    for updateCounts: nothing they touch is read before the sweep ends."""
    out = {}
    oldTopic = oneDocTopics[position]                               # :129
    newTopic = oldTopic                                             # :130
    localTopicCounts_not_i[oldTopic] -= 1                           # :146
    u_w = U[0] * (tokensPerType[type_] + beta * numTopics)          # :148
    if u_w < tokensPerType[type_]:                                  # :151-153
        u = u_w / float(tokensPerType[type_])
        ps, a = aliasTables[type_]
        k = len(ps)
        ups = u * k                                                 # generateSample, OptimizedGentleAliasMethodDynamicSize.java:112-119
        i = int(ups)
        if (ups - i) > ps[i]:
            i = int(a[i])
        wordTopicIndicatorProposal = nonZeroTypeTopics[type_][i]
    else:                                                           # :155
        wordTopicIndicatorProposal = int(((u_w - tokensPerType[type_]) / (beta * numTopics)) * numTopics)
    out["word"] = wordTopicIndicatorProposal
    if wordTopicIndicatorProposal != oldTopic:                      # :163
        al = alpha[oldTopic]                                        # :166
        n_d_zi_not_i = float(localTopicCounts_not_i[oldTopic])      # :263-268
        n_d_zstar_not_i = float(localTopicCounts_not_i[wordTopicIndicatorProposal])
        n_zstar_beta_hat = topicCountBetaHat[wordTopicIndicatorProposal]
        n_zi_beta_hat = topicCountBetaHat[oldTopic]
        n_w_zi = float(typeTopicCounts[type_][oldTopic])
        n_w_zstar = float(typeTopicCounts[type_][wordTopicIndicatorProposal])
        nom = phi[wordTopicIndicatorProposal][type_] * (al + n_d_zstar_not_i) * (beta + n_w_zi) * n_zstar_beta_hat      # :270
        denom = phi[oldTopic][type_] * (al + n_d_zi_not_i) * (beta + n_w_zstar) * n_zi_beta_hat                          # :271
        with np.errstate(invalid="ignore", divide="ignore"):
            pi_w = float(np.float64(nom) / np.float64(denom))       # :272
        out["pi_w"] = pi_w
        if pi_w > 1 or U[1] < pi_w:                                 # :168-185
            localTopicCounts[oldTopic] -= 1
            localTopicCounts[wordTopicIndicatorProposal] += 1
            oldTopic = wordTopicIndicatorProposal
    u_i = U[2] * (len(oneDocTopics) + alphaSum)                     # :193-200
    if u_i < len(oneDocTopics):
        docTopicIndicatorProposal = oneDocTopics[int(u_i)]
    else:
        docTopicIndicatorProposal = int(((u_i - len(oneDocTopics)) / alphaSum) * numTopics)
    out["doc"] = docTopicIndicatorProposal
    if docTopicIndicatorProposal != oldTopic:                       # :207
        al = alpha[oldTopic]                                        # :210
        n_d_zstar_not_i = float(localTopicCounts_not_i[docTopicIndicatorProposal])    # :249-252
        n_d_zi_not_i = float(localTopicCounts_not_i[oldTopic])
        n_d_zi = float(localTopicCounts[oldTopic])
        n_d_zstar = float(localTopicCounts[docTopicIndicatorProposal])
        nom = phi[docTopicIndicatorProposal][type_] * (al + n_d_zstar_not_i) * (al + n_d_zi)                            # :254
        denom = phi[oldTopic][type_] * (al + n_d_zi_not_i) * (al + n_d_zstar)                                            # :255
        with np.errstate(invalid="ignore", divide="ignore"):
            pi_d = float(np.float64(nom) / np.float64(denom))       # :256
        out["pi_d"] = pi_d
        if pi_d > 1 or U[3] < pi_d:                                 # :212-225
            newTopic = docTopicIndicatorProposal
        else:
            newTopic = oldTopic
    localTopicCounts[oldTopic] -= 1                                 # :235-241
    oneDocTopics[position] = newTopic
    localTopicCounts[newTopic] += 1
    localTopicCounts_not_i[newTopic] += 1
    out["new"] = newTopic
    return out


def test_token_step_is_the_java_text_on_explicit_arrays():
    """Random counts and a random Phi, whole documents position by position (words repeat: nothing moves the type-topic counts
    inside a sweep), the same uniforms on both sides, so that both branches of both proposals and both outcomes of both
    acceptances occur.  pi_w, pi_d, the proposals, the new topic and both histograms must be identical."""
    rng = np.random.default_rng(2025)
    K, V = 7, 12
    beta = 0.37
    alpha = (0.05 + 0.3 * rng.random(K)).tolist()
    total = R.alpha_sum(np.asarray(alpha), K)
    seen = dict(table=0, beta=0, acc_w=0, rej_w=0, acc_d=0, rej_d=0, same_d=0, undone=0)
    for trial in range(40):
        n_wk = rng.integers(0, 4, (V, K))
        length = int(rng.integers(1, 14))
        words = rng.integers(0, V, length)
        zdoc = rng.integers(0, K, length).tolist()
        for w, k in zip(words, zdoc):
            n_wk[w, k] += 1                                         # the document's own tokens are counted
        n_k = n_wk.sum(axis=0)
        phi = rng.dirichlet(np.full(V, 0.4), K)
        ps, a, _, nw, lists, tpt = R.build_tables(n_wk, n_k, beta)
        bh = R.bhat(n_k, beta * V)
        tables = {w: (ps[w][:nw[w]], a[w][:nw[w]]) for w in range(V)}
        nz = {w: lists[w][:nw[w]].tolist() for w in range(V)}
        ltc = np.bincount(zdoc, minlength=K).tolist()
        ltc_i = list(ltc)
        jz = list(zdoc)
        n = list(ltc)
        rz = list(zdoc)
        for pos in range(length):
            w = int(words[pos])
            U = tuple(rng.random(4).tolist())
            j = java_token(phi.tolist(), n_wk.tolist(), bh, tpt.tolist(), nz, tables, ltc, ltc_i, jz, pos, w, alpha, total, beta, K, U)
            det = {}
            R.token_step(n, rz, pos, phi[:, w].tolist(), n_wk[w].tolist(), bh, alpha, total, beta, (ps[w], a[w], lists[w], int(nw[w]), int(tpt[w])), U, det)
            assert det["word"] == j["word"] and det["doc"] == j["doc"] and det["new"] == j["new"] == rz[pos] == jz[pos]
            assert det.get("pi_w") == j.get("pi_w") and det.get("pi_d") == j.get("pi_d")
            assert n == ltc == ltc_i and rz == jz
            seen["table" if det["branch"] == R.TABLE else "beta"] += 1
            if "pi_w" in det:
                seen["acc_w" if det["acc_w"] else "rej_w"] += 1
            if "pi_d" in det:
                seen["acc_d" if det["acc_d"] else "rej_d"] += 1
            else:
                seen["same_d"] += 1
                seen["undone"] += det["acc_w"]
    assert min(seen.values()) >= 5, seen


def test_word_ratio_multiplies_left_to_right():
    """numbers worked by hand: every factor exact in binary, so the products are too"""
    got = R.word_ratio(0.5, 0.25, 0.5, 3, 1, 0.25, 2, 5, 8.0, 16.0)
    assert got == (0.5 * 3.5 * 2.25 * 8.0) / (0.25 * 1.5 * 5.25 * 16.0)
    assert np.isnan(R.word_ratio(0.0, 0.0, 0.5, 1, 0, 0.25, 1, 1, 2.0, 2.0)) and R.word_ratio(0.5, 0.0, 0.5, 1, 0, 0.25, 1, 1, 2.0, 2.0) == np.inf


# ---- the word step alone --------------------------------------------------------------------------------------------
def word_step_matrix(q, ratio, K, n0):
    P = np.zeros((K, K))
    for s in range(K):
        for t in range(K):
            if t != s:
                P[s, t] = q[t] * min(1.0, ratio(s, t, n0[t], n0[s]))    # ni[t] = n0[t], ni[s] = n0[s]: the document without the token
        P[s, s] = 1.0 - P[s].sum()
    return P


@pytest.mark.parametrize("K,alpha,equal_totals", [(3, 0.9, False), (7, 0.1, False), (7, 0.1, True)])
def test_word_step_leaves_its_target_invariant(K, alpha, equal_totals):
    """Symmetric alpha, Phi held at the point estimate (beta + n_wk) / (betaSum + n_k).  Then phi[k] * bhat[k] = beta + G[k] and
    pi_w is (alpha + ni[t]) / (alpha + ni[s]) -- as a quotient of the two four-factor products, to rounding.  A Metropolis step
    with proposal q and acceptance min(1, h(t) / h(s)) leaves h * q invariant, so the word step's target is
    (alpha + ni[k]) * q[k], q being what the table and the beta branch draw with:
        q[k] = (tokensPerType * p_k / typeMass + beta) / (tokensPerType + beta * K),   p_k = G[k] / bhat[k].
    Asserted to 1e-12 on the K x K transition matrix of a fixed document; a swapped ratio is seen.  Where every topic has the
    same total (`equal_totals`) q is proportional to beta + G[k], and the target is the model's own conditional
    (alpha + ni[k]) * phi[k][w]; otherwise it is not -- one of the reasons the chain is approximate as written."""
    rng = np.random.default_rng(K)
    V, beta = 9, 0.3
    G = rng.integers(0, 6, K)
    G[rng.integers(0, K)] = 0                                       # a topic off the word's list: only the beta branch proposes it
    G[0] = max(int(G[0]), 1)
    n_k = np.full(K, 40) if equal_totals else G + rng.integers(0, 40, K)
    beta_sum = beta * V
    bh = R.bhat(n_k, beta_sum)
    phi_w = np.array([(beta + float(G[k])) / bh[k] for k in range(K)])
    lst, ps, a, mass, tpt = R.LC.word_table(G.tolist(), n_k.tolist(), beta_sum)
    qt = SR.implied_probabilities(ps, a)
    q = np.full(K, beta / (tpt + beta * K))
    for i, k in enumerate(lst):
        q[k] += (tpt / (tpt + beta * K)) * qt[i]
    assert abs(q.sum() - 1.0) < 1e-12
    want_q = np.array([(tpt * (G[k] / bh[k]) / mass + beta) / (tpt + beta * K) for k in range(K)])
    assert np.abs(q - want_q).max() < 1e-12
    n0 = rng.integers(0, 5, K)                                      # the document without the token
    ratio = lambda s, t, ni_t, ni_s: R.word_ratio(phi_w[t], phi_w[s], alpha, ni_t, ni_s, beta, G[s], G[t], bh[t], bh[s])   # noqa: E731
    for s in range(K):
        for t in range(K):
            assert abs(ratio(s, t, n0[t], n0[s]) - (alpha + n0[t]) / (alpha + n0[s])) < 1e-12 * (alpha + n0[t]) / (alpha + n0[s])
    target = (alpha + n0) * q
    target /= target.sum()
    P = word_step_matrix(q, ratio, K, n0)
    assert np.abs(target @ P - target).max() < 1e-12
    wrong = word_step_matrix(q, lambda s, t, ni_t, ni_s: ratio(s, t, ni_s, ni_t), K, n0)     # the two document counts swapped
    assert np.abs(target @ wrong - target).max() > 1e-4
    moved = word_step_matrix(q, lambda s, t, ni_t, ni_s: R.word_ratio(phi_w[t], phi_w[s], alpha, ni_t, ni_s, beta, G[t], G[s], bh[t], bh[s]), K, n0)
    assert np.abs(target @ moved - target).max() > 1e-4             # (beta + G) on the wrong sides of the quotient is seen
    conditional = (alpha + n0) * phi_w
    conditional /= conditional.sum()
    assert (np.abs(target - conditional).max() < 1e-12) == equal_totals


# ---- the z step -----------------------------------------------------------------------------------------------------
def small_model(oracle):
    rng = np.random.default_rng(4)
    K, V = 5, 12
    lens = np.array([7, 0, 1, 30, 3])
    doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    tokens = rng.integers(0, V, lens.sum())
    z = rng.integers(0, K, lens.sum())
    return R.Model(K, V, np.array([0.1, 0.5, 0.9, 0.2, 0.3]), 0.3, 99, doc_ptr, tokens, z)


def test_counters_and_counts_after_sweeps(oracle):
    m = small_model(oracle)
    m.init_phi()
    for _ in range(4):
        before = m.z.copy()
        stats0 = m.stats.copy()
        m.sweep(1)
        s = m.stats - stats0
        assert s.sum() == m.tokens.size and s.min() >= 0
        assert s[R.STAY] <= int((m.z == before).sum())              # a token left on z0 has not moved; a proposal may also land on z0
        n_wk, n_k = R.count(m.tokens, m.z, m.V, m.K)
        assert (n_wk == m.counts()).all() and (n_k == m.topic_totals()).all()
    assert (m.stats > 0).all() and (m.branches > 0).all() and m.branches.sum() == 4 * m.tokens.size


def test_the_counts_stay_put_inside_a_sweep(oracle):
    """Unlike lightcollapsed nothing moves G for the token in flight: the z step on counts that are NOT those of z (a stale
    merge) reads them as they are and leaves them untouched."""
    m = small_model(oracle)
    m.init_phi()
    n_wk, n_k = m.start_counts()
    keep = (n_wk.copy(), n_k.copy())
    z = m.z.copy()
    R.z_step(m.doc_ptr, m.tokens, z, m.phi, n_wk, n_k, m.alpha, m.beta, R.build_tables(n_wk, n_k, m.beta), m.seed, 1)
    assert (n_wk == keep[0]).all() and (n_k == keep[1]).all() and (z != m.z).any()


# ---- distance from the enumerated posterior ---------------------------------------------------------------------------
N, THIN, SEEDS = 4000, 8, (1, 2, 3)


def chain(O, fx, seed, n=N):
    z0 = O.jrandom_ints(seed, fx.K, len(fx.tokens))
    m = R.Model(fx.K, fx.V, np.asarray(fx.alpha, np.float64), fx.beta, seed, fx.doc_ptr, fx.tokens, z0)
    m.init_phi()
    return LP.run_chain(m.sweep, lambda: m.z, fx.K, n, THIN, LP.BURN_IN, max_topic=fx.K - 1)


def test_distance_from_the_enumerated_posterior(oracle):
    """Fixture A (asymmetric alpha) and the same corpus with alpha = 0.9 symmetric; n = 4000, thin 8, three seeds: lightpclda's
    settings (tests/test_lightpclda_model.py).  The chain is approximate as written, so NO p-value is asserted: chi-square and
    total variation are printed (DESIGN.md 2 records them beside lightpclda's and lightcollapsed's).  Asserted: every visited
    state is in range and every chain visits at least half of the 729 states."""
    from oracle import oracle as O
    A = LP.FIXTURE_A
    sym = A._replace(alpha=(0.9, 0.9, 0.9))
    for name, fx in (("fixture A, alpha (0.3, 0.9, 1.7)", A), ("fixture A's corpus, alpha 0.9", sym)):
        post = LP.enumerate_posterior(fx.doc_ptr, fx.tokens, fx.K, fx.V, fx.alpha, fx.beta)
        for seed in SEEDS:
            idx = chain(O, fx, seed)
            assert idx.min() >= 0 and idx.max() < post.p.size
            v = LP.verdict(idx, post.p)
            visited = int((LP.histogram(idx, post.p.size) > 0).sum())
            print("lightpcldaw2, %s, seed %d: chi2 %.1f on %d dof (p = %.3g), total variation %.4f, n = %d, %d of %d states visited"
                  % (name, seed, v.chi2, v.dof, v.pvalue, v.tv, v.n, visited, post.p.size))
            assert v.n == N and 2 * visited >= post.p.size, (name, seed, visited)
