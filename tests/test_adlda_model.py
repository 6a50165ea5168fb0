"""scheme=adlda without a device: the restatement's per-token draw (tests/adlda_restatement.py) against the dense conditional
of scheme=collapsed's parallel schedule, with three mutants that the same check refuses; the edges of the restatement, each
with the bucket it takes; the public surface (flag, header, Java constant, kernel name, refused combinations, create_model,
the resource summary's rows)."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import adlda_restatement as R
from tests.diagnostics_cases import asymmetric_alpha

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, RB, S = R.BUCKET_Q, R.BUCKET_R, R.BUCKET_S


# ---- the public surface (the first test: it fails on a build without the scheme) --------------------------------------
def test_flag_header_java_constant_and_entry_points():
    from ldagroupedgibbssampler_amd import _lib, native, sampler
    assert native.FLAG_ADLDA == 1024 and sampler.ADLDA._scheme_flags == native.FLAG_ADLDA
    m = sampler.ADLDA(sampler.SimpleLDAConfiguration(topics=4, seed=1))
    assert isinstance(m, sampler.LDAGroupedGibbsSampler)
    for name in ("getWordTopicLists", "getSparseStats"):
        assert callable(getattr(m, name))
    with pytest.raises(NotImplementedError):
        m.getTheta()
    with pytest.raises(NotImplementedError):
        m.sampleZGivenPhi(1)
    header = open(_lib.HEADER_PATH).read()
    assert re.search(r"GGS_FLAG_ADLDA\s*=\s*1\s*<<\s*10", header)
    assert "#define GGS_ABI_VERSION 6" in header                    # a new bit, not a new ABI version
    java = open(os.path.join(ROOT, "integration", "java", "cc", "mallet", "topics", "GGSNative.java")).read()
    assert "FLAG_ADLDA = 1024" in java
    assert native.Z_KERNEL_NAMES[11] == "adlda_wave_kernel (wave per document)"
    with pytest.raises(ValueError):                                 # constructed directly: the registry keeps refusing the name
        sampler.create_model(sampler.SimpleLDAConfiguration(topics=4, seed=1), "adlda")
    assert "adlda" in sampler.create_model.__doc__


def test_flag_combinations_are_refused():
    """GGS_FLAG_ADLDA with any other scheme's flag is GGS_ERR_BAD_ARG: an argument check, answered before ggs_create asks for a
    device -- so it can be seen here."""
    from ldagroupedgibbssampler_amd import native
    for other in (native.FLAG_COLLAPSED, native.FLAG_PCGS, native.FLAG_POLYAURN, native.FLAG_SPALIAS, native.FLAG_LIGHTPCLDA,
                  native.FLAG_POLYAURN_SPARSE, native.FLAG_LIGHTCOLLAPSED, native.FLAG_NZVSSPALIAS):
        with pytest.raises(native.GGSError) as e:
            native.GGSHandle(5, 10, 0.1, 0.01, 1, flags=native.FLAG_ADLDA | other)
        assert e.value.code == native.ERR_BAD_ARG


def test_the_kernels_use_no_scratch():
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
    for k in ("ggs::adlda_wave_kernel", "ggs::adlda_head_kernel", "ggs::word_list_counts_kernel"):
        assert k in rows, "%s is not in the build" % k
        assert rows[k][3] == 0, "%s spills %d bytes per lane" % (k, rows[k][3])


# ---- states ---------------------------------------------------------------------------------------------------------------
class State:
    """A small corpus with its assignments and one token of it picked out: what token_masses needs, and the dense conditional."""

    def __init__(self, K, V, lens, alpha, beta, seed, tokens=None, z=None, pick=None):
        rng = np.random.default_rng(seed)
        self.K, self.V, self.beta = K, V, beta
        self.alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
        self.doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        n = int(self.doc_ptr[-1])
        self.tokens = rng.integers(0, V, n) if tokens is None else np.asarray(tokens)
        self.z = rng.integers(0, K, n) if z is None else np.asarray(z)
        self.n_wk, self.n_k = R.count(self.tokens, self.z, V, K)
        self.pick = int(rng.integers(0, n)) if pick is None else pick
        self.d = int(np.searchsorted(self.doc_ptr, self.pick, side="right")) - 1

    def masses(self, mutant=None):
        """the picked token's masses with every earlier token of its document still on its old topic (any state of the document
        is a state the chain can be in)"""
        b, e = int(self.doc_ptr[self.d]), int(self.doc_ptr[self.d + 1])
        st = R.DocState(self.K, self.z[b:e])
        w, z0 = int(self.tokens[self.pick]), int(self.z[self.pick])
        st.remove(z0)
        den0, s0, nw, lists = R.head(self.n_wk, self.n_k, self.alpha, self.beta)
        self.st, self.w, self.z0 = st, w, z0
        return R.token_masses(st, z0, self.n_wk[w].tolist(), lists[w, :int(nw[w])].tolist(), [int(x) for x in self.n_k], den0, s0, self.alpha,
                              self.beta, self.beta * float(self.V), mutant)

    def dense(self):
        """(alpha_k + n_dk)(beta + G'(k)) / den(k), normalised, in exact rational arithmetic: what scheme=collapsed's parallel
        restatement in the oracle scores (the document's counts and the word's and the topic's sweep-start counts, each
        without the token)"""
        b, e = int(self.doc_ptr[self.d]), int(self.doc_ptr[self.d + 1])
        nd = np.bincount(self.z[b:e], minlength=self.K).astype(np.int64)
        w, z0 = int(self.tokens[self.pick]), int(self.z[self.pick])
        nd[z0] -= 1
        beta, bs = Fraction(self.beta), Fraction(self.beta * float(self.V))   # betaSum is the rounded product, as the kernels form it
        p = []
        for k in range(self.K):
            own = 1 if k == z0 else 0
            p.append((Fraction(float(self.alpha[k])) + int(nd[k])) * (beta + int(self.n_wk[w][k]) - own) / (int(self.n_k[k]) - own + bs))
        tot = sum(p)
        return [x / tot for x in p]


GRID_BITS = 40                                                      # the grid of U: i * 2^-40, i = 1 .. 2^40 - 1, each exactly a double


def u_set_lengths(m, K):
    """The length of the set of grid points U that token_walk maps to each topic, times the grid step, and the buckets seen.
    (topic bucket, index) is monotone in U -- U * total, the comparisons with Q and R, every subtraction and the division by
    beta are monotone in their first operand -- so the 2^40 grid points are counted by bisecting for the change points
    instead of visiting them."""
    G = 1 << GRID_BITS
    h = 1.0 / G
    cache = {}

    def f(i):
        if i not in cache:
            det = {}
            t, b = R.token_walk(m, i * h, det)
            cache[i] = ((b, det.get("index", t)), t)
        return cache[i]

    counts, buckets = [0] * K, set()

    def walk(lo, hi):                                               # grid points lo .. hi inclusive
        a, b = f(lo), f(hi)
        if a[0] == b[0]:
            counts[a[1]] += hi - lo + 1
            buckets.add(a[0][0])
            return
        assert a[0] < b[0], "not monotone in U"
        mid = (lo + hi) // 2
        walk(lo, mid)
        walk(mid + 1, hi)

    walk(1, G - 1)
    return [c * h for c in counts], buckets


def rounding_bound(m):
    """A change point of the map U -> topic is where U * total passes a partial sum of the masses.  With u = 2^-53 and n = nnz_w
    + nnz_d + K terms: every term carries at most 3 u relative error (a sum, a quotient, a product), the k-order, list-order
    and walk chains at most one u of the total per operation, fewer than n + 8 operations each, S0 - x + y (x, y <= S0 up to
    rounding) two more, U * total and the division by beta one each: a change point moves by at most (2 n + 16) u in U.  The
    U-set of a topic is at most three intervals (one per bucket), six change points: 6 (2 n + 16) u, rounded up to
    16 (n + 8) u."""
    n = len(m["scores"]) + len(m["doc_list"]) + m["K"]
    return 16.0 * (n + 8) * 2.0 ** -53


def grid_allowance():
    """A union of at most three intervals holds within one grid point per interval of its length over the step: three steps
    of the 2^-40 grid, 2.8e-12 -- well inside the one step of any grid that could be visited point by point."""
    return 3.0 * 2.0 ** -GRID_BITS


def random_states():
    out = []
    for K in (1, 2, 5, 65):
        for asym in (False, True):
            for s in range(3):
                rng = np.random.default_rng(1000 * K + 10 * s + asym)
                V = int(rng.integers(1, 13))
                lens = rng.integers(1, 41, int(rng.integers(1, 7)))
                out.append(State(K, V, lens, asymmetric_alpha(K) if asym else 0.1 * (1 + s), [0.01, 0.5, 3.0][s], 77 * K + s + 5 * asym))
    return out


def zero_entry_states():
    """states whose token is the only one of (w, z0) while L_w has an entry before z0: the word's list keeps z0 with score 0.0
    behind a positive score"""
    out = []
    for K in (2, 5, 65):
        for s in range(40):
            st = State(K, 3, [12, 7, 30], 0.3, 0.1, 31 * K + s)
            w, z0 = int(st.tokens[st.pick]), int(st.z[st.pick])
            row = st.n_wk[w]
            if row[z0] == 1 and (row[:z0] > 0).any():
                out.append(st)
    assert len(out) >= 5
    return out[:8]


def worst_deviation(states, mutant=None):
    worst, bound_at = -1.0, 1.0
    for st in states:
        m = st.masses(mutant)
        lengths, _ = u_set_lengths(m, st.K)
        want = st.dense()
        dev = max(abs(Fraction(lengths[k]) - want[k]) for k in range(st.K))
        allowed = grid_allowance() + rounding_bound(m)
        if float(dev) / allowed > worst / bound_at:                  # the state nearest to (or furthest past) its bound
            worst, bound_at = float(dev), allowed
    return worst, bound_at


def test_the_draw_has_the_dense_conditional_of_the_collapsed_parallel_schedule():
    states = random_states() + zero_entry_states()
    worst, bound = worst_deviation(states)
    print("adlda conditional over %d states: worst deviation %.3g against the bound %.3g (grid %.3g + rounding %.3g)"
          % (len(states), worst, bound, grid_allowance(), bound - grid_allowance()))
    assert worst <= bound


@pytest.mark.parametrize("mutant", ["G", "T", "zero"])
def test_mutants_fail_the_same_check(mutant):
    states = random_states() + zero_entry_states()
    worst, bound = worst_deviation(states, mutant)
    print("mutant %r: worst deviation %.3g against the bound %.3g" % (mutant, worst, bound))
    assert worst > bound


# ---- edges of the restatement ---------------------------------------------------------------------------------------------
def buckets_over_a_grid(m, n=4001):
    seen = {}
    for i in range(1, n):
        t, b = R.token_walk(m, i / n)
        seen.setdefault(b, set()).add(t)
    return seen


def test_edge_one_topic():
    st = State(1, 4, [6, 3], 0.7, 0.1, 1)
    m = st.masses()
    seen = buckets_over_a_grid(m)
    assert set().union(*seen.values()) == {0}
    assert set(seen) == {Q, RB, S}                                   # the other five tokens of (d, 0) and the word's other tokens: all three buckets
    assert R.token_walk(m, 1.0 - 2.0 ** -53) == (0, S)


def test_edge_one_token_document():
    st = State(5, 3, [1, 9], 0.2, 0.1, 2, pick=0)
    m = st.masses()
    assert st.st.list == [] and m["R"] == 0.0 and m["doc_list"] == []
    seen = buckets_over_a_grid(m)
    assert RB not in seen and S in seen


def test_edge_the_words_only_token():
    tokens, z = [0, 1, 1, 2, 1, 2], [3, 1, 1, 0, 2, 2]
    st = State(4, 3, [3, 3], 0.2, 0.1, 3, tokens=tokens, z=z, pick=0)
    m = st.masses()
    assert m["list_w"] == [3] and m["scores"] == [0.0] and m["Q"] == 0.0
    seen = buckets_over_a_grid(m)
    assert Q not in seen and set(seen) == {RB, S}


def test_edge_a_zero_score_entry_among_others():
    tokens, z = [0, 0, 0, 1, 0, 1], [2, 0, 3, 1, 0, 3]
    st = State(4, 2, [3, 3], 0.2, 0.1, 4, tokens=tokens, z=z, pick=0)   # N[0] = [2, 0, 1, 1]; the token is the 1 at topic 2
    m = st.masses()
    assert m["list_w"] == [0, 2, 3] and m["scores"][1] == 0.0 and m["scores"][0] > 0 and m["scores"][2] > 0
    seen = buckets_over_a_grid(m)
    assert seen[Q] == {0, 3}                                        # the entry stays in the list and is never the word bucket's draw
    assert 2 in seen[S]                                             # its mass is the smoothing bucket's (the document has left topic 2)


def test_edge_the_last_entry_of_each_bucket():
    st = State(5, 3, [12, 7, 30], asymmetric_alpha(5), 0.1, 9)
    m = st.masses()
    total = m["S"] + m["R"] + m["Q"]
    assert len(m["scores"]) >= 2 and len(m["doc_list"]) >= 2 and m["scores"][-1] > 0
    det = {}
    assert R.token_walk(m, (m["Q"] / total) * (1 - 2.0 ** -30), det) == (m["list_w"][-1], Q) and det["index"] == len(m["scores"]) - 1
    det = {}
    assert R.token_walk(m, ((m["Q"] + m["R"]) / total) * (1 - 2.0 ** -30), det) == (m["doc_list"][-1], RB)
    assert det["index"] == len(m["doc_list"]) - 1 and "fallback" not in det
    assert R.token_walk(m, 1.0 - 2.0 ** -53) == (4, S)
    assert R.token_walk(m, 2.0 ** -53) == (m["list_w"][0], Q)


def test_edge_the_fallback_of_the_document_walk():
    """sample < R, yet sample / beta stays positive behind the list's last n_d[c] / den(c): the reference's K - 1 (:332-336).  R
    sums (beta * n) / den while the walk subtracts n / den from sample / beta, so the two can disagree by rounding.  Searched
    here at the doubles next to the bucket's upper end over 400 random states: state 393 reaches it."""
    reached = None
    for s in range(400):
        rng = np.random.default_rng(s)
        K = int(rng.integers(2, 9))
        st = State(K, int(rng.integers(2, 6)), rng.integers(2, 30, 3), float(rng.uniform(0.05, 2.0)), float(rng.uniform(0.01, 1.5)), s)
        m = st.masses()
        if not m["doc_list"]:
            continue
        total = m["S"] + m["R"] + m["Q"]
        u = (m["Q"] + m["R"]) / total
        for _ in range(6):
            u = math.nextafter(u, 0.0)
            det = {}
            t, b = R.token_walk(m, u, det)
            if det.get("fallback"):
                assert (t, b) == (K - 1, RB)
                reached = (s, u)
                break
        if reached:
            break
    print("the K - 1 fallback of the document walk: %s" % ("reached at state %d, U = %r" % reached if reached else "unreached in 400 states"))
    assert reached is not None
