"""Knife-edge rows for the token draw of scheme=adlda (a test helper, not collected; the manner and the vocabulary of
tests/lightcollapsed_knife_edge.py: Row, tags, `useful`, survey).

The token draw (ggs_z_adlda.hpp, tests/adlda_restatement.token_masses / token_walk) makes five comparisons, all of them
monotone in sample = U * (S + R + Q):

  a  word bucket          sample < Q
  b  document bucket      sample - Q < R
  c  Q walk stop          the sample left behind entry i of L_w is > 0          (the walk goes on)
  d  R walk stop          the sample (in units of beta) left behind entry i of the document's list is <= 0.0
  e  S walk stop          the sample (in units of beta) left behind topic k is not > 0.0

Knob.  There is no Phi, the counts are integers and U is fixed by (seed, iteration, global token index).  What moves
continuously is alpha, fixed at ggs_create: every knob value is a handle.  Topic SLACK = K - 1 holds no token of z0, so it
is in no word's list L_w and is no token's z0: its alpha enters S0 (the last term of the k-order chain) and the last term
of the S walk, nothing else.  S0 is global, so one alpha vector aims ONE row: _bisect over the bit pattern of alpha[SLACK]
in [A_LO, A_HI] finds two adjacent doubles between which the row's comparison flips, and the row's two handles are those.
The set of knob values at which the two sides are EQUAL, if there is one, lies next to the flip on one side of it, so a tie
is always one of the two handles and costs no third one.  Every other row still runs under every vector and is compared;
a row counts under every vector at which its comparison sits on an edge.

Corpus.  One corpus and one z0, K = 130, alpha of order 1 (eight values in turn), beta = 0.45 (no power of two: with 0.5
the division by beta is exact and (beta * n) / den is n / den halved, so the R walk in units of beta would round as the
undivided one).  N_LONG documents of 140 tokens hold 76 tokens of a word of their own on 76 different topics (a word list
and a document list of more than 64 entries; every one of those tokens is the only one of (w, z0), a score-0.0 entry of
its own list) between ballast words; N_SHORT documents of 40 to 60 tokens hold their own word on 3 to 6 of the document's 10
topics, one token of it on the lowest of them (a zero entry at the head of the word's list) and 1 to 6 on each other.  The ballast words are shared, about a hundred tokens each, so their lists pass 64 entries as well.

Rows.  A row is a document with one target token; a document carries one row.  Under the parallel schedule a token sees
the sweep-start N[w][.] and T[.] (fixed by z0: where the word's other tokens lie in the corpus does not matter) and its
document's running counts and list, so the tokens IN FRONT of the target matter: they are redrawn under the same alpha
vector, and the builder predicts them with its own step() -- the target is evaluated by running step() over its
document from the first token on, at every probe of the bisection.  Candidates are the first forty positions of a document
(and 62 to 65 of the long ones, which took no row: the search stops at the first candidate that serves).  The builder asserts through the restatement
that step() draws what the restatement draws at EVERY token (whole z steps: see Edges.restatement), and that the prefix of
a row is the same at its two handles.

Positions (the boundary between two neighbouring stops; "i|j": the flip is between a stop at i and a stop at j):
  c  0|1; 63|64 of a list of more than 64 entries; the last two entries; "zero behind": the stop at the entry right in
     front of a score-0.0 entry (the walk that goes on steps over the zero entry); "zero first": the score-0.0 entry heads
     the list, the flip is 1|2, the first stop the walk can make.  A zero entry is z0's where N[w][z0] == 1.
  d  0|1; 63|64 of a document list of more than 64 entries; the last two entries of the document's list ("last")
  e  0|1; 63|64; K-2|K-1

Tags.  The computed side of a walk's comparison is the sample BEFORE the subtraction, its bound the term subtracted: the
difference of two doubles within a factor of two is exact, so "tie" is a remaining sample of exactly 0.0 and "below" /
"above" are the neighbouring doubles of the term (zero's own neighbours are denormals no product here reaches).  For a
and b the sides are (sample, Q) and (sample - Q, R).  A (row, knob value) counts only where forcing the comparison both
ways gives two different new topics (`useful`), and a row only with a flip pair.

Which ties the grids allow.  sample = U * total moves in steps of its own ulp as alpha[SLACK] moves in finer ones, so
sample == Q is reached wherever U's and the total's mantissas multiply to 2 or more (else sample can step over a double)
and Q is not in a finer binade: nearly every a candidate.  sample - Q lies on sample's (coarser) grid, R on its own: a b
tie needs R's low bits zero, about one flip in four.  A walk's tie needs the sample left behind i - 1 subtractions
(for d and e, a division by beta too) to BE the term: one flip in fifty for d at entry 0, one in seven for e at k = 0, rarer
behind; at entry 0 of the Q walk it is a's case again.  The builder takes targets where the values it needs exist and searches as many candidates as that takes.

Proposal rows (no handle of their own: read off the first handle's z step).  Tokens drawn from the Q or the R bucket of a
list of more than 64 entries whose walk ends at entry 0, 62, 63, 64, 65 or the last one -- `decide`'s
l == 0 ? start - before : read_lane(dd, l - 1) and the carried `before` -- with, in exact rational arithmetic, start -
prefix more than 4 delta from zero on both neighbours (delta = (8 n + 64) 2^-53 T), the bucket's own comparison
included: with the margin unset the scans decide such a row whatever their association.  One more kind, "zero": a Q draw
whose entry before the stop scores 0.0 -- equal neighbours, which `decide` refuses: the row goes to the replay.

The reference's three rare paths.  Two are within the knob's reach and are rows of their own (KE.RARE):
  a "raise"     the Q walk running past its last entry: sample < Q by the chain's Q, yet the subtractions leave a positive
                rest.  In a list of 60 and more entries the doubles right under Q do that often (at 21 of the 3 870
                probes around the 30 bucket-edge candidates the search visits).  The row's lower handle is GGS_ERR_INVALID_TOPIC with
                the topic clamped to the last entry; its upper handle draws from the R bucket.
  d "fallback"  the R walk's K - 1: sample - Q < R, yet sample / beta stays positive behind the list's last n_d[c] / den(c).
                No error; the row's flip is between the stop at the last entry and K - 1 (here the slack topic).
The S walk reaching K needs U * total within a rounding of the total, that is U within 2^-50 of 1, whatever the knob: not
reached at any of the 3 870 probes within 64 doubles of the 30 a and b candidates' flips (Edges.rare; the model test
prints the counts), and no row.

step() = masses() + draw() is the builder's own arithmetic in plain Python floats, written apart from the restatement,
with `force` and the switchable SLIPS -- each a plausible rewrite of the kernel."""
import json
import os
from fractions import Fraction

import numpy as np

from oracle import oracle as O
from tests import adlda_restatement as R
from tests.adlda_restatement import PURPOSE_Z, InvalidTopic
from tests.lightpclda_knife_edge import TAGS, Row, _bisect, _bits, _dbl, tag_of  # noqa: F401

K = 130
SLACK = K - 1
ALPHA = np.resize(np.array([1.0, 1.2, 0.8, 1.1, 0.9, 1.3, 0.7, 1.05]), K)
BETA = 0.45
SEED = 4242
CORPUS_SEED = 11
ITERATION = 1
MAX_HANDLES = 48
A_LO, A_HI = 0.02, 200.0                                            # alpha[SLACK] is bisected between
WINDOW = 64                                                         # doubles around a flip searched for the rare paths
N_LONG, N_SHORT, N_WORDS = 8, 34, 18                                # documents; shared ballast words
LONG_LEN, OWN_LONG = 140, 76
BQ, BR, BS = 0, 1, 2

# slip -> the comparisons it belongs to
SLIPS = {"q_le": "a", "r_le": "b", "qwalk_ge": "c", "rwalk_lt": "d", "swalk_ge": "e", "rwalk_undivided": "d", "walk_by_prefix": "cde",
         "sum_tree": "ab", "s0_tree": "abcde", "s_assoc": "abcde", "score_mul_first": "abc", "zero_skip": "c", "den_stale": "abcde"}
# Show on random data: the stale den(z0) moves every mass a little; zero_skip draws another topic wherever a zero entry follows
# the stop, edge or no edge (cats has hundreds of such draws).  The device suite's random corpora already tell these two.
INDEX_SLIPS = ("den_stale", "zero_skip")
ORDER_SLIPS = tuple(s for s in SLIPS if s not in INDEX_SLIPS)       # must not
MASS_SLIPS = ("rwalk_undivided", "sum_tree", "score_mul_first", "den_stale")     # change masses(); the others only draw() or the head

# what the rows are to hold: (comparison, position, a tie wanted); "any": whichever boundary of the first few gives a tie
# The rarest first (a document carries one row).  A fourth element names a slip the row is to show: a score rounds otherwise
# multiplied first only where the word's count is 3, 5, 6, ..., which most words here do not have.  The second tie of d and of e is looked for at entry 0 as well: there a tie
# is likeliest (for e about one flip in seven, for d one in fifty; behind entry 0 d gave 1 tie in 120 flips).
NEEDS = [("d", "0|1", True), ("d", "0|1", True), ("d", "fallback", False), ("c", "0|1", True), ("b", "-", True), ("e", "0|1", True), ("e", "0|1", True),
         ("a", "raise", False), ("c", "zero first", False), ("c", "zero behind", False), ("c", "any", True), ("a", "-", True, "score_mul_first"),
         ("a", "-", True), ("a", "-", True), ("b", "-", False), ("b", "-", False), ("c", "63|64", False), ("c", "last two", False), ("d", "63|64", False),
         ("d", "last", False), ("e", "63|64", False), ("e", "K-2|K-1", False)]
RARE = (("a", "raise"), ("d", "fallback"))                          # the reference's rare paths that the knob reaches: rows as well
POSITIONS = {"a": ("-",), "b": ("-",), "c": ("0|1", "63|64", "last two", "zero behind", "zero first"), "d": ("0|1", "63|64", "last"),
             "e": ("0|1", "63|64", "K-2|K-1")}
MIN_FLIP_ROWS = 3                                                   # rows with a flip pair per comparison
MIN_TIES = {"a": 3, "b": 1, "c": 2, "d": 2, "e": 2}                 # c, d, e: one of them at entry 0
PROPOSAL_ENTRIES = ("0", "62", "63", "64", "65", "last")


def _chain(xs):
    s = 0.0
    for x in xs:
        s = s + x
    return s


def _tree(xs):
    xs = list(xs)
    if not xs:
        return 0.0
    while len(xs) > 1:
        xs = [xs[i] + xs[i + 1] if i + 1 < len(xs) else xs[i] for i in range(0, len(xs), 2)]
    return xs[0]


class _Doc:
    """a document's counts and the list of its topics: first-occurrence order, the last entry fills a hole"""

    def __init__(self, nK, zdoc):
        self.cnt, self.list, self.at = [0] * nK, [], {}
        for k in zdoc:
            self.add(k)

    def add(self, k):
        self.cnt[k] += 1
        if self.cnt[k] == 1:
            self.at[k] = len(self.list)
            self.list.append(k)

    def remove(self, k):
        self.cnt[k] -= 1
        if self.cnt[k] == 0:
            i, last = self.at.pop(k), self.list.pop()
            if last != k:
                self.list[i], self.at[last] = last, i


def head(n_k, alpha, beta, bS, slip=None):
    """(den0, S0, the S walk's terms alpha_k / den0[k])"""
    den0 = [float(int(t)) + bS for t in n_k]
    terms = [(alpha[k] * beta) / den0[k] for k in range(len(den0))]
    return den0, (_tree(terms) if slip == "s0_tree" else _chain(terms)), [alpha[k] / den0[k] for k in range(len(den0))]


def masses(cnt, dlist, z0, row_w, list_w, T, den0, alpha, beta, bS, slip=None):
    """What the draw of a token needs that U and S0 do not enter; cnt / dlist: the document with the token taken out.  No
    alpha but those of z0 and of the word's topics is read."""
    dz = den0[z0] if slip == "den_stale" else float(T[z0] - 1) + bS
    ab = alpha[z0] * beta
    rt, rw, sc = [], [], []
    for c in dlist:
        den = dz if c == z0 else den0[c]
        rt.append((beta * float(cnt[c])) / den)
        rw.append(float(cnt[c]) / den)
    for k in list_w:
        den = dz if k == z0 else den0[k]
        g = float(row_w[k] - (1 if k == z0 else 0))
        a = alpha[k] + float(cnt[k])
        sc.append(a * g / den if slip == "score_mul_first" else (a / den) * g)
    total = _tree if slip == "sum_tree" else _chain
    return dict(z0=z0, x=ab / den0[z0], y=ab / dz, sz=alpha[z0] / dz, R=total(rt), Q=total(sc), sc=sc, rt=rt, rw=rt if slip == "rwalk_undivided" else rw,
                list_w=list_w, dlist=list(dlist))


def draw(m, s0, sw, beta, U, slip=None, force=None, detail=None):
    """(topic, bucket, index) of the token with the masses m at the uniform U; sw = the S walk's terms over den0.
    force = (comparison, entry or None, outcome): a -- sample < Q; b -- sample - Q < R; c, d, e -- the walk stops behind
    that entry.  A forced walk that leaves its bucket is clamped; an unforced one raises as the restatement does."""
    fk, fi, fv = force if force is not None else (None, None, None)
    nK = len(sw)
    S = s0 + (m["y"] - m["x"]) if slip == "s_assoc" else s0 - m["x"] + m["y"]
    R_, Q, sc = m["R"], m["Q"], m["sc"]
    sample = U * (S + R_ + Q)
    sides = {("a", None): (sample, Q)} if detail is not None else None
    if detail is not None:
        detail.update(S=S, sample=sample, sides=sides)
    by_prefix = slip == "walk_by_prefix"
    in_q = sample <= Q if slip == "q_le" else sample < Q
    if fk == "a":
        in_q = fv
    start = s = sample
    run = 0.0
    if in_q:
        n, i = len(sc), 0
        while True:
            if i >= n:
                if force is None:
                    raise InvalidTopic("the Q walk runs past the word's last entry", (m["list_w"][n - 1], BQ, n - 1))
                i = n - 1
                break
            before = s
            if by_prefix:
                run = run + sc[i]
                s = start - run
            else:
                s = s - sc[i]
            go = s >= 0 if slip == "qwalk_ge" else s > 0
            if sides is not None:
                sides[("c", i)] = (before, sc[i])
            if fk == "c" and fi == i:
                go = not fv
            if not go:
                break
            i += 1
        if slip == "zero_skip" and i + 1 < n and sc[i + 1] == 0.0:
            i += 1
        out = (m["list_w"][i], BQ, i)
    else:
        s = sample - Q
        in_r = s <= R_ if slip == "r_le" else s < R_
        if sides is not None:
            sides[("b", None)] = (s, R_)
        if fk == "b":
            in_r = fv
        if in_r:
            if slip != "rwalk_undivided":
                s = s / beta
            start, rw = s, m["rw"]
            out = (nK - 1, BR, len(rw))                             # the reference's fallback, no error
            for i, t in enumerate(rw):
                before = s
                if by_prefix:
                    run = run + t
                    s = start - run
                else:
                    s = s - t
                stop = s < 0.0 if slip == "rwalk_lt" else s <= 0.0
                if sides is not None:
                    sides[("d", i)] = (before, t)
                if fk == "d" and fi == i:
                    stop = fv
                if stop:
                    out = (m["dlist"][i], BR, i)
                    break
        else:
            s = s - R_
            s = s / beta
            start, z0, k = s, m["z0"], 0
            while True:
                t = m["sz"] if k == z0 else sw[k]
                before = s
                if by_prefix:
                    run = run + t
                    s = start - run
                else:
                    s = s - t
                go = s >= 0 if slip == "swalk_ge" else s > 0.0
                if sides is not None:
                    sides[("e", k)] = (before, t)
                if fk == "e" and fi == k:
                    go = not fv
                if not go:
                    break
                k += 1
                if k == nK:
                    if force is None:
                        raise InvalidTopic("the S walk reaches K", (nK - 1, BS, nK - 1))
                    k = nK - 1
                    break
            out = (k, BS, k)
    if detail is not None:
        detail["out"] = out
    return out


def step(cnt, dlist, z0, row_w, list_w, T, den0, s0, sw, alpha, beta, bS, U, slip=None, force=None, detail=None):
    """the draw of one token whose old topic has been taken out of (cnt, dlist): (topic, bucket, index)"""
    return draw(masses(cnt, dlist, z0, row_w, list_w, T, den0, alpha, beta, bS, slip if slip in MASS_SLIPS else None), s0, sw, beta, U, slip, force, detail)


def z_step(doc_ptr, tokens, z, n_wk, n_k, alpha, beta, U, slips=()):
    """One z step with step() in place on z against the sweep-start counts; returns (the four counters, whether a walk
    left its bucket, {slip: tokens that slip alone draws otherwise, each from the unmutated state in front of it}) -- a
    slip with no such token gives the same z as a whole step of its own would."""
    n_wk = np.asarray(n_wk)
    V, nK = n_wk.shape
    alpha = [float(x) for x in np.broadcast_to(np.asarray(alpha, np.float64), (nK,))]
    bS = beta * float(V)
    den0, s0, sw = head(n_k, alpha, beta, bS)
    s0_of = {s: (head(n_k, alpha, beta, bS, s)[1] if s == "s0_tree" else s0) for s in slips}
    T = [int(x) for x in n_k]
    rows, lists = {}, {}
    stats, raised, changed = [0, 0, 0, 0], False, dict.fromkeys(slips, 0)
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        st = _Doc(nK, [int(k) for k in z[b:e]])
        for t in range(b, e):
            w, z0 = int(tokens[t]), int(z[t])
            if w not in rows:
                rows[w] = n_wk[w].tolist()
                lists[w] = [k for k in range(nK) if rows[w][k] > 0]
            st.remove(z0)
            m = masses(st.cnt, st.list, z0, rows[w], lists[w], T, den0, alpha, beta, bS)
            try:
                out = draw(m, s0, sw, beta, U[t])
            except InvalidTopic as ex:
                out, raised = ex.args[1], True
            for s in slips:
                ms = masses(st.cnt, st.list, z0, rows[w], lists[w], T, den0, alpha, beta, bS, s) if s in MASS_SLIPS else m
                try:
                    other = draw(ms, s0_of[s], sw, beta, U[t], s)[0]
                except InvalidTopic as ex:
                    other = ex.args[1][0]
                changed[s] += other != out[0]
            stats[out[1]] += 1
            stats[3] += len(lists[w]) + len(st.list)
            st.add(out[0])
            z[t] = out[0]
    return stats, raised, changed


class Edges:
    """rows=None: the whole search (about ten seconds).  rows = recorded(): each row aimed again at the candidate the search
    took -- its own bisection, asserted to end on the recorded bit pattern -- which is what the device test affords."""

    def __init__(self, seed=CORPUS_SEED, rows=None):
        self._corpus(np.random.default_rng(seed))
        self.searched = rows is None
        if rows is None:
            self._search()
        else:
            self._recorded(rows)
        self._settle()
        self._proposals(None if rows is None else rows["base"])

    # ---- the corpus ----------------------------------------------------------------------------------------------------------
    def _corpus(self, rng):
        lens = [LONG_LEN] * N_LONG + [int(x) for x in rng.integers(40, 61, N_SHORT)]
        self.lens = lens
        self.doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        N = int(self.doc_ptr[-1])
        self.V = N_WORDS + len(lens)                                # the ballast words, then one word per document
        tokens, z0 = np.zeros(N, np.int32), np.zeros(N, np.int32)
        for d, L in enumerate(lens):
            b = int(self.doc_ptr[d])
            if d < N_LONG:
                own = [int(k) for k in rng.permutation(K - 1)[:OWN_LONG]]
                if d % 2:                                           # topic 0 heads the word's list: "zero first" wants its token in front
                    own = [0] + [k for k in own if k != 0][:OWN_LONG - 1]
                rest = [int(k) for k in rng.integers(0, K - 1, L - OWN_LONG)]
            else:                                                   # the own word's lowest topic holds one token of it: a zero entry heads its list
                pool = sorted(int(k) for k in rng.permutation(K - 1)[:10])
                mine = sorted(pool[int(i)] for i in rng.permutation(10)[:int(rng.integers(3, 7))])
                own = [mine[0]] + [k for k in mine[1:] for _ in range(int(rng.integers(1, 7)))]
                rest = [pool[int(i)] for i in rng.integers(0, 10, L - len(own))]
            pairs = [(k, N_WORDS + d) for k in own] + [(k, int(rng.integers(0, N_WORDS))) for k in rest]
            order = rng.permutation(L)
            if d >= N_LONG or d % 2:                                # that token (pairs[0]) among the first four
                at = int(np.flatnonzero(order == 0)[0])
                order[[d % 4, at]] = order[[at, d % 4]]
            for i, j in enumerate(order):
                z0[b + i], tokens[b + i] = pairs[int(j)]
        assert N <= 3000 and not (z0 == SLACK).any()
        self.tokens, self.z0 = tokens, z0
        self.n_wk = np.zeros((self.V, K), np.int64)
        np.add.at(self.n_wk, (tokens.astype(np.int64), z0.astype(np.int64)), 1)
        self.n_k = self.n_wk.sum(axis=0)
        self.T = [int(x) for x in self.n_k]
        self.U = [float(x) for x in O.uniforms(SEED, ITERATION, PURPOSE_Z, 0, N)]
        self.bS = BETA * float(self.V)
        self.alpha = [float(x) for x in ALPHA]                      # alpha[SLACK] is the knob: read nowhere but in s0_sw()
        self.den0, _, self.sw = head(self.n_k, self.alpha, BETA, self.bS)
        self.s0_pre = _chain([(self.alpha[k] * BETA) / self.den0[k] for k in range(K - 1)])
        self.row_w = [self.n_wk[w].tolist() for w in range(self.V)]
        self.list_w = [[k for k in range(K) if r[k] > 0] for r in self.row_w]
        self.zdoc = [[int(k) for k in z0[self.doc_ptr[d]:self.doc_ptr[d + 1]]] for d in range(len(lens))]
        self.memo = [{} for _ in lens]
        self.rare = {"candidates": 0, "probes": 0, "Q walk past its last entry": 0, "R walk's K - 1 fallback": 0, "S walk reaches K": 0}

    def vector(self, a):
        v = ALPHA.copy()
        v[SLACK] = a
        return v

    def s0_sw(self, a, slip=None):
        """S0 (the k-order chain ends with SLACK's term) and the S walk's terms at alpha[SLACK] = a"""
        if slip == "s0_tree":
            s0 = _tree([(self.alpha[k] * BETA) / self.den0[k] for k in range(K - 1)] + [(a * BETA) / self.den0[SLACK]])
        else:
            s0 = self.s0_pre + (a * BETA) / self.den0[SLACK]
        return s0, self.sw[:SLACK] + [a / self.den0[SLACK]]

    def _masses(self, d, t, st, z0, slip=None):
        w = int(self.tokens[t])
        return masses(st.cnt, st.list, z0, self.row_w[w], self.list_w[w], self.T, self.den0, self.alpha, BETA, self.bS, slip)

    def run_doc(self, d, a, upto=None, slip=None, force=None, detail=None):
        """step() over the tokens 0 .. upto of document d (all of them without upto) at alpha[SLACK] = a: the list of (topic,
        bucket, index).  slip, force and detail act on the LAST of them only: the tokens in front are the unmutated draw.
        The masses of a token depend on the draws in front of it, not on a: kept per (document, those draws)."""
        b, zdoc, memo = int(self.doc_ptr[d]), self.zdoc[d], self.memo[d]
        n = len(zdoc) if upto is None else upto + 1
        s0, sw = self.s0_sw(a)
        key, out, st = (), [], None
        for pos in range(n):
            z0, last = zdoc[pos], pos == n - 1 and upto is not None
            m = memo.get(key)
            if m is None and st is None:                            # the document's state behind the draws so far
                st = _Doc(K, zdoc)
                for j in range(pos):
                    st.remove(zdoc[j])
                    st.add(key[j])
            if st is not None:
                st.remove(z0)
            if m is None:
                m = memo[key] = self._masses(d, b + pos, st, z0)
            try:
                if last and (slip or force or detail is not None):
                    if slip in MASS_SLIPS:
                        if st is None:
                            st = _Doc(K, zdoc)
                            for j in range(pos):
                                st.remove(zdoc[j])
                                st.add(key[j])
                            st.remove(z0)
                        m = self._masses(d, b + pos, st, z0, slip)
                    s0s = self.s0_sw(a, slip)[0] if slip == "s0_tree" else s0
                    o = draw(m, s0s, sw, BETA, self.U[b + pos], slip, force, detail)
                    if detail is not None:
                        detail["m"] = m
                else:
                    o = draw(m, s0, sw, BETA, self.U[b + pos])
            except InvalidTopic as ex:
                o = ex.args[1]
                self.raised = True
                if detail is not None and last:
                    detail.update(m=m, out=o, raised=True)
            if st is not None:
                st.add(o[0])
            out.append(o)
            key += (o[0],)
        return out

    def walk(self, a):
        """the builder's own z step over the whole corpus: (z, the four counters, whether a walk left its bucket)"""
        z, stats = np.zeros(self.z0.size, np.int32), [0, 0, 0, 0]
        self.raised = False
        for d in range(len(self.lens)):
            b, key = int(self.doc_ptr[d]), ()
            for pos, o in enumerate(self.run_doc(d, a)):
                m = self.memo[d][key]
                stats[o[1]] += 1
                stats[3] += len(m["list_w"]) + len(m["dlist"])
                z[b + pos] = o[0]
                key += (o[0],)
        return z, np.asarray(stats, np.int64), self.raised

    # ---- the search ----------------------------------------------------------------------------------------------------------
    def probe(self, d, p, a, slip=None, force=None):
        det = {}
        outs = self.run_doc(d, a, p, slip, force, det)
        return outs, det

    @staticmethod
    def boundaries(kind, where, m):
        """the entries i at which a stop of the row's walk is the lower side of the wanted flip, given the target's masses"""
        sc, nd = m["sc"], len(m["dlist"])
        n = len(sc)
        zero = [i for i in range(n) if sc[i] == 0.0]
        if kind in "ab":
            return [None]
        if kind == "c":
            ok = lambda i: 0 <= i and i + 1 < n and sc[i] > 0.0 and sc[i + 1] > 0.0      # noqa: E731
            if where == "0|1":
                return [0] if ok(0) else []
            if where == "63|64":
                return [63] if n > 64 and ok(63) else []
            if where == "last two":
                return [n - 2] if ok(n - 2) else []
            if where == "zero behind":
                return [i - 1 for i in zero if i >= 1 and i + 1 < n and sc[i - 1] > 0.0 and sc[i + 1] > 0.0][:1]
            if where == "zero first":
                return [1] if zero == [0] and n >= 3 else []
            return [i for i in range(0, 5) if ok(i)]
        if kind == "d":
            if where == "fallback":
                return [nd - 1] if nd >= 1 else []
            if where == "0|1":
                return [0] if nd >= 2 else []
            if where == "63|64":
                return [63] if nd > 64 else []
            if where == "last":
                return [nd - 2] if nd >= 3 else []
            return [i for i in range(0, 5) if i + 1 < nd]
        if where == "0|1":
            return [0]
        if where == "63|64":
            return [63]
        if where == "K-2|K-1":
            return [K - 2]
        return [0, 1, 2, 3, 4]

    @staticmethod
    def past(kind, i, out):
        """the row's comparison has fallen the upper way: (bucket, index) is monotone in the sample"""
        _, bucket, index = out
        if kind == "a":
            return bucket > BQ
        if kind == "b":
            return bucket > BR
        return (bucket, index) > ({"c": BQ, "d": BR, "e": BS}[kind], i)

    def useful(self, d, p, a, kind, i):
        """the comparison forced one way and the other moves the target's new topic"""
        return self.probe(d, p, a, force=(kind, i, False))[0][-1][0] != self.probe(d, p, a, force=(kind, i, True))[0][-1][0]

    def sides(self, det, kind, i):
        return det.get("sides", {}).get((kind, i))

    def aim(self, kind, where, d, p):
        """a row for the target at position p of document d, or None: the flip pair of adjacent bit patterns of alpha[SLACK]"""
        if (kind, where, d, p) not in self._aimed:
            self._aimed[(kind, where, d, p)] = self._aim(kind, where, d, p)
        return self._aimed[(kind, where, d, p)]

    def _aim(self, kind, where, d, p):
        _, det = self.probe(d, p, 1.0)
        for i in self.boundaries(kind, where, det["m"]):
            lo = _bisect(lambda a: self.past(kind, i, self.run_doc(d, a, p)[-1]), _bits(A_LO), _bits(A_HI))
            if lo is None:
                continue
            if kind in "ab" and self.searched:                      # the rare paths, next to the bucket's edge
                self.rare["candidates"] += 1
                for j in range(-WINDOW, WINDOW + 1):
                    dj = {}
                    o = self.run_doc(d, _dbl(lo + j), p, detail=dj)[-1]
                    self.rare["probes"] += 1
                    if dj.get("raised"):
                        self.rare["Q walk past its last entry" if o[1] == BQ else "S walk reaches K"] += 1
                    elif o[1] == BR and o[2] == len(dj["m"]["dlist"]):
                        self.rare["R walk's K - 1 fallback"] += 1
            pair = [self.probe(d, p, _dbl(lo + j)) for j in (0, 1)]
            (o0, d0), (o1, d1) = pair
            if bool(d0.get("raised")) != (where == "raise") or d1.get("raised") or o0[:-1] != o1[:-1] or o0[-1][0] == o1[-1][0]:
                continue                                            # the prefix moves within the pair, or the two topics are one
            falls = [o[-1][1] == BR and o[-1][2] == len(dd["m"]["dlist"]) for o, dd in pair]
            if falls != [False, where == "fallback"]:
                continue                                            # the R walk's fallback belongs to its own row
            if i not in self.boundaries(kind, where, d0["m"]):
                continue                                            # the structure the position names is not the flip's
            s0_, s1_ = self.sides(d0, kind, i), self.sides(d1, kind, i)
            if s0_ is None or s1_ is None or not (self.useful(d, p, _dbl(lo), kind, i) and self.useful(d, p, _dbl(lo + 1), kind, i)):
                continue
            row = Row()
            row.kind, row.where, row.doc, row.pos, row.beg, row.idx, row.lo = kind, where, d, p, int(self.doc_ptr[d]), i, lo
            row.target = row.beg + p
            row.tie = "tie" in (tag_of(*s0_), tag_of(*s1_))
            return row
        return None

    def moves(self, row, slip):
        """the slip, applied at the target alone, draws another topic at one of the row's two knob values"""
        return any(self.run_doc(row.doc, _dbl(row.lo + j), row.pos, slip)[-1][0] != self.run_doc(row.doc, _dbl(row.lo + j), row.pos)[-1][0] for j in (0, 1))

    def _search(self):
        self.rows, used, self._aimed = [], set(), {}
        self.tried = {}
        for need, (kind, where, tie, *shows) in enumerate(NEEDS):
            got = None
            spots = []
            early, late = (0, 1, 2, 3, 5, 8, 4, 6, 7) + tuple(range(9, 40)), (63, 64, 1, 62, 2, 65, 0, 3, 5, 8)
            for p in (early if tie or (kind, where) in RARE else late[need % 10:] + late[:need % 10] + early[9:]):
                for d in range(len(self.lens)):
                    dd = (d + 5 * need) % len(self.lens)            # the needs begin at different documents
                    if dd not in used and p < self.lens[dd] - 1 and (p < 62 or dd < N_LONG):
                        spots.append((dd, p))
            for d, p in spots:
                self.tried[(kind, where, tie) + tuple(shows)] = self.tried.get((kind, where, tie) + tuple(shows), 0) + 1
                row = self.aim(kind, where, d, p)
                if row is not None and (row.tie or not tie) and all(self.moves(row, s) for s in shows):
                    got = row
                    break
            assert got is not None, "no target takes the %s row at %s%s" % (kind, where, " with a tie" if tie else "")
            used.add(got.doc)
            self.rows.append(got)
        self._knobs()

    def _recorded(self, rec):
        self.rows, self._aimed, self.tried = [], {}, {}
        for kind, where, d, p, lo in rec["rows"]:
            row = self.aim(kind, where, d, p)
            assert row is not None and row.lo == lo, "the recorded %s row at %s (document %d, position %d) is not found again" % (kind, where, d, p)
            self.rows.append(row)
        self._knobs()

    def record(self):
        """what recorded() reads: the candidates the search took, their flips and the proposal rows' handle"""
        return {"rows": [[r.kind, r.where, r.doc, r.pos, r.lo] for r in self.rows], "base": self.base}

    def _knobs(self):
        self.knob = []
        for row in self.rows:
            row.own = (len(self.knob), len(self.knob) + 1)
            self.knob += [_dbl(row.lo), _dbl(row.lo + 1)]
        assert len(self.knob) <= MAX_HANDLES == 48

    def handles(self):
        return list(range(len(self.knob)))

    def knobs(self, h):
        """the alpha vector of handle h"""
        return self.vector(self.knob[h])

    # ---- the rows under every handle -------------------------------------------------------------------------------------------
    def at(self, row, h, slip=None, force=None):
        """(the new topic of the row's target at handle h, detail)"""
        outs, det = self.probe(row.doc, row.pos, self.knob[h], slip, force)
        return outs[-1][0], det

    def classify(self, row, h):
        """the row's tag at handle h, or None; "-" for a useful value off the edge (a flip partner)"""
        _, det = self.at(row, h)
        sd = self.sides(det, row.kind, row.idx)
        if sd is None or not self.useful(row.doc, row.pos, self.knob[h], row.kind, row.idx):
            return None
        return tag_of(*sd) or "-"

    def _settle(self):
        """row.tags and self.expect[h] = {token: topic} over every row's target and the tokens in front of it, at every
        handle; after the whole search also the builder's whole z step at every handle"""
        self.expect = {h: {} for h in self.handles()}
        self._walks, self.checked = {}, {}
        for row in self.rows:
            row.tags, row.prefix = {}, {}
            for h in self.handles():
                outs = self.run_doc(row.doc, self.knob[h], row.pos)
                self.expect[h].update((row.beg + i, o[0]) for i, o in enumerate(outs))
                t = self.classify(row, h)
                if t is not None and (t != "-" or h in row.own):
                    row.tags[h] = t
                    row.prefix[h] = [o[0] for o in outs[:-1]]
            lo, hi = row.own
            assert lo in row.tags and hi in row.tags, self.describe(row)
            assert row.prefix[lo] == row.prefix[hi], "%s: a token before the target moves within the flip pair" % self.describe(row)
            assert self.expect[lo][row.target] != self.expect[hi][row.target], self.describe(row)
            assert self.past(row.kind, row.idx, self.at(row, lo)[1]["out"]) != self.past(row.kind, row.idx, self.at(row, hi)[1]["out"])
        self.raises = {row.own[0] for row in self.rows if row.where == "raise"}
        if self.searched:                                           # no other token of the corpus leaves its bucket at any handle
            for h in self.handles():
                z, _, raised = self.walk_at(h)
                assert raised == (h in self.raises), h
                assert all(z[t] == k for t, k in self.expect[h].items())

    def walk_at(self, h):
        if h not in self._walks:
            self._walks[h] = self.walk(self.knob[h])
        return self._walks[h]

    def full_handles(self):
        """where the device test compares the whole z step: the first and the last handle, the proposal rows' and one per comparison"""
        hs = {self.handles()[0], self.handles()[-1], self.base}
        for kind in "abcde":
            own = [h for row in self.rows if row.kind == kind and (row.kind, row.where) not in RARE for h in row.own]
            if not hs & set(own):
                hs.add(own[1])
        return sorted(hs)

    def check_step(self, h):
        """The restatement's z step over the whole corpus at handle h, (z, the four counters): the targets and the tokens in
        front of them are where the rows were classified with them, and (after the whole search) every token lands where
        the builder's step() puts it, with the same counters."""
        z = self.z0.astype(np.int64)
        try:
            stats, raised = R.z_step(self.doc_ptr, self.tokens, z, self.n_wk, self.n_k, self.knobs(h), BETA, SEED, ITERATION), False
        except InvalidTopic:                                        # after the whole step, as the device reports it: z is complete
            stats, raised = None, True
        assert raised == (h in self.raises), "handle %d: the restatement %s" % (h, "raises" if raised else "does not raise")
        for t, k in self.expect[h].items():
            assert z[t] == k, "handle %d: token %d: the restatement draws %d, the builder %d" % (h, t, z[t], k)
        if self.searched:
            mine, mstats, _ = self.walk_at(h)
            bad = np.flatnonzero(z != mine)
            assert bad.size == 0, "handle %d: the restatement and the builder's step() differ at tokens %s" % (h, bad[:8])
            assert stats is None or [int(x) for x in stats] == [int(x) for x in mstats], "handle %d: the counters differ" % h
            stats = mstats
        return z.astype(np.int32), (None if stats is None else np.asarray(stats, np.int64))

    def restatement(self, h):
        if h not in self.checked:
            self.checked[h] = self.check_step(h)
        return self.checked[h]

    def describe(self, row):
        return "%s row at %s, entry %s, token %d (document %d, position %d of %d)" % (row.kind, row.where, row.idx, row.target, row.doc, row.pos,
                                                                                       self.lens[row.doc])

    def label(self, row, h):
        return (row.kind, row.where, row.tags.get(h, "-"))

    def survey(self):
        """counts[(comparison, position)]: rows with a flip pair; counts[(comparison, tag)]: rows reaching the tag;
        counts[(comparison, "tie at 0")]: tie rows of a walk at its first entry"""
        counts = {}
        for row in self.rows:
            keys = [(row.kind, row.where), (row.kind, "flip")] + [(row.kind, t) for t in set(row.tags.values()) - {"-"}]
            if row.idx == 0 and "tie" in row.tags.values():
                keys.append((row.kind, "tie at 0"))
            for k in keys:
                counts[k] = counts.get(k, 0) + 1
        return counts

    # ---- the proposal rows ---------------------------------------------------------------------------------------------------
    def _proposals(self, base=None):
        """self.proposals = {(bucket, entry): tokens} at ONE of the handles' vectors (self.base: the first handle whose z step
        holds every kind, else the one holding most), each token with its margins in exact arithmetic"""
        want = {(b, e) for b in "QR" for e in PROPOSAL_ENTRIES} | {("Q", "zero")}
        self.base, self.proposals = None, {}
        for h in (self.handles()[::2] if base is None else [base]):
            got = self._proposals_at(self.knob[h])
            if len(want & set(got)) > len(want & set(self.proposals)) or self.base is None:
                self.base, self.proposals = h, got
            if want <= set(got):
                break

    def _proposals_at(self, a):
        s0, _ = self.s0_sw(a)
        found = {}
        u = Fraction(1, 2 ** 53)
        for d in range(len(self.lens)):
            b, key = int(self.doc_ptr[d]), ()
            for pos, o in enumerate(self.run_doc(d, a)):
                m = self.memo[d][key]
                key += (o[0],)
                terms, e = (m["sc"], m["rt"], ())[o[1]], o[2]
                if e >= len(terms):
                    continue
                zero = o[1] == BQ and e > 0 and terms[e - 1] == 0.0   # equal neighbours: the replay's
                name = "last" if e == len(terms) - 1 else str(e)
                if not zero and (len(terms) <= 64 or name not in PROPOSAL_ENTRIES):
                    continue
                Rx, Qx = sum(map(Fraction, m["rt"])), sum(map(Fraction, m["sc"]))
                total = Fraction(s0 - m["x"] + m["y"]) + Rx + Qx
                delta4 = 4 * (8 * (len(m["sc"]) + len(m["dlist"])) + 64) * u * total
                start = Fraction(self.U[b + pos]) * total - (Qx if o[1] == BR else 0)
                pre = sum(map(Fraction, terms[:e]))
                sure = start - pre - Fraction(terms[e]) < -delta4 and (e == 0 or start - pre > delta4) and start - (Rx if o[1] == BR else Qx) < -delta4
                if o[1] == BR:
                    sure = sure and start > delta4
                if sure and zero:
                    found.setdefault(("Q", "zero"), []).append(b + pos)
                elif sure and len(terms) > 64 and name in PROPOSAL_ENTRIES:
                    found.setdefault(("QR"[o[1]], name), []).append(b + pos)
        return found


_cache = {}
ROWS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adlda_knife_edge_rows.json")


def recorded():
    with open(ROWS_PATH) as f:
        return json.load(f)


def edges(search=False):
    """the builder's result, built once per process: from the whole search, or from the recorded candidates
    (tests/test_adlda_knife_edge_model.py asserts that the two are the same rows and handles)"""
    if search not in _cache:
        _cache[search] = Edges() if search else Edges(rows=recorded())
    return _cache[search]


if __name__ == "__main__":                                          # python -m tests.adlda_knife_edge: the search's result into tests/golden
    O.build()
    with open(ROWS_PATH, "w") as f:
        json.dump(Edges().record(), f)
        f.write("\n")
