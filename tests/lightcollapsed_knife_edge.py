"""Knife-edge rows for the token step of scheme=lightcollapsed (a test helper, not collected; the manner and the
vocabulary of tests/lightpclda_knife_edge.py: Row, tags, `useful`, survey).

The token step (CollapsedLightLDA.java:925-1046, tests/lightcollapsed_restatement.token_step) makes seven comparisons:

  a  table or beta branch   u_w = U1 * (tpt + beta * K)            <  tpt                          knob beta
  b  table cell             frac = (u_w / tpt) * nnz - i           >  ps[w][i]   (list_w[a[i]] or list_w[i])   beta
  c  beta cell              (int)(((u_w - tpt) / (beta * K)) * K)  on either side of an integer m  beta
  d  word accept            U2 < pi_w, five quotients              knob alpha[z0], a topic the row owns
  e  length branch          ui = U3 * (len + alphaSum) < len       knob alphaSum, through a slack topic's alpha
  f  alpha cell             (int)(((ui - len) / alphaSum) * K)     on either side of an integer m  alphaSum
  g  document accept        U4 < pi_d, four quotients              knob alpha[s], a topic the row owns; s = z0 (state
                                                                   "A") or the accepted word proposal ("B", "B0")

Isolation.  There is no Phi.  Under the parallel schedule a token sees the sweep-start n_wk / n_k (fixed by z0), its
document's running histogram and z of its document.  A row is a document with one TARGET token whose word is the
document's own (word nK + d); further tokens of that word lie only BEHIND the target in the same document, where they
shape the word's count row (hence its table and G) without being sampled before it.  The tokens before the target carry
filler words (word k sits on topic k; the small topics 2 .. 35 hold 30 to 300 tokens -- 20 to 200 in BetaEdges -- in
sizes announced before the rows are planned and made exact by ballast documents at the end, the big ones 36 .. 39
hold thousands): such a token keeps its topic unless a uniform
of 10^-4 says otherwise, and what it does is predicted by the builder's own step() anyway.  The builder asserts through
the restatement that under every knob value a row is tagged at, the tokens before its target land on the topics the
row was classified with, and that the restatement draws at EVERY token what step() predicts.

Knobs.  Counts are integers and the uniforms are fixed by (seed, iteration, global token index); what moves is alpha
(per topic) and beta, both fixed at ggs_create: every knob value is a handle.
  AlphaEdges  d, e, f, g: N_VECTORS alpha vectors over K = 250 topics (40 K-side, a pool of topics to own, the slack topic).
              A d or g row owns a topic s_r that only its document uses (table-drawn d rows and alpha-branch g rows own
              a second one, the proposal's); alpha[s_r] is solved per tag (alpha +- 4096 ulps and the half-ulp grid of
              the sums), and vector v carries tag TAGS[v % 3].  The d rows take their word proposal from the table
              or from the beta branch (there ni[t] = 0 and pi_w moves in alpha's own steps, which reaches more of
              the three tags).  e and f rows move alphaSum through the slack topic (the last one): one row per three vectors.
              alphaSum also decides a g row's document proposal, so a g row is aimed under the alphaSum of ONE triple
              of vectors and counts there; a d row counts under every vector.
              f: the integers m = 249 (last), 3, 96 and 80.  ((ui - len) / alphaSum) * K moves in steps of K * ulp(x);
              for m = 1 that is 0.98 ulp(1.0) while pred(1.0) lies HALF an ulp(1.0) below 1.0, and none of the 110
              candidate documents has a target that reaches pred(1), 1 and succ(1) within 4096 ulps of alphaSum: no row
              aims there, the first aimed cell is m = 3.  (K = 250 is chosen for it: its mantissa 1.95 exceeds that of
              3, 80, 96 and 249, so the steps are finer than the doubles at those m; at a power of two m the double
              below is again half a step away.)
  BetaEdges   a, b, c: K = 100, one aimed row per beta value.  c: m = 1, 48 and 99, all three tags each (at K = 100 the
              steps at m = 1 are 0.78 ulp(1.0) and a target reaching pred(1) exists).  b: ups moves with beta, ps hardly
              (it moves by the rounding of p / mass); frac = ups - i is a multiple of ulp(ups).  In cell 0 frac has
              ps's grid and all three tags are reached (three rows); for i >= 1 frac's grid is at least twice as coarse
              as ps's, so for a given ps either the tie or the two neighbours exist, not both: two rows in cell 1 (one
              on a list of more than 64 entries) take what their ps allows, chosen so that the fused fraction (which is
              another double only behind cell 0) moves them, plus an untagged value on the other side as the flip pair
              where needed.  No row aims at a cell i >= 2: there a tie needs ps on a grid four and more times its own.
              The lists hold pool topics only or start behind topic 0, so i indexes the list and not the topic; nnz is
              3, 5, 6, 7 or above 64, no power of two (u_w * nnz / tpt would round as (u_w / tpt) * nnz does).
g rows come per source of the document proposal (SOURCES of the lightpclda builder: "alpha", "old", "chunk" -- the
register path, "earlier" -- gathered from memory) and per state: "A" the word proposal was not accepted or there was
none; "B" accepted; "B0" accepted and the document proposal is z0 (the t_is_z0 arm).

Tags as in the other builders; a (row, knob value) counts only where forcing the comparison both ways gives two
different new topics (`useful`), and a row only with a flip pair.

step() is the builder's own arithmetic in plain Python floats, written apart from the restatement, with `force` and the
switchable SLIPS -- each a plausible rewrite of the kernel."""
from fractions import Fraction

import numpy as np

from tests import lightcollapsed_restatement as R
from tests import lightpclda_knife_edge as PK
from tests.lightpclda_knife_edge import MAX_HANDLES, OUT_OF_BOUNDS, SOURCES, TAGS, Row, _bisect, _bits, _dbl, _next, dt_source, tag_of  # noqa: F401

K = 40                                                              # the K-side topics: 0, 1 kept small, 2 .. 39 the fillers'
ALPHA = np.resize(np.array([0.1, 0.12, 0.08, 0.1, 0.15, 0.1, 0.09, 0.11]), K)
BETA = 0.01
SEED = 4242
ITERATION = 1
STATES = ("A", "B", "B0")
MIN_PER_CATEGORY = 8                                                # d, g: rows per (comparison, tag)
MIN_PER_SOURCE = 4                                                  # g: rows per (dt source, state)
MIN_GLOBAL_ROWS = 3                                                 # a, b, c, e, f: rows per tag (each costs a handle)
N_VECTORS = 24
WINDOW = 4096
FILL = tuple(range(2, K - 4))                                       # the small fillers: topic k holds exactly target(k) tokens of word k
BIG = tuple(range(K - 4, K))                                        # the big ones: where every other token starts

# slip -> the comparison it belongs to
SLIPS = {"cancel_G": "d", "cancel_T": "d", "assoc": "d", "word_le": "d", "alpha_t": "d",
         "doc_assoc": "g", "doc_le": "g", "stale_z0": "g", "alpha_z0": "g",
         "branch_le": "a", "alias_ge": "b", "ups_mul_first": "b", "fused_frac": "b", "cell_mul_first": "c",
         "len_le": "e", "alpha_cell_mul_first": "f"}
INDEX_SLIPS = ("alpha_z0", "alpha_t", "stale_z0")                   # may show on random data
ORDER_SLIPS = tuple(s for s in SLIPS if s not in INDEX_SLIPS)       # must not


def pi_word(a, a_t, b, bS, ni_t, ni_s, Gt, Gs, Tt, Ts, slip=None):
    q1 = ((a_t if slip == "alpha_t" else a) + float(ni_t)) / (a + float(ni_s))
    r2 = (b + float(Gt)) / (b + (float(Gs) - 1.0))
    r3 = (bS + (float(Ts) - 1.0)) / (bS + float(Tt))
    r4 = (b + float(Gs)) / (b + float(Gt))
    r5 = (bS + float(Tt)) / (bS + float(Ts))
    if slip == "cancel_G":
        return q1 * ((b + float(Gs)) / (b + (float(Gs) - 1.0))) * r3 * r5
    if slip == "cancel_T":
        return q1 * r2 * ((bS + (float(Ts) - 1.0)) / (bS + float(Ts))) * r4
    if slip == "assoc":
        return q1 * (r2 * r3) * r4 * r5
    return q1 * r2 * r3 * r4 * r5


def pi_doc(a, b, bS, ni_t, ni_s, n_t, n_s, Gt, Gs, Tt, Ts, slip=None):
    q1 = (a + float(ni_t)) / (a + float(ni_s))
    q2 = (b + float(Gt)) / (b + (float(Gs) - 1.0))
    q3 = (bS + (float(Ts) - 1.0)) / (bS + float(Tt))
    q4 = (a + float(n_s)) / (a + float(n_t))
    if slip == "doc_assoc":
        return q1 * (q2 * q3) * q4
    return q1 * q2 * q3 * q4


def step(n, zdoc, pos, G, T, alpha, alpha_total, beta, V, table, U, slip=None, force=None, detail=None):
    """The new topic of the token at pos; n (the document's histogram, the token counted), zdoc, G (the word's
    sweep-start row) and T (the sweep-start totals) are left alone.  table = (ps_w, a_w, list_w, nnz, tokensPerType).
    slip: one of SLIPS.  force = (comparison, outcome): "branch" / "alias" / "word" / "len" / "doc" with a bool, "bcell" /
    "cell" with the beta- / alpha-branch topic."""
    nK = len(n)
    fK = float(nK)
    U1, U2, U3, U4 = U
    fname, fval = force if force is not None else (None, None)
    ps_w, a_w, list_w, nnz, tpt = table
    bS, bK, ftpt = beta * float(V), beta * fK, float(tpt)
    z0 = s = int(zdoc[pos])
    u_w = U1 * (ftpt + bK)
    tb = u_w <= ftpt if slip == "branch_le" else u_w < ftpt
    if fname == "branch":
        tb = fval
    cell = frac = psv = up = v = None
    if tb:
        ups = u_w * float(nnz) / ftpt if slip == "ups_mul_first" else (u_w / ftpt) * float(nnz)
        cell = int(ups)
        if cell >= nnz:
            if fname != "branch" and slip is None:
                raise R.InvalidTopic("table draw reaches nnz")
            cell = nnz - 1                                          # as the kernel clamps
        frac = float(Fraction(u_w / ftpt) * nnz - cell) if slip == "fused_frac" else ups - float(cell)
        psv = float(ps_w[cell])
        up = frac >= psv if slip == "alias_ge" else frac > psv
        if fname == "alias":
            up = fval
        wp = int(list_w[int(a_w[cell])]) if up else int(list_w[cell])
    else:
        v = (u_w - ftpt) * fK / bK if slip == "cell_mul_first" else ((u_w - ftpt) / bK) * fK
        wp = int(v)
        if fname == "bcell":
            wp = fval
        if fname == "branch":
            wp = min(max(wp, 0), nK - 1)
        if wp >= nK:
            raise R.InvalidTopic("beta branch reaches K")
    flen = float(len(zdoc))
    ui = U3 * (flen + alpha_total)
    inside = ui <= flen if slip == "len_le" else ui < flen
    if fname == "len":
        inside = fval
    idx = av = None
    if inside:
        idx = min(int(ui), len(zdoc) - 1) if fname == "len" else int(ui)
        if idx >= len(zdoc):
            return OUT_OF_BOUNDS
        dt = int(zdoc[idx])
    else:
        av = (ui - flen) * fK / alpha_total if slip == "alpha_cell_mul_first" else ((ui - flen) / alpha_total) * fK
        dt = int(av)
        if fname == "cell":
            dt = fval
        dt = max(dt, 0) if fname == "len" else dt
        if dt >= nK:
            raise R.InvalidTopic("alpha branch reaches K")
    cnt = list(n)
    pi_w = pi_d = w_args = d_args = None
    acc_w = acc_d = False
    if wp != s:
        w_args = (float(alpha[wp]), beta, bS, cnt[wp], cnt[s] - 1, G[wp], G[s], T[wp], T[s])
        pi_w = pi_word(float(alpha[s]), *w_args, slip=slip)
        acc_w = pi_w > 1.0 or (U2 <= pi_w if slip == "word_le" else U2 < pi_w)
        if fname == "word":
            acc_w = fval
        if acc_w:
            cnt[s] -= 1
            cnt[wp] += 1
            s = wp
    new = z0
    if dt != s:
        moved = 1 if s != z0 else 0                                 # G and T are the sweep-start counts with the token moved
        back = 1 if (moved and dt == z0 and slip != "stale_z0") else 0
        d_args = (beta, bS, cnt[dt], cnt[s] - 1, cnt[dt], cnt[s], G[dt] - back, G[s] + moved, T[dt] - back, T[s] + moved)
        pi_d = pi_doc(float(alpha[z0] if slip == "alpha_z0" else alpha[s]), *d_args, slip=slip)
        acc_d = pi_d > 1.0 or (U4 <= pi_d if slip == "doc_le" else U4 < pi_d)
        if fname == "doc":
            acc_d = fval
        new = dt if acc_d else s
    if detail is not None:
        detail.update(u_w=u_w, tb=tb, cell=cell, frac=frac, ps=psv, up=up, v=v, word=wp, pi_w=pi_w, w_args=w_args, acc_w=acc_w, ui=ui,
                      inside=inside, idx=idx, av=av, doc=dt, s=s, pi_d=pi_d, d_args=d_args, acc_d=acc_d, new=new,
                      state="A" if not acc_w else "B0" if dt == z0 else "B")
    return new


def z_step(doc_ptr, tokens, z, n_wk, n_k, alpha, beta, tables, U, slip=None):
    """R.z_step's parallel schedule with step(): one z step in place on z; returns how many tokens left the array's
    bounds (a slip can).  U[t] = the uniforms of global token t."""
    ps, a, _, nw, lists, tpt = tables
    V, nK = n_wk.shape
    alpha = [float(x) for x in np.broadcast_to(np.asarray(alpha, np.float64), (nK,))]
    total = R.alpha_sum(alpha, nK)
    T = [int(x) for x in n_k]
    rows, out = {}, 0
    for d in range(len(doc_ptr) - 1):
        b, e = int(doc_ptr[d]), int(doc_ptr[d + 1])
        zdoc = [int(k) for k in z[b:e]]
        n = [0] * nK
        for k in zdoc:
            n[k] += 1
        for pos in range(e - b):
            w = int(tokens[b + pos])
            if w not in rows:
                rows[w] = (n_wk[w].tolist(), (ps[w], a[w], lists[w], int(nw[w]), int(tpt[w])))
            new = step(n, zdoc, pos, rows[w][0], T, alpha, total, beta, V, rows[w][1], U[b + pos], slip)
            if new == OUT_OF_BOUNDS:
                out += 1
                continue
            n[zdoc[pos]] -= 1
            n[new] += 1
            zdoc[pos] = new
        z[b:e] = zdoc
    return out


class _Edges:
    """What both builders share: the corpus, the trial evaluation of a planned document, the checks."""
    FORCES = {"a": "branch", "b": "alias", "d": "word", "e": "len", "g": "doc"}

    def _layout(self, lens, rng):
        self.lens = [int(x) for x in lens]
        self.doc_ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
        N = int(self.doc_ptr[-1])
        self.V = self.nK + len(lens)
        if not hasattr(self, "U"):
            self.U = [R.token_uniforms(SEED, ITERATION, t) for t in range(N)]
        self.z0 = np.asarray(BIG)[rng.integers(0, 4, N)].astype(np.int32)
        self.tokens = self.z0.copy()                                # a filler's word is its topic
        self.target = {k: int(self.TSCALE * 10.0 ** (i / (len(FILL) - 1.0))) for i, k in enumerate(FILL)}
        self.T_est = [0, 0] + [self.target[k] for k in FILL] + [N // 4] * 4 + [0] * (self.nK - K)
        self.rows, self.row_of = [], {}

    def _ballast(self, first):
        """the documents from `first` on bring every small filler topic to its announced size: what the rows were planned with"""
        at = int(self.doc_ptr[first])
        for k in FILL:
            need = self.target[k] - int((self.z0 == k).sum())
            assert 0 <= need <= self.z0.size - at, (k, need)
            self.z0[at:at + need] = self.tokens[at:at + need] = k
            at += need

    def _put(self, d, topics, words):
        for k in set(topics):                                       # a small filler topic is never planned past its announced size
            assert k not in self.target or int((self.z0 == k).sum()) + topics.count(k) <= self.target[k], (d, k)
        b = int(self.doc_ptr[d])
        self.z0[b:b + len(topics)] = topics
        self.tokens[b:b + len(topics)] = words

    def _row(self, d, pos, kind):
        row = Row()
        row.kind, row.doc, row.beg, row.pos = kind, d, int(self.doc_ptr[d]), pos
        row.target = row.beg + pos
        row.word = self.nK + d
        row.U = self.U[row.target]
        row.tags = {}
        self.rows.append(row)
        self.row_of[d] = row
        return row

    def trial(self, topics, words, d, pos, alpha, total, beta, force=None, slip=None):
        """step() at the target of a PLANNED document over the estimated totals: (new, detail)"""
        nK, W = self.nK, self.nK + d
        T = list(self.T_est)
        for k in set(topics):
            if k >= K or k < 2:                                     # a topic of the row's own, or a shared small one
                T[k] = topics.count(k)
        G = [0] * nK
        for k, w in zip(topics, words):
            if w == W:
                G[k] += 1
        lst, ps, a, _, tot = R.word_table(G, T, beta * float(self.V))
        det = {}
        try:
            new = step(np.bincount(topics, minlength=nK).tolist(), topics, pos, G, T, alpha, total, beta, self.V, (ps, a, lst, len(lst), tot),
                       self.U[int(self.doc_ptr[d]) + pos], slip, force, det)
        except R.InvalidTopic:
            return None, det
        return new, det

    # ---- after the corpus is final ------------------------------------------------------------------------------
    def _count(self):
        self.n_wk, self.n_k = R.count(self.tokens, self.z0, self.V, self.nK)
        self.T = [int(x) for x in self.n_k]
        self._tab, self._built = {}, {}

    def built(self, beta):
        if beta not in self._built:
            self._built[beta] = R.build_tables(self.n_wk, self.n_k, beta)
        return self._built[beta]

    def table(self, w, beta):
        if (w, beta) not in self._tab:
            lst, ps, a, _, tot = R.word_table(self.n_wk[w].tolist(), self.T, beta * float(self.V))
            self._tab[(w, beta)] = (ps, a, lst, len(lst), tot)
        return self._tab[(w, beta)]

    def walk(self, alpha, beta):
        """the builder's own z step over the whole corpus"""
        z = self.z0.astype(np.int64)
        assert z_step(self.doc_ptr, self.tokens, z, self.n_wk, self.n_k, alpha, beta, self.built(beta), self.U) == 0
        return z

    def state(self, row, z):
        """(n, zdoc) at the row's target, given the z step's result z: new topics before it, old ones from it on"""
        e = int(self.doc_ptr[row.doc + 1])
        zdoc = [int(k) for k in z[row.beg:row.target]] + [int(k) for k in self.z0[row.target:e]]
        return np.bincount(zdoc, minlength=self.nK).tolist(), zdoc

    def eval(self, row, st, alpha, total, beta, slip=None, force=None):
        det = {}
        try:
            new = step(st[0], st[1], row.pos, self.n_wk[row.word].tolist(), self.T, alpha, total, beta, self.V, self.table(row.word, beta), row.U,
                       slip, force, det)
        except R.InvalidTopic:
            new = None
        return new, det

    def at(self, row, h, slip=None, force=None):
        """the new topic of the row's target at handle h"""
        alpha, total, beta = self.knobs(h)
        return self.eval(row, self.state(row, self.walks[h]), alpha, total, beta, slip, force)

    def both_sides(self, row):
        if row.kind == "c":
            return [("bcell", row.m - 1), ("bcell", row.m)]
        if row.kind == "f":
            return [("cell", row.m - 1), ("cell", row.m)]
        return [(self.FORCES[row.kind], False), (self.FORCES[row.kind], True)]

    def useful(self, row, ev):
        """the row's comparison forced one way and the other moves the target's new topic; ev(force) -> (new, detail)"""
        one, two = self.both_sides(row)
        return ev(one)[0] != ev(two)[0]

    def sides(self, row, det):
        """(the computed side, the uniform or bound) of the row's comparison, or None where the step did not make it"""
        k = row.kind
        if k == "a":
            return det["u_w"], float(row.tpt)
        if k == "b":
            return (det["frac"], det["ps"]) if det["cell"] == row.cell else None
        if k == "c":
            return (det["v"], float(row.m)) if det["v"] is not None else None
        if k == "d":
            return (det["pi_w"], row.U[1]) if det["pi_w"] is not None and det["word"] == row.t else None
        if k == "e":
            return det["ui"], float(self.lens[row.doc])
        if k == "f":
            return (det["av"], float(row.m)) if det["av"] is not None else None
        if k == "g":
            return (det["pi_d"], row.U[3]) if det["pi_d"] is not None and (det["s"], det["doc"], det["state"]) == (row.s, row.dt, row.state) else None
        return None

    def outcome(self, row, det):
        return {"a": det["tb"], "b": (det["cell"], det["up"]), "c": det["word"], "d": det["acc_w"], "e": det["inside"], "f": det["doc"],
                "g": det["acc_d"]}[row.kind]

    def knobs(self, h):
        raise NotImplementedError

    def classify(self, row, h):
        """the row's tag at handle h, or None; "-" for a useful value off the edge (a flip partner)"""
        alpha, total, beta = self.knobs(h)
        st = self.state(row, self.walks[h])
        ev = lambda force=None: self.eval(row, st, alpha, total, beta, force=force)     # noqa: E731
        _, det = ev()
        sd = self.sides(row, det) if det else None
        if sd is None or not self.useful(row, ev):
            return None, None
        return tag_of(*sd) or "-", self.outcome(row, det)

    def check_step(self, h):
        """The restatement's z step over the whole corpus at handle h: every token lands where step() says, and the
        tokens before the target of every row tagged at h are on the topics the row was classified with.  Returns (z,
        the three counters)."""
        alpha, total, beta = self.knobs(h)
        assert R.alpha_sum(alpha, self.nK) == total
        z = self.z0.astype(np.int64)
        stats = R.z_step(self.doc_ptr, self.tokens, z, self.n_wk, self.n_k, alpha, beta, self.built(beta), SEED, ITERATION)
        bad = np.flatnonzero(z != self.walks[h])
        assert bad.size == 0, "handle %s: the restatement and the builder's step() differ at tokens %s" % (h, bad[:8])
        for row in self.rows:
            if h in row.tags:
                assert [int(k) for k in z[row.beg:row.target]] == row.prefix[h], "handle %s: %s: a token before the target moved" % (h, self.describe(row))
        return z.astype(np.int32), np.asarray(stats, np.int64)

    def restatement(self, h):
        if h not in self.checked:
            self.checked[h] = self.check_step(h)
        return self.checked[h]

    def describe(self, row):
        return "%s row, token %d (document %d, position %d of %d)" % (row.kind, row.target, row.doc, row.pos, self.lens[row.doc])

    def label(self, row, h):
        return (row.kind, row.tags.get(h, "-"), "%s/%s" % (row.source, row.state) if row.kind == "g" else "-")

    def survey(self):
        """counts[(comparison, tag)] and, for g, counts[("g", source, state)]: rows, not (row, knob value) pairs"""
        counts = {}
        for row in self.rows:
            have = set(row.tags.values()) - {"-"}
            for t in have:
                counts[(row.kind, t)] = counts.get((row.kind, t), 0) + 1
            if row.kind == "g" and have:
                counts[("g", row.source, row.state)] = counts.get(("g", row.source, row.state), 0) + 1
        return counts

    def _settle(self, pairs):
        """row.tags from the walks; a row without a flip pair among its useful values is a plain row"""
        for row in self.rows:
            if row.kind == "plain":
                continue
            outs = set()
            for h in pairs(row):
                t, out = self.classify(row, h)
                if t is not None:
                    row.tags[h] = t
                    outs.add(out)
            if len(outs) < 2 or not (set(row.tags.values()) - {"-"}):
                row.kind, row.tags = "plain", {}
            else:                                                   # the scan of one edge: the same alphaSum (a triple) or the row's betas
                row.prefix = {h: [int(k) for k in self.walks[h][row.beg:row.target]] for h in row.tags}
                for h in row.tags:
                    same = [g for g in row.tags if self.scan_of(g) == self.scan_of(h)]
                    assert all(row.prefix[g] == row.prefix[h] for g in same), "%s: a token before the target moves within a scan" % self.describe(row)

    def scan_of(self, h):
        return 0


def _scan(f, bound, lo, grids=()):
    """{tag: the knob values x nearest the flip first with f(x) == pred(bound), bound, succ(bound)} over the doubles within WINDOW
    of bit pattern lo and, per grid step h, over _dbl(lo) + j * h; f takes an array (its operations are IEEE per element)"""
    js = np.array(sorted(range(-WINDOW, WINDOW + 1), key=abs), np.int64)
    xs = (js + lo).view(np.float64)
    for h in grids:
        xs = np.concatenate((xs, _dbl(lo) + np.array(sorted(range(-512, 513), key=abs), np.float64) * h))
    v = f(xs)
    want = {"below": _next(bound, False), "tie": bound, "above": _next(bound, True)}
    return {t: xs[v == w] for t, w in want.items() if (v == w).any()}


def solve(pi, U, lo_bits, hi_bits, grids=()):
    """{tag: knob} for pi(knob) == pred(U), U, succ(U) around the flip of U < pi(knob), and the flip's knob; None without a flip"""
    lo = _bisect(lambda x: U < pi(x), lo_bits, hi_bits)
    if lo is None:
        return None
    centre = _dbl(lo)
    found = {t: float(xs[0]) for t, xs in _scan(pi, U, lo, [float(np.spacing(centre + g)) / 2.0 for g in grids]).items()}
    return centre, found


class AlphaEdges(_Edges):
    """d, e, f and g rows: one beta, N_VECTORS alpha vectors."""
    TSCALE, N_BALLAST = 30, 45
    N_D, N_E, N_F = 32, 40, 110                                     # d rows; e and f candidates
    N_PER = {"alpha": 14, "old": 10, "chunk": 7, "earlier": 14}      # g: documents per state, by the source they are to take
    N_G = 3 * sum(N_PER.values())
    # K-side topics, a pool of topics to own, the slack topic.  250 = 1.95 * 2^7: ((ui - len) / alphaSum) * nK moves in steps
    # finer than the doubles at m wherever m's mantissa is below 1.95, so pred(m), m and succ(m) are all reached there
    nK = 250
    SLACK = nK - 1
    # f: the integer m between cells m - 1 and m, in order of preference: last, first (m = 1: see the module's docstring),
    # two middle ones
    CELLS = (nK - 1, 3, 96, 80, 100, 72, 48)
    A_LO, A_HI, A_POOL = 0.02, 0.5, 0.04                            # an owned alpha's range; an unowned pool topic's alpha
    FLOOR, CEIL = 40.0, 90.0                                        # alphaSum of every vector lies between

    def __init__(self, seed=3):
        self._plan(np.random.default_rng(seed))
        self._count()
        self._solve()

    # ---- the plan: documents, positions, structure ---------------------------------------------------------------
    def _plan(self, rng):
        nK = self.nK
        plan = [(src, st) for src in SOURCES for st in STATES for _ in range(self.N_PER[src])]
        glen = {"alpha": (12, 25), "old": (30, 51), "chunk": (69, 77), "earlier": (69, 100)}
        lens = np.concatenate(([int(rng.integers(*glen[src])) for src, _ in plan], rng.integers(10, 17, self.N_D), rng.integers(4, 13, self.N_E),
                               rng.integers(6, 61, self.N_F), np.full(self.N_BALLAST, 100)))
        lens[self.N_G - 6:self.N_G] = 131
        c0 = 3 * (self.N_PER["alpha"] + self.N_PER["old"])          # and two per state of the chunk source: the second chunk's register path
        for i in range(3):
            lens[c0 + (i + 1) * self.N_PER["chunk"] - 2:c0 + (i + 1) * self.N_PER["chunk"]] = 131
        self._layout(lens, rng)
        self.base = np.full(nK, self.A_POOL)
        self.base[:K] = ALPHA
        self.free = [k for k in range(K, nK - 1) if not any(k in (m - 1, m) for m in self.CELLS)]
        # e and f rows first: they fix alphaSum per triple of vectors
        self.aimed, self.sums = [], []
        d0 = self.N_G + self.N_D
        cands = {"e": list(range(d0, d0 + self.N_E)), "f": list(range(d0 + self.N_E, d0 + self.N_E + self.N_F))}
        for q in range(4):
            got = None
            while got is None:
                assert cands["e"], "too few candidates for e rows"
                d = cands["e"].pop(0)
                got = self._aim_ef("e", d, self.lens[d], rng, 0)
            self.aimed.append(got[0])
            self.sums.append(got[1])
        self.cells = []
        for m in self.CELLS:                                        # in order of preference, until four rows stand
            for d in cands["f"]:
                got = self._aim_ef("f", d, self.lens[d], rng, m)
                if got is not None:
                    cands["f"].remove(d)
                    self.cells.append(m)
                    self.aimed.append(got[0])
                    self.sums.append(got[1])
                    break
            if len(self.cells) == 4:
                break
        assert 3 * len(self.aimed) == N_VECTORS <= MAX_HANDLES
        for d, (src, st) in enumerate(plan):                        # g rows, the triple to begin with in turn
            self._plan_g(d, self.lens[d], src, st, d % 8, rng)
        for j in range(self.N_D):
            self._plan_d(self.N_G + j, self.lens[self.N_G + j], rng)
        self._ballast(len(lens) - self.N_BALLAST)

    def _claim(self, k=None):
        if k is None:
            return self.free.pop(0)
        self.free.remove(k)
        return k

    def _aim_ef(self, kind, d, L, rng, m):
        """A target whose U3 puts ui on len (e) or the alpha-branch cell on m (f) at an alphaSum between FLOOR and CEIL; the
        alphaSum per tag, or None."""
        nK, fL = self.nK, float(L)
        for pos in range(L - 1):                                    # not the last token: e's index branch reads z[len - 1]
            U3 = self.U[int(self.doc_ptr[d]) + pos][2]
            A0 = fL * (1.0 - U3) / U3 if kind == "e" else (fL * (1.0 - U3) / (U3 - m / float(nK)) if U3 > m / float(nK) else -1.0)
            if not self.FLOOR < A0 <= self.CEIL:
                continue
            if kind == "e":
                val, bound = (lambda A: U3 * (fL + A)), fL
            else:
                val, bound = (lambda A: ((U3 * (fL + A) - fL) / A) * float(nK)), float(m)
            lo = _bisect(lambda A: val(A) < bound, _bits(A0 * 0.999), _bits(A0 * 1.001))
            if lo is None:
                continue
            sums = {t: [float(x) for x in xs[:6]] for t, xs in _scan(val, bound, lo).items()}
            if len(sums) < 3:
                continue
            # the target on the largest topic, alone with its word: the proposals of the two sides go to small topics
            topics = [int(k) for k in np.asarray(BIG)[rng.integers(0, 3, L)]]   # (the target alone on the last big topic)
            topics[pos] = BIG[3]
            if kind == "e":
                topics[L - 1] = 1
            words = list(topics)
            words[pos] = nK + d
            alpha = self.base.tolist()
            A = sums["tie"][0]
            one, two = ([("len", False), ("len", True)] if kind == "e" else [("cell", m - 1), ("cell", m)])
            if self.trial(topics, words, d, pos, alpha, A, BETA, one)[0] == self.trial(topics, words, d, pos, alpha, A, BETA, two)[0]:
                continue
            self._put(d, topics, words)
            row = self._row(d, pos, kind)
            row.m = m
            return row, sums
        return None

    def _plan_g(self, d, L, src, state, q, rng):
        beg, nK = int(self.doc_ptr[d]), self.nK
        q0 = q
        first = {"chunk": (63, 127), "earlier": (64, 127)}.get(src, (0,))      # a chunk's last lane and its first, in both chunks
        order = [p for p in first[::1 - 2 * (d % 2)] if p < L] * 40 + list(rng.permutation(L) if L < 60 else 40 + rng.permutation(L - 40))
        if len(self.free) < 3:
            self._row(d, 0, "plain")
            return
        s_r = self.free[0]
        alo, ahi = self.base.tolist(), self.base.tolist()
        alo[s_r], ahi[s_r] = self.A_LO * 1.5, self.A_HI * 0.8
        for trial in range(60 * len(order)):
            p = int(order[trial % len(order)])
            q = (q0 + trial // len(order)) % 8                      # the triple whose alphaSum the row is aimed under
            A = self.sums[q]["tie"][0]
            U = self.U[beg + p]
            if not 0.03 <= U[3] <= 0.97:
                continue
            ui = U[2] * (float(L) + A)
            idx = int(ui) if ui < float(L) else None
            if dt_source(idx, p) != src:
                continue
            cell = None if idx is not None else int(((ui - float(L)) / A) * nK)
            if cell is not None and not (2 <= cell < K or cell in self.free[1:]):
                continue
            zt, dtk = [int(k) for k in np.asarray(FILL)[rng.permutation(len(FILL) if state == "A" else 12)[:2]]]      # (q3 is small after a move)
            g_s = int(rng.integers(0, 3)) if state == "A" else int(rng.integers(1, 5))
            x_s, g_t, x_t = int(rng.integers(0, 2)), int(rng.integers(0, 5)), int(rng.integers(0, 3))
            z0 = s_r if state == "A" else zt
            dt = z0 if state == "B0" else dtk
            if cell is not None:
                dt = cell
                z0 = cell if state == "B0" else z0
            if idx == p and state != "B0" or dt == z0 and state != "B0":
                continue
            W = nK + d
            need = [(s_r, W)] * g_s + [(s_r, s_r)] * x_s + [(dt, W)] * g_t + [(dt, dt)] * x_t
            nsuf = L - p - 1
            fixed = idx is not None and idx > p
            if len(need) + fixed > nsuf:
                continue
            suffix = need + [(int(k), int(k)) for k in self.z0[beg + p + 1 + len(need) + fixed:beg + L]]
            suffix = [suffix[i] for i in rng.permutation(len(suffix))]
            if fixed:
                suffix.insert(idx - p - 1, (dt, dt))
            topics = [int(k) for k in self.z0[beg:beg + p]] + [z0] + [k for k, _ in suffix]
            words = list(topics[:p]) + [W] + [w for _, w in suffix]
            if idx is not None and idx < p:
                topics[idx] = words[idx] = dt
            if any(topics[i] == z0 for i in range(p)) and state == "A":
                continue
            ok = True
            for al, sign in ((alo, 1.0), (ahi, -1.0)):              # pi_d falls as alpha[s] grows
                _, det = self.trial(topics, words, d, p, al, A, BETA)
                if not det or det["pi_d"] is None or (det["s"], det["doc"], det["state"]) != (s_r, dt, state) or sign * (det["pi_d"] - U[3]) <= 0:
                    ok = False
                    break
            if not ok or any(int((self.z0 == k).sum()) + topics.count(k) > self.target[k] for k in set(topics) if k in self.target):
                continue
            self._claim(s_r)
            if cell is not None and cell >= K:
                self._claim(cell)
            self._put(d, topics, words)
            row = self._row(d, p, "g")
            row.s_r, row.s, row.dt, row.state, row.source, row.q = s_r, s_r, dt, state, src, q
            return
        self._row(d, 0, "plain")

    def _plan_d(self, d, L, rng):
        beg, nK, W = int(self.doc_ptr[d]), self.nK, self.nK + d
        if len(self.free) < 3:
            self._row(d, 0, "plain")
            return
        s_r, t_r = self.free[0], self.free[1]
        alo, ahi = self.base.tolist(), self.base.tolist()
        alo[s_r], ahi[s_r] = self.A_LO * 1.5, self.A_HI * 0.8
        A = self.sums[0]["tie"][0]
        for trial in range(400):
            beta_branch = trial % 2 == 1                            # the proposal from the beta branch: ni[t] = 0, pi_w moves in alpha's own steps
            ni_s = int(rng.integers(1 if beta_branch else 2, 6))
            ni_t = 0 if beta_branch else int(rng.integers(1, ni_s))
            g_s, g_t = int(rng.integers(1 if beta_branch else 0, ni_s + 1)), (0 if beta_branch else int(rng.integers(1, ni_t + 1)))
            p = int(rng.integers(0, L - ni_s - ni_t))
            U = self.U[beg + p]
            need = [(s_r, W)] * g_s + [(s_r, s_r)] * (ni_s - g_s) + [(t_r, W)] * g_t + [(t_r, t_r)] * (ni_t - g_t)
            suffix = need + [(int(k), int(k)) for k in self.z0[beg + p + 1 + len(need):beg + L]]
            suffix = [suffix[i] for i in rng.permutation(len(suffix))]
            topics = [int(k) for k in self.z0[beg:beg + p]] + [s_r] + [k for k, _ in suffix]
            words = list(topics[:p]) + [W] + [w for _, w in suffix]
            t = t_r
            if beta_branch:
                _, det = self.trial(topics, words, d, p, alo, A, BETA)
                if not det or det["tb"] or not (det["word"] in FILL or det["word"] in self.free[1:]):
                    continue
                t = det["word"]
            ok = True
            for al, sign in ((alo, -1.0), (ahi, 1.0)):              # pi_w grows with alpha[z0]: ni[t] < ni[s]
                _, det = self.trial(topics, words, d, p, al, A, BETA)
                if not det or det["pi_w"] is None or det["word"] != t or sign * (det["pi_w"] - U[1]) <= 0:
                    ok = False
                    break
            if not ok:
                continue
            t_r = t
            self._claim(s_r)
            if t_r >= K:
                self._claim(t_r)
            self._put(d, topics, words)
            row = self._row(d, p, "d")
            row.s_r, row.t = s_r, t_r
            return
        self._row(d, 0, "plain")

    # ---- the knobs over the exact counts ---------------------------------------------------------------------------
    def _solve(self):
        nK = self.nK
        for d in range(len(self.lens)):
            if d not in self.row_of:
                self._row(d, 0, "plain")
        self.rows.sort(key=lambda r: r.doc)
        # the rows' states under the nominal vector of each triple
        nominal = []
        for q in range(8):
            vec = self.base.copy()
            for row in self.rows:
                if row.kind in "dg":
                    vec[row.s_r] = 0.1
            A = self.sums[q]["tie"][0]
            vec[self.SLACK] = A - R.alpha_sum(vec[:nK - 1], nK - 1)
            nominal.append((vec, R.alpha_sum(vec, nK), self.walk(vec, BETA)))
        for row in self.rows:
            if row.kind not in "dg":
                continue
            vec, total, z = nominal[row.q if row.kind == "g" else 0]
            st = self.state(row, z)
            _, det = self.eval(row, st, vec, total, BETA)
            row.knob = {}
            if row.kind == "d" and det["pi_w"] is not None and det["word"] == row.t:
                args = det["w_args"]
                got = solve(lambda a: pi_word(a, *args), row.U[1], _bits(self.A_LO), _bits(self.A_HI), (float(args[3]), float(args[4])))
            elif row.kind == "g" and det["pi_d"] is not None and (det["doc"], det["state"]) == (row.dt, row.state):
                args = det["d_args"]
                got = solve(lambda a: pi_doc(a, *args), row.U[3], _bits(self.A_LO), _bits(self.A_HI), (float(args[2]), float(args[3]), float(args[5])))
            else:
                got = None
            if got is None:
                row.kind = "plain"
                continue
            row.centre, row.knob = got
        self.vectors, self.totals = [], []
        for v in range(N_VECTORS):
            tag, q = TAGS[v % 3], v // 3
            vec = self.base.copy()
            for row in self.rows:
                if row.kind in "dg":
                    vec[row.s_r] = row.knob.get(tag, row.centre) if (row.kind == "d" or row.q == q) else row.centre
            done = False
            for nudge in range(16):                                 # the last pool topic's alpha moves the partial sum's last bits
                vec[nK - 2] = self.A_POOL + nudge * 2.0 ** -49
                S = R.alpha_sum(vec[:nK - 1], nK - 1)
                assert S < self.FLOOR - 0.5, S
                for A in self.sums[q][tag]:
                    a = A - S
                    for k in (0, 1, -1, 2, -2):                     # the k-order sum ends with the slack topic
                        ak = _dbl(_bits(a) + k)
                        if S + ak == A:
                            vec[self.SLACK], done = ak, True
                            break
                    if done:
                        break
                if done:
                    break
            assert done, "no slack alpha for vector %d: S %r, sums %r" % (v, S, self.sums[q])
            self.vectors.append(vec)
            self.totals.append(A)
        self.walks = {v: self.walk(self.vectors[v], BETA) for v in range(N_VECTORS)}
        self._settle(lambda row: [v for v in range(N_VECTORS) if row.kind == "d" or (row.kind == "g" and row.q == v // 3) or self.aimed[v // 3] is row])
        for row in self.rows:                                       # e and f: all three tags; d and g: "above" accepts, the others do not
            have = set(row.tags.values())
            if row.kind in "ef":
                assert have == set(TAGS), (self.describe(row), have)
        self.checked = {}

    def knobs(self, v):
        return self.vectors[v].tolist(), self.totals[v], BETA

    def scan_of(self, v):
        return v // 3

    def handles(self):
        return list(range(N_VECTORS))


class BetaEdges(_Edges):
    """a, b and c rows: one alpha vector, one beta value per handle, one aimed row per value."""
    nK = 100
    B_LO, B_HI = 0.004, 0.03
    N_SHORT, N_LONG, TSCALE, N_BALLAST = 90, 10, 20, 30
    # c: the integers m between cells m - 1 and m, first (see the module's docstring), middle, last; alternatives in order of preference
    PLAN = [("b", "long"), ("c", (nK - 1,)), ("c", (48, 56)), ("c", (1, 3)), ("a", (0,)), ("a", (0,)), ("a", (0,)), ("b", "cell 0"), ("b", "cell 0"),
            ("b", "cell 0"), ("b", "short")]

    def __init__(self, seed=5):
        nK = self.nK
        self.alpha = np.resize(ALPHA[:8], nK).tolist()
        self.total = R.alpha_sum(self.alpha, nK)
        self._plan(np.random.default_rng(seed))
        self._count()
        self._solve()

    def _plan(self, rng):
        lens = np.concatenate((rng.integers(8, 17, self.N_SHORT), np.full(self.N_LONG, 131), np.full(self.N_BALLAST, 100)))
        self._layout(lens, rng)
        self.free = list(range(K, self.nK - 1))                     # a pool topic belongs to one row
        for kind, what in self.PLAN:
            docs = [d for d in range(self.N_SHORT + self.N_LONG) if d not in self.row_of and (kind != "b" or (self.lens[d] > 100) == (what == "long"))]
            row = None
            for m in (what if kind != "b" else (0,)):
                for d in docs:
                    row = self._plan_b(d, what, rng) if kind == "b" else self._plan_ac(d, kind, m, rng)
                    if row is not None:
                        break
                if row is not None:
                    break
            assert row is not None, "no document takes the %s row (%s)" % (kind, what)
        self._ballast(self.N_SHORT + self.N_LONG)

    def _doc(self, d, p, z0, own, rng):
        """the document's planned (topics, words): fillers, the target at p on z0, the word's further tokens `own` behind it"""
        beg, L, W = int(self.doc_ptr[d]), self.lens[d], self.nK + d
        suffix = [(k, W) for k in own] + [(int(k), int(k)) for k in self.z0[beg + p + 1 + len(own):beg + L]]
        suffix = [suffix[i] for i in rng.permutation(len(suffix))]
        topics = [int(k) for k in self.z0[beg:beg + p]] + [z0] + [k for k, _ in suffix]
        return topics, [int(k) for k in self.z0[beg:beg + p]] + [W] + [w for _, w in suffix]

    def closure(self, kind, U1, tpt, m):
        """(the computed side as a function of beta, the bound) of an a or c row: no count enters"""
        fK, ftpt = float(self.nK), float(tpt)
        if kind == "a":
            return (lambda b: U1 * (ftpt + b * fK)), ftpt
        return (lambda b: ((U1 * (ftpt + b * fK) - ftpt) / (b * fK)) * fK), float(m)

    def _plan_ac(self, d, kind, m, rng):
        nK, L, beg = self.nK, self.lens[d], int(self.doc_ptr[d])
        for p in range(L - 1):
            U1 = self.U[beg + p][0]
            for tpt in range(1, min(9, L - p)):
                den = U1 - m / float(nK)
                if den <= 0.0:
                    continue
                beta0 = tpt * (1.0 - U1) / den / nK
                if not 0.0045 <= beta0 <= 0.028 or tpt - 1 > len(self.free):
                    continue
                val, bound = self.closure(kind, U1, tpt, m)
                lo = _bisect(lambda b: val(b) < bound, _bits(beta0 * 0.999), _bits(beta0 * 1.001))
                if lo is None or len(_scan(val, bound, lo)) < 3:
                    continue
                z0 = int(FILL[int(rng.integers(len(FILL)))])
                own = self.free[:tpt - 1]
                topics, words = self._doc(d, p, z0, own, rng)
                one, two = [("bcell", m - 1), ("bcell", m)] if kind == "c" else [("branch", False), ("branch", True)]
                ev = lambda f: self.trial(topics, words, d, p, self.alpha, self.total, beta0, f)[0]     # noqa: E731
                if ev(one) == ev(two) or ev(one) is None or ev(two) is None:
                    continue
                del self.free[:tpt - 1]
                self._put(d, topics, words)
                row = self._row(d, p, kind)
                row.m, row.tpt, row.beta0, row.lo = m, tpt, beta0, lo
                return row
        return None

    def key(self, row, det):
        """what grows with beta: past the row's comparison or not"""
        if not det:
            return True
        if row.kind == "a":
            return not det["tb"]
        if row.kind == "c":
            return det["tb"] is False and det["word"] >= row.m
        return (not det["tb"]) or (det["cell"], det["up"]) > (row.cell, False)

    def _plan_b(self, d, what, rng):
        nK, L, beg = self.nK, self.lens[d], int(self.doc_ptr[d])
        for trial in range(300 if what != "long" else 2000):
            if what == "long":
                nnz = int(rng.integers(65, 69))
                p = int(rng.integers(0, L - nnz - 2))
                if not 0.012 <= self.U[beg + p][0] <= 0.03:
                    continue
            else:
                nnz = int((3, 5, 6, 7)[int(rng.integers(4))])       # no power of two: (u_w / tpt) * nnz and u_w * nnz / tpt differ
                p = int(rng.integers(0, max(1, L - 2 * nnz)))
            if nnz - (len(FILL) if what == "long" else 0) > len(self.free):
                continue
            lst = sorted((list(FILL) + self.free[:nnz - len(FILL)]) if what == "long" else [self.free[int(i)] for i in rng.permutation(len(self.free))[:nnz]])
            cnts = [1] * nnz if what == "long" else [int(c) for c in rng.integers(1, 4, nnz)]
            if sum(cnts) > L - p:
                continue
            if what == "long":                                      # a few doubled: the table is not all ties
                for i in rng.permutation(nnz)[:min(L - p - nnz - 1, 12)]:
                    cnts[int(i)] += 1
            z0 = lst[int(rng.integers(nnz))]
            own = [k for k, c in zip(lst, cnts) for _ in range(c)]
            own.remove(z0)
            topics, words = self._doc(d, p, z0, own, rng)
            row = Row()
            row.kind = "b"
            ev = lambda b, f=None: self.trial(topics, words, d, p, self.alpha, self.total, b, f)     # noqa: E731
            _, det = ev(0.01)
            if not det or not det["tb"]:
                continue
            row.cell = det["cell"]
            if row.cell != (0 if what == "cell 0" else 1):          # i = 1: frac's grid is twice ps's, the finest after cell 0
                continue
            lo = _bisect(lambda b: self.key(row, ev(b)[1]), _bits(self.B_LO), _bits(self.B_HI))
            if lo is None:
                continue
            _, one = ev(_dbl(lo))
            _, two = ev(_dbl(lo + 1))
            if not (one and two and one["tb"] and two["tb"] and one["cell"] == two["cell"] == row.cell) or one["ps"] >= 1.0:
                continue
            if one["ps"] < 0.5:                                     # below 0.5 ps moves on a finer grid than frac
                continue
            tags = set()
            for j in sorted(range(-WINDOW, WINDOW + 1), key=abs):   # what the scan will reach: all three in cell 0, one at least behind it
                _, det = ev(_dbl(lo + j))
                if det and det["tb"] and det["cell"] == row.cell:
                    t = tag_of(det["frac"], det["ps"])
                    if t is not None and what != "cell 0":          # behind cell 0 the fused fraction is another double: the row shows it
                        t = t if self.trial(topics, words, d, p, self.alpha, self.total, _dbl(lo + j), slip="fused_frac")[0] != det["new"] else None
                    tags.add(t)
                if len(tags - {None}) == 3 or abs(j) > 64 and what != "cell 0":
                    break
            if len(tags - {None}) < (3 if what == "cell 0" else 1):
                continue
            if ev(_dbl(lo), ("alias", False))[0] == ev(_dbl(lo), ("alias", True))[0]:
                continue
            if any(int((self.z0 == k).sum()) + topics.count(k) > self.target[k] for k in set(topics) if k in self.target):
                continue
            self.free = [k for k in self.free if k not in lst]
            self._put(d, topics, words)
            r = self._row(d, p, "b")
            r.cell, r.nnz, r.beta0, r.what = row.cell, nnz, _dbl(lo), what
            return r
        return None

    def _solve(self):
        for d in range(len(self.lens)):
            if d not in self.row_of:
                self._row(d, 0, "plain")
        self.rows.sort(key=lambda r: r.doc)
        self.betas, self.aimed = [], []
        for row in self.rows:
            if row.kind == "plain":
                continue
            st = self.state(row, self.walk(self.alpha, row.beta0))
            ev = lambda b, f=None: self.eval(row, st, self.alpha, self.total, b, force=f)     # noqa: E731
            found, outs, partner = {}, {}, {}
            if row.kind in "ac":                                    # the candidates per tag from the closed form, the first useful one taken
                val, bound = self.closure(row.kind, row.U[0], row.tpt, row.m)
                cands = [(t, float(b)) for t, xs in _scan(val, bound, row.lo).items() for b in xs[:8]]
            else:
                lo = _bisect(lambda b: self.key(row, ev(b)[1]), _bits(self.B_LO), _bits(self.B_HI))
                cands = [(None, _dbl(lo + j)) for j in sorted(range(-WINDOW, WINDOW + 1), key=abs)] if lo is not None else []
            for want, b in cands:
                _, det = ev(b)
                sd = self.sides(row, det) if det else None
                if sd is None:
                    continue
                t, out = tag_of(*sd), self.outcome(row, det)
                assert want is None or t == want
                if (t in found) or (t is None and out in partner):
                    continue
                if not self.useful(row, lambda f: ev(b, f)):
                    continue
                if t is None:
                    partner[out] = b
                else:
                    found[t], outs[t] = b, out
                if len(found) == 3:
                    break
            self._tab = {}
            chosen = [found[t] for t in TAGS if t in found]
            if len(set(map(repr, outs.values()))) < 2:              # the flip pair: an untagged value on the other side
                chosen += [b for out, b in partner.items() if out not in outs.values()][:1]
            for b in chosen:
                self.betas.append(b)
                self.aimed.append(row)
        assert len(self.betas) <= MAX_HANDLES, len(self.betas)
        self.walks = {h: self.walk(self.alpha, self.betas[h]) for h in range(len(self.betas))}
        self._settle(lambda row: [h for h in range(len(self.betas)) if self.aimed[h] is row])
        self.checked = {}

    def knobs(self, h):
        return self.alpha, self.total, self.betas[h]

    def handles(self):
        return list(range(len(self.betas)))


# ---- the random corpora: tests/test_lightcollapsed_gpu.py::test_ragged_corpus and the cats fixture -----------------------
RAGGED = dict(K=7, V=6, alpha=0.3, beta=0.1, seed=777, zseed=5)


def ragged_corpus():
    """(doc_ptr, tokens): documents of 0 and 1 tokens, 63, 64 and 65 (chunk boundaries), 130 and 700 tokens over 5 of V = 6 words"""
    return PK.ragged_corpus()


# ---- the table build on its edge -----------------------------------------------------------------------------------------
EQUAL_NNZ = (1, 2, 3, 5, 7, 64, 65)
EQUAL_K = 80


def equal_count_words():
    """(n_wk [len(EQUAL_NNZ) + 1][EQUAL_K], n_k): word i sits with the same count on EQUAL_NNZ[i] topics, the last word
    levels n_k, so every topic has the same total: each p_i of a word is the same double, p_i / typeMass - 1.0 / nnz is
    +-0 or one rounding away, and the lows / highs split of the pairing chain sits on its edge."""
    rng = np.random.default_rng(65)
    n_wk = np.zeros((len(EQUAL_NNZ) + 1, EQUAL_K), np.int64)
    for i, nnz in enumerate(EQUAL_NNZ):
        n_wk[i, np.sort(rng.permutation(EQUAL_K)[:nnz])] = 1 + i % 3
    n_wk[-1] = n_wk[:-1].sum(axis=0).max() + 1 - n_wk[:-1].sum(axis=0)
    return n_wk, n_wk.sum(axis=0)


def equal_count_corpus():
    """(doc_ptr, tokens, z0) with exactly those counts: the (word, topic) pairs shuffled into documents of 1 to 90 tokens"""
    n_wk, _ = equal_count_words()
    rng = np.random.default_rng(66)
    w, k = np.nonzero(n_wk)
    pairs = np.repeat(np.stack((w, k), axis=1), n_wk[w, k], axis=0)[rng.permutation(int(n_wk.sum()))]
    lens = []
    while sum(lens) < len(pairs):
        lens.append(min(int(rng.integers(1, 91)), len(pairs) - sum(lens)))
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64), pairs[:, 0].astype(np.int32), pairs[:, 1].astype(np.int32)


_cache = {}


def edges(name):
    """the builders' results, built once per process: "alpha", "beta" """
    if name not in _cache:
        _cache[name] = {"alpha": AlphaEdges, "beta": BetaEdges}[name]()
    return _cache[name]
