"""Knife-edge rows for the held-out estimator's particle pass (a test helper, not collected; the manner of
tests/lightpclda_knife_edge.py).

One particle's pass over one test document (MarginalProbEstimatorPlain.leftToRight, MPE:123-519) makes five comparisons
per token.  With sample = u * (smoothingOnlyMass + topicBetaMass + topicTermMass):

  a  term bucket      sample < topicTermMass
  b  term walk        sample -= score[cell]; sample > 0                 (goes on to the next cell)
  c  beta bucket      sample - topicTermMass < topicBetaMass
  d  beta walk        sample -= n[topic] / denom[topic]; sample <= 0.0  (ends at this topic of the particle's own)
  e  smoothing walk   sample -= alpha[topic] / denom[topic]; sample > 0.0   (goes on to the next topic)

Random data never puts a sample on a bound, so < against <= is invisible to parity runs.  A row here is a (test document,
particle, token) whose comparison is ON the bound.  The knob is continuous: the alpha of a slack topic (the last one,
without a training token, which no row's word has a count on).  It moves smoothingOnlyMass alone, hence every sample.
Alpha is fixed at create: every alpha vector is a handle of its own and aims ONE target.

Tags.  "tie": the computed side equals the bound; "below" / "above": it is the neighbouring double under / over it.  For a
and c the computed side is the sample and the bound the mass.  For the walks the comparison is with zero after a
subtraction; x - y > 0 exactly when x > y in IEEE arithmetic, so the computed side is the sample BEFORE the subtraction
and the bound is what is subtracted (doubles next to zero are out of reach of a difference of two such numbers).

A (row, vector) counts only where forcing the comparison one way and the other changes the bits of the document's log
likelihood (`useful`).

step() is the builder's own arithmetic of one pass -- plain Python floats, written apart from oracle/ggs_oracle.c -- with
switchable slips (SLIPS) and with `force`.  It walks a word's non-zero cells only: a zero cell multiplies to 0.0, adds
+0.0 to the mass and subtracts 0.0 in the walk, which changes no bit and ends no walk.
"""
import bisect

import numpy as np

PURPOSE_HELDOUT = 5
TAGS = ("below", "tie", "above")
MIN_PER_CATEGORY = 4
SCAN = 64
CAP = 64                                                            # the deepest coefficient table (kHeldoutCoefCaps[0]): what a small K gets

# slip -> its comparison.  The comparison slips put the other relation; the order slips round the sample another way:
#   total_assoc     sample = u * (smoothing + (betaMass + termMass))            (the word probability keeps the right sum)
#   beta_div_first  the smoothing bucket divides first: sample / beta - betaMass / beta for (sample - betaMass) / beta
SLIPS = {"term_le": "a", "walk_ge": "b", "beta_le": "c", "betawalk_lt": "d", "smooth_ge": "e", "total_assoc": "a", "beta_div_first": "e"}
COMPARISON_SLIPS = ("term_le", "walk_ge", "beta_le", "betawalk_lt", "smooth_ge")


class InvalidTopic(Exception):
    """what Java throws (MPE:416,447,455,464-469) and both sides report as INVALID_TOPIC"""


def _bits(x):
    return int(np.float64(x).view(np.int64))


def _dbl(b):
    return float(np.int64(b).view(np.float64))


def _next(x, up):
    return float(np.nextafter(x, np.inf if up else -np.inf))


def tag_of(computed, bound):
    if computed == bound:
        return "tie"
    if computed == _next(bound, False):
        return "below"
    if computed == _next(bound, True):
        return "above"
    return None


def step(doc, cells, alpha, denom, beta, smoothing, alpha_sum, num_types, U, slip=None, force=None, detail=None, survey=False, stop=None):
    """One particle's pass over doc; returns its word probabilities (0.0 at out-of-vocabulary positions).

    cells[w]: the word's non-zero (topic, count) cells in topic order.  U: the particle's uniforms, one per in-vocabulary token.
    force = (token, comparison, index, outcome): at in-vocabulary token number `token`, the comparison's outcome is imposed --
    for the walks at cell / own-topic / topic number `index`; outcome True means "a" in the term bucket, "b" goes on, "c" in
    the beta bucket, "d" ends here, "e" goes on.
    detail: a list that gets one record per in-vocabulary token: u, masses, the comparisons made as
    (comparison, index, computed, bound, outcome), the topic drawn, the particle's count of it before; with survey also the
    sample at which every comparison of the token would be on its bound (`edges`) and the particle's counts.
    stop: the pass ends after in-vocabulary token number `stop` (the builder's searches need no more)."""
    nK = len(alpha)
    counts = [0] * nK
    mine = []                                                       # the particle's non-zero topics, ascending
    beta_mass = 0.0
    so_far = 0
    probs = [0.0] * len(doc)
    for pos, w in enumerate(doc):
        if w >= num_types:
            continue
        row = cells[w]
        scores = []
        mass = 0.0
        for k, c in row:
            s = (alpha[k] + float(counts[k])) / denom[k] * float(c)
            scores.append(s)
            mass += s
        total = smoothing + beta_mass + mass
        u = U[so_far]
        sample = u * (smoothing + (beta_mass + mass)) if slip == "total_assoc" else u * total
        probs[pos] = total / (alpha_sum + float(so_far))
        forced = force if force is not None and force[0] == so_far else None
        cmps = []
        rec = None
        if detail is not None:
            rec = dict(token=so_far, pos=pos, u=u, smoothing=smoothing, beta_mass=beta_mass, mass=mass, cmps=cmps)
            if survey:
                edges = []
                if mass > 0.0:
                    edges.append(("a", None, mass))
                run = 0.0
                for j, s in enumerate(scores):
                    run += s
                    edges.append(("b", j, run))
                if beta_mass > 0.0:
                    edges.append(("c", None, mass + beta_mass))
                run = 0.0
                for j, k in enumerate(mine):
                    run += float(counts[k]) / denom[k]
                    edges.append(("d", j, mass + beta * run))
                run = 0.0
                for k in range(nK - 1):
                    run += alpha[k] / denom[k]
                    edges.append(("e", k, mass + beta_mass + beta * run))
                rec["edges"] = edges
                rec["counts"] = list(counts)
                rec["mine"] = list(mine)
            detail.append(rec)
        so_far += 1
        new = -1
        in_term = sample <= mass if slip == "term_le" else sample < mass
        if forced is not None and forced[1] == "a":
            in_term = forced[3]
        cmps.append(("a", None, sample, mass, in_term))
        if in_term:
            if sample > 0:
                for j, s in enumerate(scores):
                    before = sample
                    sample -= s
                    on = sample >= 0 if slip == "walk_ge" else sample > 0
                    if forced is not None and forced[1] == "b" and forced[2] == j:
                        on = forced[3]
                    cmps.append(("b", j, before, s, on))
                    if not on:
                        new = row[j][0]
                        break
        else:
            sample -= mass
            in_beta = sample <= beta_mass if slip == "beta_le" else sample < beta_mass
            if forced is not None and forced[1] == "c":
                in_beta = forced[3]
            cmps.append(("c", None, sample, beta_mass, in_beta))
            if in_beta:
                sample /= beta
                for j, k in enumerate(mine):
                    part = float(counts[k]) / denom[k]
                    before = sample
                    sample -= part
                    end = sample < 0.0 if slip == "betawalk_lt" else sample <= 0.0
                    if forced is not None and forced[1] == "d" and forced[2] == j:
                        end = forced[3]
                    cmps.append(("d", j, before, part, end))
                    if end:
                        new = k
                        break
            else:
                if slip == "beta_div_first":
                    sample = sample / beta - beta_mass / beta
                else:
                    sample -= beta_mass
                    sample /= beta
                k = 0
                while True:
                    part = alpha[k] / denom[k]
                    before = sample
                    sample -= part
                    on = sample >= 0.0 if slip == "smooth_ge" else sample > 0.0
                    if forced is not None and forced[1] == "e" and forced[2] == k:
                        on = forced[3]
                    cmps.append(("e", k, before, part, on))
                    if not on:
                        new = k
                        break
                    k += 1
                    if k >= nK:
                        break
        if new < 0:
            raise InvalidTopic("token %d" % (so_far - 1))
        if rec is not None:
            rec["topic"], rec["count"] = new, counts[new]
        beta_mass -= beta * float(counts[new]) / denom[new]
        if counts[new] == 0:
            bisect.insort(mine, new)
        counts[new] += 1
        beta_mass += beta * float(counts[new]) / denom[new]
        if stop is not None and so_far > stop:
            break
    return probs


class Vector:
    """one alpha vector = one handle: its slack alpha and the row it aims"""

    def __init__(self, slack, doc, particle, token, kind, index, tag, useful, ends_at, count, invalid, late):
        self.slack, self.doc, self.particle, self.token, self.kind, self.index, self.tag = slack, doc, particle, token, kind, index, tag
        self.useful, self.ends_at, self.count, self.invalid, self.late = useful, ends_at, count, invalid, late

    def key(self):
        return (self.doc, self.particle, self.token, self.kind, self.index)


class Model:
    """Counts, a test set and the builder's own arithmetic around step(): the estimator of a whole test set as a function of
    the last topic's alpha."""

    def __init__(self, O, alpha, beta, n_wk, docs, particles, seed, iteration):
        self.O = O
        self.K, self.V = len(alpha), len(n_wk)
        self.SLACK = self.K - 1
        self.alpha0, self.beta = [float(a) for a in alpha], float(beta)
        self.n_wk = np.asarray(n_wk, np.int64)
        assert self.n_wk.shape == (self.V, self.K)
        self.n_k = self.n_wk.sum(axis=0)
        self.docs, self.P, self.seed, self.iteration = [[int(w) for w in d] for d in docs], int(particles), seed, iteration
        self.cells = [[(k, int(c)) for k, c in enumerate(r) if c] for r in self.n_wk]
        beta_sum = self.beta * self.V
        self.denom = [float(n) + beta_sum for n in self.n_k]
        self._U = {}
        self._tables = {}
        self._probs = {}


    # ---- the builder's own arithmetic around step()
    def uniforms(self, d, q):
        """the stream of particle q of test document d: Philox block b of element d * P + q gives uniforms 2b and 2b + 1"""
        if (d, q) not in self._U:
            n = sum(w < self.V for w in self.docs[d])
            elem = d * self.P + q
            out = []
            for blk in range((n + 1) // 2):
                o = self.O.philox([elem & 0xffffffff, elem >> 32, (PURPOSE_HELDOUT << 24) | blk, self.iteration], [self.seed & 0xffffffff, self.seed >> 32])
                out += [float(((o[0] >> 6) << 27) + (o[1] >> 5)) * 2.0 ** -53, float(((o[2] >> 6) << 27) + (o[3] >> 5)) * 2.0 ** -53]
            assert not out or out[0] == self.O.uniforms(self.seed, self.iteration, PURPOSE_HELDOUT, elem, 1)[0]
            self._U[(d, q)] = out
        return self._U[(d, q)]

    def tables(self, slack):
        """(alpha, smoothingOnlyMass, alphaSum): running sums in topic order (MPE:75-78)"""
        if slack not in self._tables:
            alpha = self.alpha0[:-1] + [float(slack)]
            smoothing = a_sum = 0.0
            for k in range(self.K):
                smoothing += alpha[k] * self.beta / self.denom[k]
                a_sum += alpha[k]
            if len(self._tables) > 4096:
                self._tables.clear()
            self._tables[slack] = (alpha, smoothing, a_sum)
        return self._tables[slack]

    def particle(self, slack, d, q, slip=None, force=None, detail=None, survey=False, stop=None):
        alpha, smoothing, a_sum = self.tables(slack)
        return step(self.docs[d], self.cells, alpha, self.denom, self.beta, smoothing, a_sum, self.V, self.uniforms(d, q), slip, force, detail, survey, stop)

    def doc_value(self, slack, d, slip=None, force=None, particle=None):
        """the document's log likelihood (MPE:102-111): per position the particles' sum in particle order, log, minus
        log(P); the positions in order.  slip / force apply to `particle` alone (or, a slip, to all when particle is None).
        Raises InvalidTopic."""
        if (slack, d) not in self._probs:
            if len(self._probs) > 64:
                self._probs.clear()
            self._probs[(slack, d)] = [self.particle(slack, d, q) for q in range(self.P)]
        rows = self._probs[(slack, d)]
        if particle is not None:
            rows = list(rows)
            rows[particle] = self.particle(slack, d, particle, slip, force)
        elif slip is not None:
            rows = [self.particle(slack, d, q, slip) for q in range(self.P)]
        sums = []
        for pos in range(len(self.docs[d])):
            s = 0.0
            for r in rows:
                s += r[pos]
            sums.append(s)
        logs = self.O.log(np.array(sums + [float(self.P)])).tolist() if sums else [0.0]
        ll = 0.0
        for s, lg in zip(sums, logs):
            if s > 0.0:
                ll += lg - logs[-1]
        return ll

    def values(self, slack, slip=None):
        """(total, per-document values) of the whole test set; the total is the running sum in document order (MPE:116)"""
        ll = [self.doc_value(slack, d, slip) for d in range(len(self.docs))]
        total = 0.0
        for v in ll:
            total += v
        return total, np.array(ll, np.float64)


class Family(Model):
    """A training corpus (its counts n_wk, laid down with set_z), a test set and the vectors aimed on it.

    docs: the test documents; particles: P; want: the categories to fill --
      ("tag", comparison, tag)       MIN_PER_CATEGORY useful rows
      ("end", comparison, position)  one useful row of any tag whose walk ends there (b: compacted-cell index or "last";
                                     d: "first", "last" or ("topic", k); e: the topic)
      ("slip", name)                 one useful row of the slip's comparison that the slip changes (the order slips show only
                                     past a document's first token, where topicBetaMass > 0, and only where they round up)
      ("cap", n)                     one useful row whose comparison takes in the coefficient of a topic the particle holds n times
    """

    def __init__(self, O, name, alpha, beta, n_wk, docs, particles, want, seed=2024, iteration=1, start=1.0, max_tries=1500, near=None):
        Model.__init__(self, O, alpha, beta, n_wk, docs, particles, seed, iteration)
        self.name = name
        assert not self.n_wk[:, self.SLACK].any()
        self.vectors, self.have, self.near = [], {}, near
        self.walks_off_the_row = 0
        self._build(want, start, max_tries)

    # ---- the fixture as arrays
    def train_corpus(self):
        """(doc_ptr, tokens, z): every (word, topic) cell as many tokens, 50 to a document"""
        w, k = np.nonzero(self.n_wk)
        reps = self.n_wk[w, k]
        tokens, z = np.repeat(w, reps).astype(np.int32), np.repeat(k, reps).astype(np.int32)
        ptr = np.unique(np.concatenate((np.arange(0, tokens.size, 50), [tokens.size]))).astype(np.int64)
        return ptr, tokens, z

    def test_corpus(self):
        ptr = np.concatenate(([0], np.cumsum([len(d) for d in self.docs]))).astype(np.int64)
        return ptr, np.array([t for d in self.docs for t in d], np.int32)

    def alpha_vector(self, slack):
        return np.array(self.alpha0[:-1] + [slack], np.float64)

    # ---- aiming
    def _record(self, slack, d, q, token, survey=False):
        """(the draws before `token`, the token's record) or None where the pass raises before"""
        det = []
        try:
            self.particle(slack, d, q, detail=det, survey=survey, stop=token)
        except InvalidTopic:
            pass
        if len(det) <= token:
            return None
        return [r.get("topic") for r in det[:token]], det[token]

    @staticmethod
    def _made(rec, kind, index):
        for c in rec["cmps"]:
            if c[0] == kind and c[1] == index:
                return c
        return None

    def _slack_for(self, rec, at):
        """the slack alpha that puts u * total on `at` given the token's masses"""
        alpha, smoothing, _ = self.tables(rec["slack"])
        rest = smoothing - alpha[self.SLACK] * self.beta / self.denom[self.SLACK]
        s = at / rec["u"] - rec["beta_mass"] - rec["mass"]
        return (s - rest) * self.denom[self.SLACK] / self.beta

    def aim(self, d, q, token, kind, index, start):
        """{tag: slack alpha} for the comparison (kind, index) of token `token` of particle q of document d, or {}.
        The draws before the token must be the same at every value tried (the bisection's and the scan's)."""
        slack, prefix = start, None
        for _ in range(6):
            got = self._record(slack, d, q, token, survey=True)
            if got is None:
                return {}
            before, rec = got
            at = [e[2] for e in rec["edges"] if e[0] == kind and e[1] == index]
            if not at or rec["u"] <= 0.0:
                return {}
            rec["slack"] = slack
            new = self._slack_for(rec, at[0])
            if not 1e-6 < new < 1e6:
                return {}
            if prefix is not None and before == prefix and abs(new - slack) <= 1e-9 * slack:
                break
            slack, prefix = new, before
        else:
            return {}

        def outcome(x):
            got = self._record(x, d, q, token)
            if got is None or got[0] != prefix:
                return None
            return self._made(got[1], kind, index)

        lo, hi = _bits(slack * (1.0 - 1e-7)), _bits(slack * (1.0 + 1e-7))
        a, b = outcome(_dbl(lo)), outcome(_dbl(hi))
        if a is None or b is None or a[4] == b[4]:
            return {}
        while hi - lo > 1:
            mid = (lo + hi) // 2
            m = outcome(_dbl(mid))
            if m is None:
                return {}
            if m[4] == a[4]:
                lo = mid
            else:
                hi = mid
        found = {}
        for j in sorted(range(-SCAN, SCAN + 1), key=abs):
            x = _dbl(lo + j)
            m = outcome(x)
            if m is None:
                continue
            t = tag_of(m[2], m[3])
            if t is not None and t not in found:
                found[t] = x
        return found

    def _classify(self, slack, d, q, token, kind, index, tag):
        """the Vector of an aimed (row, tag), with its usefulness and where the row's walk ends"""
        before, rec = self._record(slack, d, q, token, survey=True)
        values = []
        for side in (False, True):
            try:
                values.append(_bits(self.doc_value(slack, d, force=(token, kind, index, side), particle=q)))
            except InvalidTopic:
                values.append(None)
        try:
            self.particle(slack, d, q)
            invalid = False
        except InvalidTopic:
            invalid = True
        ends_at = None
        if not invalid and kind in "bde":
            last = [c for c in rec["cmps"] if c[0] == kind][-1]
            if kind == "b":
                ends_at = "last" if last[1] == len(self.cells[self.docs[d][rec["pos"]]]) - 1 else last[1]
            elif kind == "d":
                mine = rec["mine"]
                ends_at = [("topic", mine[last[1]])]
                if last[1] == 0:
                    ends_at.append("first")
                if last[1] == len(mine) - 1 and len(mine) > 1:
                    ends_at.append("last")
            else:
                ends_at = last[1]
        # the particle's counts of the topics whose coefficient the compared side takes in
        word = self.cells[self.docs[d][rec["pos"]]]
        upto = len(word) if kind == "a" else index + 1 if kind == "b" else 0
        count = sorted({rec["counts"][k] for k, _ in word[:upto]})
        return Vector(slack, d, q, token, kind, index, tag, values[0] != values[1], ends_at, count, invalid, rec["beta_mass"] > 0.0)

    def _wanted(self, want, v):
        """the categories of `want` that vector v would add to"""
        out = []
        if not v.useful or v.invalid:
            return out
        rows = self.have
        if ("tag", v.kind, v.tag) in want and len(rows.get(("tag", v.kind, v.tag), ())) < MIN_PER_CATEGORY:
            out.append(("tag", v.kind, v.tag))
        for c in want:
            if c[0] == "slip" and SLIPS[c[1]] == v.kind and v.late and not rows.get(c) and self.shows(v, c[1]):
                out.append(c)
        ends = v.ends_at if isinstance(v.ends_at, list) else [v.ends_at]
        for e in ends:
            if ("end", v.kind, e) in want and not rows.get(("end", v.kind, e)):
                out.append(("end", v.kind, e))
        for n in v.count:
            if ("cap", n) in want and not rows.get(("cap", n)):
                out.append(("cap", n))
        return out

    def shows(self, v, slip):
        """does the slip, in the row's particle alone, change the document's value?"""
        try:
            return _bits(self.doc_value(v.slack, v.doc, slip=slip, particle=v.particle)) != _bits(self.doc_value(v.slack, v.doc))
        except InvalidTopic:
            return True

    def missing(self, want):
        return [c for c in want if len(self.have.get(c, ())) < (MIN_PER_CATEGORY if c[0] == "tag" else 1)]

    def _candidates(self, want, d, q, start):
        """(token, comparison, index) worth aiming at for particle q of document d: what the pass at `start` shows"""
        det = []
        try:
            self.particle(start, d, q, detail=det, survey=True)
        except InvalidTopic:
            pass
        kinds = {c[1] for c in want if c[0] in ("tag", "end")}
        caps = {c[1] for c in want if c[0] == "cap"}
        out = []
        for rec in det:
            word = self.cells[self.docs[d][rec["pos"]]]
            rec["slack"] = start
            for kind, index, at in rec["edges"]:
                new = self._slack_for(rec, at) if rec["u"] > 0.0 else -1.0
                if not 1e-6 < new < 1e6 or (self.near is not None and not start / self.near < new < start * self.near):
                    continue                                        # out of the knob's reach, or so far that the draws before move
                if caps:
                    upto = len(word) if kind == "a" else index + 1 if kind == "b" else 0
                    if kind in "ab" and any(rec["counts"][k] in caps for k, _ in word[:upto]):
                        out.append((rec["token"], kind, index))
                    continue
                if kind not in kinds:
                    continue
                if kind in "cde" and rec["mass"] > 0.0:             # the sample loses its last bits to the subtraction of the term mass
                    continue
                if kind == "b" and index not in (0, 1, 6, 7, 8, 62, 63, 64, len(word) - 2, len(word) - 1):
                    continue
                if kind == "e" and index not in (0, 1, self.K - 3, self.K - 2):
                    continue
                out.append((rec["token"], kind, index))
        return out

    def _could_fill(self, c, d, token, kind, index, last):
        """can an edge at (kind, index) add to category c?  Past the first step of a walk only ties are in reach (see the
        fixtures), but for the two steps the fixtures make heavy: the one before the last cell and before the last topic."""
        if c[0] == "cap":
            return kind in "ab"
        if c[0] == "slip":
            return SLIPS[c[1]] == kind and token > 0
        if c[1] != kind:
            return False
        if kind == "d":
            return True
        if c[0] == "tag":
            return c[2] == "tie" or index in (None, 0)
        p = c[2]
        if kind == "b":
            return index == (last - 1 if p == "last" else p)
        return index == min(p, self.K - 2)

    def _build(self, want, start, max_tries):
        want = list(want)
        order = [q for pair in zip(range(64), range(64, 128)) for q in pair if q < self.P] + list(range(128, self.P))
        tries, seen = 0, set()
        for q in order:
            for d in range(len(self.docs)):
                if not self.missing(want) or tries >= max_tries:
                    break
                for token, kind, index in self._candidates(want, d, q, start):
                    missing = self.missing(want)
                    if not missing:
                        break
                    # is anything this comparison could give still missing?
                    last = len(self.cells[self.docs[d][[i for i, w in enumerate(self.docs[d]) if w < self.V][token]]]) - 1
                    if not any(self._could_fill(c, d, token, kind, index, last) for c in missing):
                        continue
                    if (d, q, token, kind, index) in seen:
                        continue
                    seen.add((d, q, token, kind, index))
                    tries += 1
                    found = self.aim(d, q, token, kind, index, start)
                    for tag in TAGS:
                        if tag not in found:
                            continue
                        v = self._classify(found[tag], d, q, token, kind, index, tag)
                        if v.invalid:
                            self.walks_off_the_row += 1
                            self.vectors.append(v)
                            continue
                        cats = self._wanted(want, v)
                        if cats:
                            self.vectors.append(v)
                            for c in cats:
                                self.have.setdefault(c, []).append(v.key())
        self.tries = tries
        self.want = want

    def describe(self, v):
        return "%s: %s[%s] %s, document %d particle %d token %d, slack alpha %r (ends at %s, counts %s)" % (
            self.name, v.kind, v.index, v.tag, v.doc, v.particle, v.token, v.slack, v.ends_at, v.count)


# ---------------------------------------------------------------- the two fixtures
# Deep in a walk the sample is a difference on the grid of u * total while the bound has an ulp of its own: whether
# "sample == bound" can hold at all is then decided by the low bits of the fixture's constants, not by the particle.  Both
# fixtures therefore keep every quotient of the walks dyadic: beta = 0.1 and V = 10 (betaSum = 1.0 exactly, and a division
# by beta still rounds), topic totals n_k = 2^m - 1 (the
# denominators n_k + betaSum are powers of two) and alphas with a few bits.  Ties are then reachable at every depth of every
# walk; the neighbouring doubles where the sample and the bound share a binade (the first step of a walk, a and c).
WIDE_K = 80
BETA = 0.1
NUM_TYPES = 10
assert BETA * NUM_TYPES == 1.0


def _fill(n_wk, filler, least=None):
    """the filler word's counts: what brings every topic's total to 2^m - 1 (at least least[k]); the slack topic stays empty"""
    for k in range(n_wk.shape[1] - 1):
        have = int(n_wk[:, k].sum())
        want = max(have, 1 if least is None else least[k])
        total = 1
        while total - 1 < want:
            total *= 2
        n_wk[filler, k] += total - 1 - have
    assert all(((int(n) + 1) & int(n)) == 0 for n in n_wk.sum(axis=0))
    return n_wk


def wide_family(O):
    """K = 80.  Word 0 has 70 non-zero topics (compacted cells 0 .. 69: two rounds of 64 lanes, the second of 6 cells -- not
    a multiple of kHeldoutBatch = 8 -- and compacted index != topic), heavy at cells 0, 7, 8, 63, 64, 68 and 69.  Word 1 sits on
    topics 3, 7, 8 and 40 (what a particle then holds: the beta walk's topics), word 2 tells those apart, word 3 has no
    training token (topicTermMass = +0.0: the beta and smoothing buckets at full resolution), word 4 tells the first and
    the last topics apart, word 5 only fills the topic totals.  P = 100: two blocks per document, 28 dead lanes."""
    nK = WIDE_K
    n_wk = np.zeros((NUM_TYPES, nK), np.int64)
    topics = [k for k in range(2, 78) if k not in (5, 20, 33, 47, 60, 71)]
    assert len(topics) == 70
    for j, k in enumerate(topics):
        n_wk[0, k] = 40 if j in (0, 7, 8, 63, 64, 68, 69) else 1
    n_wk[1, [3, 7, 8, 40]] = (4, 5, 5, 4)
    n_wk[2, [3, 7, 8, 40]] = (1, 2, 3, 4)
    n_wk[4, [0, 1, 2, 77, 78]] = (1, 2, 1, 1, 3)
    least = [(1, 3, 7, 15, 3, 7)[k % 6] for k in range(nK)]
    for j in (7, 63, 69):                                           # neighbouring heavy cells on topics of different totals: what follows tells them apart
        least[topics[j]] = 127
    _fill(n_wk, 5, least)
    alpha = [(2.0 ** -8, 3 * 2.0 ** -9, 2.0 ** -7)[k % 3] for k in range(nK)]
    alpha[0], alpha[1] = 0.0625, 0.09375
    for k in (3, 7, 8, 40):                                         # word 1's topics: its particles stay on them
        alpha[k] = 0.25
    # the step before the last cell and the step before the last topic are as heavy as all before them: the sample there
    # shares the bound's binade, and "above" -- the walk that goes on to the last cell, the last topic -- is in reach
    alpha[topics[68]], alpha[78] = 0.25, 1.0
    docs = [[0, 0, 2], [0, 0, 2], [0, 4, 0], [0, 11, 0, 2], [0, 2, 0],
            [1, 1, 1, 3, 2], [1, 1, 1, 3, 2], [1, 1, 3, 3, 2], [1, 2, 1, 3, 2], [1, 1, 1, 3, 2],
            [3, 4, 3, 2], [3, 4, 3, 2], [3, 3, 4], [3, 4, 1, 3, 4], [], [4, 3, 3, 4]]
    want = [("tag", kind, tag) for kind in "abcde" for tag in TAGS]
    want += [("end", "b", p) for p in (0, 7, 8, 63, 64, "last")]
    want += [("end", "d", p) for p in ("first", ("topic", 7), ("topic", 8), "last")]
    want += [("end", "e", p) for p in (0, 1, nK - 2, nK - 1)]
    want += [("slip", "total_assoc"), ("slip", "beta_div_first")]                        # where the order of the three masses, of the division by beta, can show
    return Family(O, "wide", alpha, BETA, n_wk, docs, 100, want)


def cap_family(O):
    """K = 4 (the deepest coefficient table, CAP rows): long documents of one word whose particles pile up on topic 1, aimed
    where a particle holds it CAP - 1, CAP and CAP + 1 times -- the last table entry, the first two divisions.  P = 65."""
    n_wk = np.zeros((NUM_TYPES, 4), np.int64)
    n_wk[0] = (3, 50, 3, 0)
    _fill(n_wk, 1, least=[63, 1023, 15, 0])
    alpha = [0.5, 200.0, 0.5, 1.0]
    docs = [[0] * 100] * 6
    want = [("cap", n) for n in (CAP - 1, CAP, CAP + 1)]
    return Family(O, "cap", alpha, BETA, n_wk, docs, 65, want, start=1.0, max_tries=600, near=1.5)


_cache = {}


def families(O):
    """the two families, built once per process"""
    if "f" not in _cache:
        _cache["f"] = (wide_family(O), cap_family(O))
    return _cache["f"]
