"""The knife-edge rows of scheme=polyaurn_sparse (tests/polyaurn_sparse_knife_edge.py) on the CPU: the builder reaches
every edge it aims at, the restatement draws what the builder expects there, and a numpy model of the kernel's proposal
(the wave scans, eps, thr, dm, delta, the look-back at sel - 1) never decides a token differently from the restatement --
in the kernel's own association of the scans and in three others -- while with the margin taken away (eps_scale = 0) it
does: the rows reach the decisions the margins are there for."""
import time

import numpy as np

from tests import polyaurn_sparse_knife_edge as KE

FIXTURES = ("narrow", "wide")


def _row_scores(ke, row):
    """scores [J][n] of the row's candidates at every scan value: (double)cnt * phi, as the kernel forms them"""
    cand = np.asarray(row.cand, np.int64)
    return np.stack([row.cntv * ke.column(row, j)[cand] for j in range(ke.J)])


def test_builder_reaches_every_category_and_the_restatement_draws_it(oracle):
    t0 = time.time()
    counts, pairs, ties, raised = {}, {}, 0, {}
    for name in FIXTURES:
        ke = KE.fixture(name)
        sv = ke.survey()
        for k, v in sv["counts"].items():
            counts[k] = counts.get(k, 0) + v
        for k, v in sv["pairs"].items():
            pairs[k] = pairs.get(k, 0) + v
        ties += sv["ps_ties"]
        raised[name] = len(sv["invalid"])
        # the restatement's draw of every target at every scan value is the candidate the builder picks on its own
        aimed = 0
        for row, ev in zip(ke.rows, sv["evals"]):
            for j, (cat, want, new, det) in enumerate(ev):
                if cat != "invalid":
                    assert new == want, (name, KE.LIST_NAME[row.lst], row.kind, row.pos, cat, j)
                    aimed += cat in KE.EDGE_CATS
        assert aimed > 1000
        # whole z steps: the prefix tokens stay where they are (the rows are in the state they were built for)
        targets = np.array([row.target for row in ke.rows])
        js = [j for j in (0, ke.SCAN // 2, ke.SCAN, ke.SCAN + ke.SCAN // 2, ke.NEAR - 1, ke.J - 1) if j not in sv["invalid"]]
        for j in js if name == "narrow" else js[::2]:
            z, stats = ke.restatement_z(j)
            prefix = np.ones(z.size, bool)
            prefix[targets] = False
            assert (z[prefix] == ke.z0[prefix]).all(), "a prefix token moved"
            assert (z[targets] == [ev[j][2] for ev in sv["evals"]]).all()
            assert stats[KE.R.UNIFORM] == 0 and stats[KE.WORD] > 0 and stats[KE.DOC] > 0
        for j in sv["invalid"][:2]:
            assert ke.restatement_z(j)[0] is None
        n = [row.n for row in ke.rows]
        print("%s: %d rows, %d tokens, K = %d, %d to %d candidates, %d scan values, %d of them raise" %
              (name, len(ke.rows), len(ke.tokens), ke.K, min(n), max(n), ke.J, raised[name]))
        # the choice of the list at its own edge: nw == nd goes to the document's list, nw == nd - 1 to the word's
        aimed_rows = [row for row in ke.rows if row.kind != "plain"]
        assert sum(row.lst == KE.DOC and np.count_nonzero(row.col) == row.nd for row in aimed_rows) >= 4
        assert sum(row.lst == KE.WORD and row.n == row.nd - 1 for row in aimed_rows) >= 4
        if name == "wide":
            assert min(row.n for row in ke.rows if row.kind != "plain") > 64
    print("scan values per (list, kind, position): tie / below / above")
    for key in KE.required_categories():
        got = [counts.get(key + (cat,), 0) for cat in KE.EDGE_CATS]
        print("  %-5s %-8s %-7s %5d %5d %5d" % (key + tuple(got)))
        for cat, c in zip(KE.EDGE_CATS, got):
            assert c >= KE.MIN_PER_CATEGORY, (key, cat, c)
    print("pairs per (list, kind): %s; exact ties frac == ps[w][i]: %d" % (sorted(pairs.items()), ties))
    for lname in KE.LIST_NAME.values():
        for kind in KE.PAIR_KINDS:
            assert pairs.get((lname, kind), 0) >= KE.MIN_PER_CATEGORY, (lname, kind, pairs)
        assert counts.get((lname, "plain", "-", "plain"), 0) > 0
    print("wall time %.1f s" % (time.time() - t0))


def test_the_proposal_model_restates_the_scans():
    rng = np.random.default_rng(0)
    x = rng.random((3, 64))
    exact = np.cumsum(x, axis=1)
    for assoc in KE.ASSOCIATIONS:
        got, last = KE.block_sums(x, assoc)
        assert np.allclose(got, exact, rtol=1e-14, atol=0) and (last == got[:, 63]).all()
    ints = rng.integers(0, 1000, (2, 150)).astype(np.float64)      # exact in every association
    for assoc in KE.ASSOCIATIONS:
        got, last = KE.block_sums(ints, assoc)
        assert (got == np.cumsum(ints, axis=1)).all() and (last == got[:, -1]).all()
    # the dpp association is not the chain's: the measured support for the walk rows
    for n in (4, 100):
        s = rng.random((200, n))
        differ = (KE.block_sums(s, "dpp")[0] != np.cumsum(s, axis=1)).mean()
        print("n = %d: the dpp scan's prefix differs from the chain's at %.0f %% of entries" % (n, 100 * differ))
        assert differ > 0.05


def test_the_margin_is_sufficient_and_the_rows_reach_the_decision(oracle):
    """eps_scale = 1: whenever the proposal decides, in any association, it decides the restatement's topic; every tie is
    left to the replay.  eps_scale = 0, the dpp association: the proposal draws wrong topics on walk tokens of both lists
    (asserted), and the counts among the branch, ps and cell pairs are printed; a pair kind that yields none there is
    not forced."""
    t0 = time.time()
    wrong0, wrong0_pairs, undecided, aimed = {}, {}, {}, {}
    total = decided = far_total = far_decided = 0
    for name in FIXTURES:
        ke = KE.fixture(name)
        sv = ke.survey()
        for row, ev in zip(ke.rows, sv["evals"]):
            scores = _row_scores(ke, row)
            lname = KE.LIST_NAME[row.lst]
            for assoc in KE.ASSOCIATIONS:
                cuml, last = KE.block_sums(scores, assoc)
                for j, (cat, want, new, det) in enumerate(ev):
                    # the word's alias table: the restatement's where it read one; built here where U is close enough to
                    # the threshold for a proposal to take the alias branch instead; else the proposal must not read it
                    if det["tables"] is None and row.U < det["thr"] * (1.0 + 1e-6):
                        det["tables"] = KE.SR.alias_table(ke.column(row, j) * KE.ALPHA)[:2]
                    ps, a = det["tables"] if det["tables"] is not None else (None, None)
                    args = (scores[j], det["tn"], row.U, ke.K, ps, a, row.cand)
                    got = KE.proposal(*args, eps_scale=1.0, assoc=assoc, sums=(cuml[j], float(last[j])))
                    if got is not None:
                        assert cat != "invalid" and got == new, (name, lname, row.kind, row.pos, cat, j, assoc, got, new)
                    if assoc != "dpp" or cat == "invalid":
                        continue
                    total += 1
                    decided += got is not None
                    if j >= ke.NEAR and row.kind != "plain":
                        far_total += 1
                        far_decided += got is not None
                    if cat in KE.EDGE_CATS:
                        aimed[cat] = aimed.get(cat, 0) + 1
                        undecided[cat] = undecided.get(cat, 0) + (got is None)
                        if cat == "tie":
                            assert got is None, (name, lname, row.kind, row.pos, j)
                    got0 = KE.proposal(*args, eps_scale=0.0, assoc=assoc, sums=(cuml[j], float(last[j])))
                    if got0 is not None and got0 != new:
                        if not det["prior"]:
                            wrong0[lname] = wrong0.get(lname, 0) + 1
                        if "pair" in det:
                            key = (lname, det["pair"])
                            wrong0_pairs[key] = wrong0_pairs.get(key, 0) + 1
    print("eps_scale = 1: undecided of the aimed scan values: %s; decided of all target tokens: %d of %d" %
          (", ".join("%s %d of %d" % (c, undecided.get(c, 0), aimed.get(c, 0)) for c in KE.EDGE_CATS), decided, total))
    print("of the aimed rows' scan values 2^7 .. 2^22 ulps away from the edge it decides %d of %d" % (far_decided, far_total))
    assert far_decided > far_total // 4, "the model's proposal decides next to nothing: it shows nothing about the margin"
    print("eps_scale = 0, dpp: wrong topics on walk tokens per list %s; among the pairs %s" % (sorted(wrong0.items()), sorted(wrong0_pairs.items())))
    print("wall time %.1f s" % (time.time() - t0))
    for lname in KE.LIST_NAME.values():
        assert wrong0.get(lname, 0) > 0, "without the margin the proposal is never wrong on the %s list: the rows do not reach the decision" % lname
