"""The knife-edge rows of scheme=adlda (tests/adlda_knife_edge.py) on the CPU: the builder against the restatement -- the
whole z step of tests/adlda_restatement.py at every handle, every token where the builder's step() puts it -- the
minimums the rows are to meet, and the POWER of the rows: each deliberately wrong variant of the token draw (KE.SLIPS:
<= for <, >= for >, the R walk on the undivided sample, a walk that compares start - prefix, tree sums for the chains,
S0 + (y - x), the score multiplied first, a walk that moves on to a zero entry, a stale den(z0)) moves the new topic of a
target of its own comparison, while on the random data the device suite compares (cats at K = 20 under both pairs of
priors of tests/test_adlda_gpu.py, two sweeps) the order and comparison slips move nothing at all: such a kernel differs
from the restatement about once in 2^50 draws, and only rows put on the edge can tell.  (The stale den and the walk that
takes a zero entry do show there -- 7 and 333 of 31 152 draws: a zero entry follows the stop of many a walk, edge or no
edge -- so the device suite's random corpora tell those two already; KE.INDEX_SLIPS.)
tests/test_adlda_knife_edge_gpu.py puts the same rows through the device.

Measured on the CPU this was written on: 30 to 38 s for the file (the search for the rows 10 s, the builder's and the
restatement's whole z step at each of the 44 handles 15 s, the slips on cats 5 s)."""
import numpy as np

from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import adlda_knife_edge as KE
from tests import adlda_restatement as R

WALKS = "cde"


def print_survey(ed):
    counts = ed.survey()
    print("rows with a flip pair per (comparison, position): %s" % sorted((k, v) for k, v in counts.items() if k[1] in KE.POSITIONS[k[0]] + ("any", "flip")))
    print("rows reaching a tag: %s" % sorted((k, v) for k, v in counts.items() if k[1] in KE.TAGS + ("tie at 0",)))
    print("the reference's rare paths: rows %s" % sorted((k, v) for k, v in counts.items() if k in KE.RARE))
    if ed.searched:
        print("    within %d doubles of the flips of %d a and b candidates (%d probes) the Q walk ran past its last entry %d times, the R walk fell "
              "back to K - 1 %d times, the S walk reached K %d times; candidates tried per need: %s" % (
                  KE.WINDOW, ed.rare["candidates"], ed.rare["probes"], ed.rare["Q walk past its last entry"], ed.rare["R walk's K - 1 fallback"],
                  ed.rare["S walk reaches K"], sorted(ed.tried.items())))
    print("proposal rows at handle %d: %s" % (ed.base, sorted((k, len(v)) for k, v in ed.proposals.items())))
    print("%d handles, %d tokens, K = %d; handles that raise: %s" % (len(ed.handles()), ed.tokens.size, KE.K, sorted(ed.raises)))


def assert_survey(ed):
    """the minimums of tests/adlda_knife_edge.py: conditions on the inputs, not measurements"""
    counts = ed.survey()
    assert KE.MAX_HANDLES == 48 and len(ed.handles()) <= KE.MAX_HANDLES
    assert ed.tokens.size <= 3000
    for kind, names in KE.POSITIONS.items():
        for where in names:
            assert counts.get((kind, where), 0) >= 1, (kind, where, counts)
        assert counts.get((kind, "flip"), 0) >= KE.MIN_FLIP_ROWS, (kind, counts)
        assert counts.get((kind, "tie"), 0) >= KE.MIN_TIES[kind], (kind, counts)
        assert kind not in WALKS or counts.get((kind, "tie at 0"), 0) >= 1, (kind, counts)
    for bucket in "QR":
        for entry in KE.PROPOSAL_ENTRIES:
            assert ed.proposals.get((bucket, entry)), (bucket, entry)
    assert ed.proposals.get(("Q", "zero"))


def test_the_builder_against_the_restatement(oracle):
    ed = KE.edges(search=True)
    print_survey(ed)
    assert_survey(ed)
    for h in ed.handles():
        assert ed.restatement(h) is not None                        # asserts inside: every token as step() predicts, the counters, no prefix moves
    for row in ed.rows:
        lo, hi = row.own
        assert ed.knobs(hi)[KE.SLACK] == np.nextafter(ed.knobs(lo)[KE.SLACK], np.inf) and (ed.knobs(lo)[:KE.SLACK] == KE.ALPHA[:KE.SLACK]).all()
        (new_lo, det_lo), (new_hi, det_hi) = ed.at(row, lo), ed.at(row, hi)
        assert new_lo != new_hi and ed.past(row.kind, row.idx, det_lo["out"]) != ed.past(row.kind, row.idx, det_hi["out"]), ed.describe(row)
        for h in row.tags:                                          # `useful`, once more from outside
            assert ed.at(row, h, force=(row.kind, row.idx, False))[0] != ed.at(row, h, force=(row.kind, row.idx, True))[0], (ed.describe(row), h)
        m = det_lo["m"]
        if row.where == "63|64":                                    # the seam of a list of more than 64 entries
            assert row.idx == 63 and (row.kind != "c" or len(m["sc"]) > 64) and (row.kind != "d" or len(m["dlist"]) > 64)
            assert {det_lo["out"][2], det_hi["out"][2]} == {63, 64}
        if row.where == "zero behind":                              # the walk that goes on steps over the zero entry
            assert m["sc"][row.idx + 1] == 0.0 and {det_lo["out"][2], det_hi["out"][2]} == {row.idx, row.idx + 2}
        if row.where == "zero first":
            assert m["sc"][0] == 0.0 and {det_lo["out"][2], det_hi["out"][2]} == {1, 2}
        if row.where == "last two":
            assert {det_lo["out"][2], det_hi["out"][2]} == {len(m["sc"]) - 2, len(m["sc"]) - 1}
        if row.where == "last":
            assert {det_lo["out"][2], det_hi["out"][2]} == {len(m["dlist"]) - 2, len(m["dlist"]) - 1}
        if row.where == "K-2|K-1":
            assert {det_lo["out"][0], det_hi["out"][0]} == {KE.K - 2, KE.K - 1}
        if row.where == "raise":                                    # sample < Q, yet the walk stays positive: the clamped last entry, an error
            assert lo in ed.raises and det_lo.get("raised") and det_lo["out"][1:] == (KE.BQ, len(m["sc"]) - 1) and det_hi["out"][1] == KE.BR
        if row.where == "fallback":                                 # sample - Q < R, yet the walk stays positive: K - 1, no error
            assert det_hi["out"] == (KE.K - 1, KE.BR, len(m["dlist"])) and hi not in ed.raises and KE.K - 1 not in m["dlist"]
    assert ed.raises == {row.own[0] for row in ed.rows if row.where == "raise"}
    z = ed.walk_at(ed.base)[0]                                           # the proposal rows lie in the bucket and at the entry they are named for
    for (bucket, entry), toks in ed.proposals.items():
        for t in toks:
            d = int(np.searchsorted(ed.doc_ptr, t, side="right")) - 1
            det = ed.probe(d, t - int(ed.doc_ptr[d]), ed.knob[ed.base])[1]
            n = len(det["m"]["sc"] if bucket == "Q" else det["m"]["dlist"])
            assert det["out"][0] == z[t] and det["out"][1] == "QR".index(bucket)
            if entry == "zero":
                assert det["m"]["sc"][det["out"][2] - 1] == 0.0
            else:
                assert n > 64 and det["out"][2] == (n - 1 if entry == "last" else int(entry))


def test_the_recorded_rows_are_the_searchs(oracle):
    """tests/golden/adlda_knife_edge_rows.json names the candidates the search took (python -m tests.adlda_knife_edge writes
    it); the device test aims at those alone.  The corpus again from its seed, every row's own bisection again: the same
    rows, knob values, tags, expected z and proposal rows as the whole search gives."""
    one, two = KE.edges(search=True), KE.edges()
    assert one.record() == KE.recorded()
    assert np.array_equal(one.tokens, two.tokens) and np.array_equal(one.z0, two.z0) and np.array_equal(one.doc_ptr, two.doc_ptr) and one.U == two.U
    assert one.knob == two.knob and one.raises == two.raises and one.base == two.base and one.proposals == two.proposals
    assert [(r.kind, r.where, r.target, r.idx, r.own, sorted(r.tags.items())) for r in one.rows] == [
        (r.kind, r.where, r.target, r.idx, r.own, sorted(r.tags.items())) for r in two.rows]
    assert one.expect == two.expect and one.full_handles() == two.full_handles()
    for h in two.full_handles()[:2]:                                # the restatement's z as the recorded rows' builder returns it
        assert np.array_equal(one.restatement(h)[0], two.restatement(h)[0]) and (one.restatement(h)[1] == two.restatement(h)[1]).all()


def random_models(cats):
    for alpha, beta in ((5.0, 7.0), (0.1, 0.01)):
        yield "cats alpha %g beta %g" % (alpha, beta), R.Model(20, cats.num_types, alpha, beta, 777, cats.doc_ptr, cats.tokens,
                                                               java_lcg_initial_z(cats.num_tokens, 20, 5))


def random_corpus_changes(oracle, cats, slips, sweeps=2):
    """{slip: tokens that the slip draws otherwise, over `sweeps` z steps of each random model}; the unmutated step() is
    asserted to be the restatement's on the way"""
    changed, n = dict.fromkeys(slips, 0), 0
    for name, m in random_models(cats):
        for _ in range(sweeps):
            z, n_wk, n_k = m.z.copy(), m.n_wk.copy(), m.n_k.copy()
            U = [float(x) for x in oracle.uniforms(m.seed, m.iteration + 1, R.PURPOSE_Z, 0, z.size)]
            before = m.stats.copy()
            m.sweep(1)
            stats, raised, ch = KE.z_step(m.doc_ptr, m.tokens, z, n_wk, n_k, m.alpha, m.beta, U, slips)
            assert not raised and (z == m.z).all() and stats == (m.stats - before).tolist(), name
            n += z.size
            for s in slips:
                changed[s] += ch[s]
    return changed, n


def test_every_slip_shows_on_the_edge_rows_and_none_on_the_random_data(oracle, cats):
    ed = KE.edges(search=True)
    edge = {}
    for slip, kinds in KE.SLIPS.items():
        moved = set()
        for row in ed.rows:
            if row.kind in kinds:
                for h, tag in row.tags.items():
                    if ed.at(row, h, slip=slip)[0] != ed.at(row, h)[0]:
                        moved.add((row.target, row.kind, tag))
        edge[slip] = moved
    rand, n = random_corpus_changes(oracle, cats, tuple(KE.SLIPS))
    for slip, kinds in KE.SLIPS.items():
        print("slip %-16s (%-5s): changes %2d edge rows (comparisons %s, tags %s); %d of the %d random draws" % (
            slip, kinds, len({r for r, _, _ in edge[slip]}), "".join(sorted({k for _, k, _ in edge[slip]})), sorted({t for _, _, t in edge[slip]}), rand[slip], n))
    for slip in KE.SLIPS:
        assert edge[slip], "slip %s moves no edge row of the comparisons %s" % (slip, KE.SLIPS[slip])
    for slip in KE.ORDER_SLIPS:
        assert rand[slip] == 0, "slip %s shows on the random data: %d tokens" % (slip, rand[slip])
    for slip in KE.INDEX_SLIPS:                                     # what the random corpora of the device suite can tell already
        assert rand[slip] > 0
    # the comparison slips show exactly where the two sides are equal
    for slip in ("q_le", "r_le", "qwalk_ge", "rwalk_lt", "swalk_ge"):
        assert {t for _, _, t in edge[slip]} == {"tie"}, (slip, edge[slip])
