"""The knife-edge rows of scheme=lightcollapsed (tests/lightcollapsed_knife_edge.py) on the CPU: the builder against the
restatement, and the POWER of the rows -- each deliberately wrong variant of the token step (KE.SLIPS: the cancelling
quotients of pi_w cancelled, another association, <= for <, >= for >, a cell multiplied first, the table's fraction
fused, the t_is_z0 decrement forgotten, a wrong alpha) moves the new topic of a target of its own comparison, while on
the random corpora of tests/test_lightcollapsed_gpu.py (the ragged one and cats) the order and comparison slips move
nothing at all: such a kernel differs from the restatement about once in 2^50 draws, and only rows put on the edge can
tell.  tests/test_lightcollapsed_knife_edge_gpu.py puts the same rows through the device.  The last test puts the
table build on ITS edge: words whose topics all weigh the same."""
import numpy as np
import pytest

from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import lightcollapsed_knife_edge as KE
from tests import lightcollapsed_restatement as R
from tests.test_lightcollapsed_model import implied_dense

RANDOM_STEPS = 3                                                    # z steps of each random corpus the slips are tried on
FAMILIES = ("alpha", "beta")


def print_survey(counts):
    print("rows reached per (comparison, tag): %s" % sorted((k, v) for k, v in counts.items() if len(k) == 2))
    print("g rows per (dt source, state): %s" % sorted((k[1:], v) for k, v in counts.items() if len(k) == 3))


def assert_survey(counts):
    """the minimums of tests/lightcollapsed_knife_edge.py: conditions on the inputs, not measurements"""
    for tag in KE.TAGS:
        for kind in "dg":
            assert counts.get((kind, tag), 0) >= KE.MIN_PER_CATEGORY, (kind, tag, counts)
        for kind in "abcef":
            assert counts.get((kind, tag), 0) >= KE.MIN_GLOBAL_ROWS, (kind, tag, counts)
    for src in KE.SOURCES:
        for state in KE.STATES:
            assert counts.get(("g", src, state), 0) >= KE.MIN_PER_SOURCE, (src, state, counts)


def test_the_builder_against_the_restatement(oracle):
    ae, be = KE.edges("alpha"), KE.edges("beta")
    for ed in (ae, be):
        assert len(ed.handles()) <= KE.MAX_HANDLES
        for h in ed.handles():
            assert ed.restatement(h) is not None                    # asserts inside: every token as step() predicts, no prefix moves
        for row in ed.rows:                                         # every aimed row carries a tag and has its flip pair
            assert (row.kind == "plain") == (not row.tags), ed.describe(row)
            if row.kind != "plain":
                outs = {repr(ed.outcome(row, ed.at(row, h)[1])) for h in row.tags}
                assert len(outs) >= 2 and set(row.tags.values()) - {"-"}, ed.describe(row)
                for h in row.tags:                                  # `useful`, once more from outside
                    one, two = ed.both_sides(row)
                    assert ed.at(row, h, force=one)[0] != ed.at(row, h, force=two)[0], (ed.describe(row), h)
    counts = dict(list(ae.survey().items()) + list(be.survey().items()))
    print_survey(counts)
    print("handles: %d alpha vectors, %d beta values; f cells %s, c cells %s" % (len(ae.handles()), len(be.handles()), ae.cells,
                                                                              sorted(r.m for r in be.rows if r.kind == "c")))
    assert_survey(counts)
    for row in ae.rows:                                             # e and f rows carry all three tags
        assert row.kind not in "ef" or set(row.tags.values()) == set(KE.TAGS), ae.describe(row)
    assert ae.cells[0] == ae.nK - 1 and min(ae.cells) <= 3 and len(ae.cells) == 4      # last, first (see the builder), two middle ones
    cs = sorted(r.m for r in be.rows if r.kind == "c")
    assert cs[0] <= 3 and cs[-1] == be.nK - 1 and len(cs) == 3
    g = [r for r in ae.rows if r.kind == "g"]
    lanes = {("lane 0", "lane 63", "other")[(0, 63).index(r.pos % 64) if r.pos % 64 in (0, 63) else 2] for r in g}
    assert lanes == {"lane 0", "lane 63", "other"}
    assert any(r.pos >= 64 and r.source == "earlier" for r in g) and any(r.pos >= 64 and r.source == "chunk" for r in g)
    at = [sum(r.pos == p for r in g) for p in (0, 63, 64, 127)]     # a chunk's first and last lane, in the first chunk and behind it
    print("g rows at positions 0 / 63 / 64 / 127: %s" % at)
    assert min(at) >= 1
    b = [r for r in be.rows if r.kind == "b"]
    assert any(r.nnz > 64 for r in b) and all(1 < r.nnz < be.nK for r in b)
    for r in b:                                                     # i indexes the list and not the topic
        assert be.table(r.word, KE.BETA)[2][r.cell] != r.cell
    assert any(r.cell == 0 for r in b) and any(r.cell > 0 for r in b)
    d = [r for r in ae.rows if r.kind == "d"]                       # word proposals from the table and from the beta branch
    assert {ae.at(r, next(iter(r.tags)))[1]["tb"] for r in d} == {True, False}


def test_the_same_seed_gives_the_same_rows(oracle):
    for name, cls in (("alpha", KE.AlphaEdges), ("beta", KE.BetaEdges)):
        one, two = KE.edges(name), cls()
        assert np.array_equal(one.tokens, two.tokens) and np.array_equal(one.z0, two.z0) and np.array_equal(one.doc_ptr, two.doc_ptr)
        assert [(r.kind, r.target, sorted(r.tags.items())) for r in one.rows] == [(r.kind, r.target, sorted(r.tags.items())) for r in two.rows]
        assert [one.knobs(h)[1:] for h in one.handles()] == [two.knobs(h)[1:] for h in two.handles()]
        assert all(one.knobs(h)[0] == two.knobs(h)[0] for h in one.handles())


def random_models(cats):
    doc_ptr, tokens = KE.ragged_corpus()
    g = KE.RAGGED
    yield "ragged", R.Model(g["K"], g["V"], g["alpha"], g["beta"], g["seed"], doc_ptr, tokens, java_lcg_initial_z(len(tokens), g["K"], g["zseed"]))
    alpha = 0.02 + 0.07 * np.arange(20)
    yield "cats", R.Model(20, cats.num_types, alpha, 0.01, 777, cats.doc_ptr, cats.tokens, java_lcg_initial_z(cats.num_tokens, 20, 5))


def random_corpus_changes(cats, slips):
    """{slip: tokens whose topic differs from the restatement's, summed over RANDOM_STEPS z steps of each random corpus};
    the unmutated step() is asserted to be the restatement's on the way."""
    changed = dict.fromkeys(slips, 0)
    n = 0
    for name, m in random_models(cats):
        for _ in range(RANDOM_STEPS):
            zb, it = m.z.copy(), m.iteration + 1
            U = [R.token_uniforms(m.seed, it, t) for t in range(len(m.tokens))]
            n_wk, n_k, tables = m.n_wk.copy(), m.n_k.copy(), m.tables()
            m.sweep(1)
            for slip in (None,) + tuple(slips):
                z = zb.copy()
                out = KE.z_step(m.doc_ptr, m.tokens, z, n_wk, n_k, m.alpha, m.beta, tables, U, slip)
                if slip is None:
                    assert out == 0 and (z == m.z).all(), name
                    n += z.size
                else:
                    changed[slip] += out + int((z != m.z).sum())
    return changed, n


def test_the_unmutated_step_equals_the_restatement(oracle, cats):
    n = 0
    for name in FAMILIES:
        ed = KE.edges(name)
        for h in ed.handles():
            alpha, total, beta = ed.knobs(h)
            tb = ed.built(beta)
            for row in ed.rows:
                nn, zdoc = ed.state(row, ed.walks[h])
                w = row.word
                G, T = ed.n_wk[w].tolist(), list(ed.T)
                det = {}
                R.token_step(list(nn), list(zdoc), row.pos, G, T, alpha, total, beta, beta * float(ed.V),
                             (tb[0][w], tb[1][w], tb[4][w], int(tb[3][w]), int(tb[5][w])), row.U, det)
                assert ed.at(row, h)[0] == det["new"], (ed.describe(row), h)
                n += 1
    _, tokens = random_corpus_changes(cats, ())
    print("step() equals R.token_step on %d (row, knob value) pairs and on %d tokens of the random corpora" % (n, tokens))


def test_every_slip_shows_on_the_edge_rows_and_none_on_the_random_corpus(oracle, cats):
    by_kind = {k: KE.edges("alpha") for k in "defg"}
    by_kind.update({k: KE.edges("beta") for k in "abc"})
    edge = {}
    for slip, kind in KE.SLIPS.items():
        ed = by_kind[kind]
        rows = set()
        for row in ed.rows:
            if row.kind == kind:
                for h, tag in row.tags.items():
                    if tag != "-" and ed.at(row, h, slip=slip)[0] != ed.at(row, h)[0]:
                        rows.add((row.target, tag))
        edge[slip] = rows
    rand, _ = random_corpus_changes(cats, tuple(KE.SLIPS))
    for slip, kind in KE.SLIPS.items():
        tags = sorted({t for _, t in edge[slip]})
        print("slip %-21s (%s): changes %3d edge rows (tags %s); %d tokens of the random corpora in %d steps each" % (
            slip, kind, len({r for r, _ in edge[slip]}), tags, rand[slip], RANDOM_STEPS))
    for slip in KE.SLIPS:
        assert edge[slip], "slip %s moves no edge row of comparison %s" % (slip, KE.SLIPS[slip])
    for slip in KE.ORDER_SLIPS:
        assert rand[slip] == 0, "slip %s shows on the random corpora: %d tokens" % (slip, rand[slip])
    # the comparison slips show exactly where the two sides are equal
    for slip in ("branch_le", "alias_ge", "word_le", "len_le", "doc_le"):
        assert {t for _, t in edge[slip]} == {"tie"}, (slip, edge[slip])


# ---- the table build on its edge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.01, 0.1, 0.37])
def test_equal_count_tables_imply_the_normalised_probabilities(beta):
    n_wk, n_k = KE.equal_count_words()
    assert len(set(n_k.tolist())) == 1
    V = n_wk.shape[0]
    seen = set()
    for i, nnz in enumerate(KE.EQUAL_NNZ):
        lst, ps, a, mass, tot = R.word_table(n_wk[i].tolist(), n_k.tolist(), beta * V)
        assert len(lst) == nnz and tot == nnz * (1 + i % 3)
        p = np.array([n_wk[i, k] / (n_k[k] + beta * V) for k in lst])
        assert len(set(p.tolist())) == 1
        bs = p / mass - 1.0 / nnz
        assert np.abs(bs).max() <= 2.0 ** -52, bs                   # +-0, or one rounding away
        seen.add("zero" if not bs.any() else "below" if (bs < 0).all() else "above" if (bs > 0).all() else "mixed")
        assert np.abs(implied_dense(ps, a) - p / mass).max() < 1e-12
        assert np.abs(implied_dense(ps, a) - 1.0 / nnz).max() < 1e-12
        assert ((0 <= a) & (a < nnz)).all() and (ps <= 1.0).all() and (ps >= 1.0 - nnz * 2.0 ** -51).all()
    print("beta %g: bs of the equal-count words: %s" % (beta, sorted(seen)))
