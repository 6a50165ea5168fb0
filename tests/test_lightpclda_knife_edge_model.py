"""The knife-edge rows of scheme=lightpclda (tests/lightpclda_knife_edge.py) on the CPU: the builder against the
restatement, and the POWER of the rows -- each deliberately wrong variant of the token step (KE.SLIPS: another
association, the division first, >= for >, <= for <, the alpha cell multiplied first, alpha[z0] after an accepted word
proposal) moves the new topic of a target of its own comparison, while on the random corpus of
tests/test_lightpclda_gpu.py::test_ragged_corpus the order and comparison slips move nothing at all: with four 53-bit
uniforms per token such a kernel differs from the restatement with probability about 2^-52 per token, and only rows put
on the edge can tell.  tests/test_lightpclda_knife_edge_gpu.py puts the same rows through the device."""
import numpy as np

from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z
from tests import lightpclda_knife_edge as KE
from tests import lightpclda_restatement as R
from tests import spalias_restatement as SR

RANDOM_STEPS = 3                                                    # z steps of the random corpus the slips are tried on


def handles(ed):
    """(scan value or vector, Phi, alpha) for every z step the rows are put through"""
    if isinstance(ed, KE.AlphaEdges):
        return [(v, ed.phi, ed.vectors[v]) for v in range(KE.N_VECTORS)]
    return [(j, ed.phi(j), KE.ALPHA) for j in range(2 * KE.SCAN + 1)]


def test_the_builder_against_the_restatement(oracle):
    pe, ae, al = KE.edges("phi"), KE.edges("alpha"), KE.edges("alias")
    for ed in (pe, ae):
        for h, _, _ in handles(ed):
            assert ed.restatement(h) is not None                    # asserts inside: no one-hot token moves, every target as predicted
        for row in ed.rows:                                         # every aimed row carries its tag
            assert (row.kind == "plain") == (not row.tags), ed.describe(row)
    counts = dict(list(pe.survey().items()) + list(ae.survey().items()))
    print("rows reached per (comparison, tag): %s" % sorted((k, v) for k, v in counts.items() if len(k) == 2))
    print("e rows per (dt source, after an accepted word proposal): %s" % sorted((k[1:], v) for k, v in counts.items() if len(k) == 3))
    for tag in KE.TAGS:
        for kind in "abe":
            assert counts.get((kind, tag), 0) >= KE.MIN_PER_CATEGORY, (kind, tag, counts)
        for kind in "cd":
            assert counts.get((kind, tag), 0) >= KE.MIN_ALPHA_ROWS, (kind, tag, counts)
    for src in KE.SOURCES:
        for after in (False, True):
            assert counts.get(("e", src, after), 0) >= KE.MIN_PER_SOURCE, (src, after, counts)
    assert len(ae.vectors) <= KE.MAX_HANDLES
    # flip pairs everywhere: c and d rows carry all three tags (below / tie is the pair of c, below / tie that of d), b
    # rows "above" and one of the others; a and e rows have theirs by construction (PhiEdges._classify)
    for row in ae.rows:
        have = set(row.tags.values())
        assert row.kind == "plain" or (have == set(KE.TAGS) if row.kind in "cd" else "above" in have and len(have) > 1), ae.describe(row)
    assert sorted(row.m for row in ae.rows if row.kind == "d") == sorted(ae.CELLS)
    lanes = {("lane 0", "lane 63", "other")[(0, 63).index(r.pos % 64) if r.pos % 64 in (0, 63) else 2] for r in pe.rows if r.kind == "e"}
    assert lanes == {"lane 0", "lane 63", "other"} and any(r.pos >= 64 for r in pe.rows if r.kind == "e")
    assert any(r.pos >= 64 and r.source == "earlier" for r in pe.rows if r.kind == "e")
    n_alias = sum(r.kind == "a" for r in al.rows)
    assert n_alias >= KE.MIN_PER_CATEGORY and all(r.tags for r in al.rows if r.kind == "a")
    print("one-token alias rows for spalias: %d" % n_alias)


def test_the_same_seed_gives_the_same_rows(oracle):
    for name, cls in (("phi", KE.PhiEdges), ("alpha", KE.AlphaEdges)):
        one, two = KE.edges(name), cls()
        assert np.array_equal(one.tokens, two.tokens) and np.array_equal(one.z0, two.z0) and np.array_equal(one.doc_ptr, two.doc_ptr)
        assert [(r.kind, r.target, sorted(r.tags.items())) for r in one.rows] == [(r.kind, r.target, sorted(r.tags.items())) for r in two.rows]
        if name == "phi":
            assert all(np.array_equal(one.phi(j), two.phi(j)) for j in (0, KE.SCAN, 2 * KE.SCAN))
        else:
            assert np.array_equal(one.phi, two.phi) and np.array_equal(np.array(one.vectors), np.array(two.vectors))


def test_the_unmutated_step_equals_the_restatement(oracle):
    n = 0
    for ed in (KE.edges("phi"), KE.edges("alpha")):
        for h, phi, alpha in handles(ed):
            alpha = np.broadcast_to(alpha, (ed.nK,))
            for row in ed.rows:
                col = phi[:, row.word]
                ps, a, _ = SR.alias_table(col * alpha)
                det = {}
                R.token_step(list(row.n), list(row.zdoc), row.pos, col, alpha, R.alpha_sum(alpha, ed.nK), ps, a, row.U, det)
                assert ed.eval(row, col, alpha)[0] == det["new"], (ed.describe(row), h)
                n += 1
    print("step() equals R.token_step on %d (row, scan value or vector) pairs" % n)


def random_corpus_changes():
    """{slip: tokens whose topic differs from the restatement's, summed over RANDOM_STEPS z steps of the ragged corpus}"""
    doc_ptr, tokens = KE.ragged_corpus()
    g = KE.RAGGED
    m = KE.ragged_model(java_lcg_initial_z(len(tokens), g["K"], g["zseed"]))
    changed = dict.fromkeys(KE.SLIPS, 0)
    for _ in range(RANDOM_STEPS):
        zb, it = m.z.copy(), m.iteration + 1
        U = [R.token_uniforms(g["seed"], it, t) for t in range(len(tokens))]
        phi, tables = m.phi, m.tables
        m.sweep(1)
        for slip in (None,) + tuple(KE.SLIPS):
            z = zb.copy()
            out = KE.z_step(doc_ptr, tokens, z, phi, g["alpha"], tables, g["seed"], it, slip, U)
            if slip is None:
                assert out == 0 and (z == m.z).all()                # the unmutated step is the restatement's here too
            else:
                changed[slip] += out + int((z != m.z).sum())
    return changed


def test_every_slip_shows_on_the_edge_rows_and_none_on_the_random_corpus(oracle):
    by_kind = {"a": KE.edges("phi"), "e": KE.edges("phi"), "b": KE.edges("alpha"), "c": KE.edges("alpha"), "d": KE.edges("alpha")}
    edge = {}
    for slip, kind in KE.SLIPS.items():
        ed = by_kind[kind]
        rows = set()
        for h, phi, alpha in handles(ed):
            for row in ed.rows:
                if row.kind == kind and h in row.tags:
                    col = phi[:, row.word]
                    if ed.eval(row, col, alpha, slip=slip)[0] != ed.eval(row, col, alpha)[0]:
                        rows.add((row.target, row.tags[h]))
        edge[slip] = rows
    rand = random_corpus_changes()
    for slip, kind in KE.SLIPS.items():
        tags = sorted({t for _, t in edge[slip]})
        print("slip %-15s (%s): changes %3d edge rows (tags %s); %d tokens of the random corpus in %d steps" % (
            slip, kind, len({r for r, _ in edge[slip]}), tags, rand[slip], RANDOM_STEPS))
    for slip in KE.SLIPS:
        assert edge[slip], "slip %s moves no edge row of comparison %s" % (slip, KE.SLIPS[slip])
    for slip in KE.ORDER_SLIPS:
        assert rand[slip] == 0, "slip %s shows on the random corpus: %d tokens" % (slip, rand[slip])
    # the comparison slips show exactly where the two sides are equal
    for slip in ("alias_ge", "word_le", "doc_le", "len_le"):
        assert {t for _, t in edge[slip]} == {"tie"}, (slip, edge[slip])
