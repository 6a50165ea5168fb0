"""The hot words' pair-chunks (csrc/ggs_corpus_lists.hpp, hot_pair_lists; z_pairs_kernel reads them) without a GPU: a short
driver (tests/hot_pair_lists_driver.cpp) is compiled with the host compiler, builds the lists with and without the
pair-chunks and prints the former: every hot token in exactly one chunk's token list, a chunk's pairs distinct, in
(document, row) order and of at most kHotPairDocs documents, each token's pair lane naming its own document and word, token
counts and the cap respected, a pair's tokens never split (a pair of more tokens than the cap: once per cap of them, each
piece in a chunk of its own), and every other list the same as without them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.hot_pairs_cases import HOT, edges_corpus
from tests.test_corpus_lists_cpu import corpora, doc_of_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc")

SHAPES = {
    "hot12_warm": dict(hot_cap=12, warm_cap=16, warm_docs=6, warm_tiers_max=3, warm_min_fill_pct=40, warm_min_chunks_per_wave=3, sliced_waves=4),
    "hot40": dict(hot_cap=40, warm_cap=0, warm_docs=2, warm_tiers_max=3, warm_min_fill_pct=40, warm_min_chunks_per_wave=3, sliced_waves=1024),
    "hot_edges": dict(hot_cap=HOT, warm_cap=0, warm_docs=2, warm_tiers_max=0, warm_min_fill_pct=40, warm_min_chunks_per_wave=3, sliced_waves=4),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("hot_pair_lists") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "hot_pair_lists_driver.cpp"), "-o", exe])
    return exe


def run(driver, tmp_path, c, shape):
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        np.array([c.num_docs, c.num_tokens], np.int64).tofile(f)
        c.doc_ptr.astype(np.int64).tofile(f)
        c.tokens.astype(np.int32).tofile(f)
    args = ["%s=%d" % kv for kv in dict(shape, V=c.num_types).items()]
    out = subprocess.run([driver, path] + args, check=True, capture_output=True, text=True).stdout
    L = {}
    for line in out.splitlines():
        name, n, *vals = line.split()
        L[name] = np.array(vals, np.int64)
        assert len(L[name]) == int(n)
    for k in list(L):
        if k not in ("inv", "hot_words", "hp_pair", "hp_docs", "hp_tok"):
            L[k] = int(L[k][0])
    return L


def check_pair_chunks(c, L):
    """Every invariant of the pair-chunk lists; returns per chunk (pairs, tokens)."""
    N, doc_of = c.num_tokens, doc_of_tokens(c)
    slots, cap, lane_shift, slot_shift = L["kWarmDocSlots"], L["kHotPairTokenCap"], L["kHotPairLaneShift"], L["kWarmSlotShift"]
    maxdocs = L["kHotPairDocs"]
    Cp, hot_words = L["Cp"], L["hot_words"]
    assert len(L["hp_pair"]) == 64 * Cp and len(L["hp_docs"]) == slots * Cp and len(L["hp_tok"]) % 256 == 0
    tok = L["hp_tok"].reshape(-1, 4)
    seen = np.zeros(N, np.int64)
    entries = {}                                                   # (document, row) -> [(chunk, tokens of the entry, pairs of its chunk)]
    rounds, sizes = 0, []
    for ch in range(Cp):
        meta = L["hp_docs"][slots * ch:slots * (ch + 1)]
        ntok, npairs, round0 = int(meta[L["kHotPairTokSlot"]]), int(meta[L["kHotPairCountSlot"]]), int(meta[L["kHotPairRoundSlot"]])
        assert 1 <= npairs <= 64 and npairs <= ntok <= cap, "pair and token counts, the cap"
        assert round0 == rounds, "a chunk's token rounds follow the chunk before's"
        nr = -(-ntok // 64)
        rounds += nr
        pairs = L["hp_pair"][64 * ch:64 * ch + 64]
        assert (pairs[npairs:] == 0).all()
        p = pairs[:npairs]
        slot, row = p >> slot_shift, p & ((1 << slot_shift) - 1)
        assert (np.diff(p) > 0).all(), "distinct pairs in (document, row) order"
        assert slot.max() < maxdocs and (row < len(hot_words)).all()
        docs = meta[:maxdocs]
        used = int(slot.max()) + 1
        assert (np.diff(docs[:used]) > 0).all() and (docs[used:] == docs[0]).all(), "consecutive documents in order, unused slots repeat the first"
        assert set(slot) == set(range(used)), "a document of the chunk has a pair in it"
        t = tok[64 * round0:64 * (round0 + nr)]
        act, idle = t[:ntok], t[ntok:]
        assert (act[:, 1] >= 0).all() and (idle == np.array([0, -1, 0, 0])).all(), "active lanes are a prefix, a chunk's rounds are whole"
        lane, word = act[:, 0] >> lane_shift, act[:, 0] & ((1 << lane_shift) - 1)
        assert lane.max() < npairs and (word == p[lane]).all(), "a token's lane is its pair's"
        assert (np.diff(lane) >= 0).all() and set(lane) == set(range(npairs)), "tokens in pair order, no pair without a token"
        idx = act[:, 1]
        assert (doc_of[idx] == docs[slot[lane]]).all() and (c.tokens[idx] == hot_words[row[lane]]).all(), "the pair names the token's document and word"
        assert (act[:, 2] == L["inv"][idx]).all() and (act[:, 3] == 0).all()
        seen[idx] += 1
        for j in range(npairs):
            entries.setdefault((int(docs[slot[j]]), int(row[j])), []).append((ch, int((lane == j).sum()), npairs))
        sizes.append((npairs, ntok))
    assert rounds * 64 == len(tok)
    hot = np.isin(c.tokens, hot_words)
    assert (seen[hot] == 1).all() and (seen[~hot] == 0).all(), "every hot token in exactly one chunk's token list, no other token"
    # a pair's tokens are never split -- but for a pair of more than the cap: whole caps, each alone in its chunk, then the rest
    row_of = np.full(c.num_types, -1)
    row_of[hot_words] = np.arange(len(hot_words))
    for (d, r), ent in entries.items():
        n = int(((doc_of == d) & (row_of[c.tokens] == r)).sum())
        assert sum(e[1] for e in ent) == n
        if n <= cap:
            assert len(ent) == 1, "a pair's tokens are in one chunk"
        else:
            assert [e[1] for e in ent] == [cap] * (n // cap) + ([n % cap] if n % cap else [])
            assert all(e[2] == 1 for e in ent if e[1] == cap) and len(set(e[0] for e in ent)) == len(ent)
    return sizes


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
@pytest.mark.parametrize("sname", ["hot12_warm", "hot40"])
def test_pair_chunks(driver, tmp_path, cname, c, sname):
    L = run(driver, tmp_path, c, SHAPES[sname])
    assert L["old_lists_same"] == 1, "the cold / hot / warm lists are what they are without the pair-chunks"
    assert L["absent_without"] == 1, "no pair-chunks unless asked for"
    check_pair_chunks(c, L)
    assert (L["Cp"] > 0) == (L["Cs"] > L["Cc"])


def test_pair_chunk_edges(driver, tmp_path):
    c = edges_corpus()
    L = run(driver, tmp_path, c, SHAPES["hot_edges"])
    assert L["old_lists_same"] == 1 and sorted(L["hot_words"]) == list(range(HOT))
    sizes = check_pair_chunks(c, L)
    cap = L["kHotPairTokenCap"]
    # the edge rows, as the builder cuts them (documents in order; see edges_corpus):
    assert cap == 256
    want = [
        (1, 256),        # one word 300 times: a piece of the cap, alone
        (64, 44 + 63),   # ... its rest, and 63 of the next non-empty document's 64 distinct words: 64 pairs across two documents
        (64, 64),        # that document's last word and 63 of the next one's 65: 64 pairs, 64 tokens, every pair one token
        (3, 3),          # its last two words and the document of one hot token (a third document would be one too many)
        (41, 41),        # the other document of one hot token, and 40 distinct words
        (64, 64),        # 24 words and 40 of the next document's 41: closed by the pair count
        (25, 25),        # the 41st and the next document's 24
        (64, 256),       # 32 words x 4 and 32 words x 4 of the next: 64 pairs and 64 x 4 tokens, both limits at once
        (64, 65),        # its 33rd word (the last row: one token) and 63 pairs of the last edge document, one of them twice: 64 + 1 tokens
    ]
    assert sizes[:len(want)] == want
    assert max(p for p, _ in sizes) == 64 and max(t for _, t in sizes) == cap
