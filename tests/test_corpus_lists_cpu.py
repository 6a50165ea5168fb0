"""The host half of ggs_set_corpus (csrc/ggs_corpus_lists.hpp) without a GPU: a short driver
(tests/corpus_lists_driver.cpp) is compiled with the host compiler and the lists it prints are checked against the
corpus -- every token in exactly one of the cold / hot / warm lists, chunk sizes and document limits, active lanes a
prefix, the two-row chunk table a gapless cover, the pcgs order a permutation, the warm tiers' keep rule."""
import hashlib
import os
import shutil
import subprocess

import numpy as np
import pytest

from ldagroupedgibbssampler_amd.corpus import Corpus, random_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ldagroupedgibbssampler_amd", "csrc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("corpus_lists") / "driver")
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "corpus_lists_driver.cpp"), "-o", exe])
    return exe


def with_long_document(c, length, seed):
    """c with one document of `length` tokens appended by hand."""
    rng = np.random.default_rng(seed)
    extra = rng.integers(0, c.num_types, length).astype(np.int32)
    return Corpus(np.append(c.doc_ptr, c.doc_ptr[-1] + length).astype(np.int64), np.concatenate([c.tokens, extra]), c.num_types)


def corpora():
    # empty documents (every 7th, and the first and last), documents longer than 64 tokens, one longer than 32 767
    a = random_corpus(300, 500, 150, seed=11, empty_every=7)
    b = random_corpus(2000, 3000, 90, seed=12, empty_every=5)
    c = with_long_document(random_corpus(120, 400, 100, seed=13, empty_every=9), 40000, seed=14)
    d = random_corpus(1, 50, 0, seed=15)                 # one empty document: no token at all
    return [("ragged", a), ("many_docs", b), ("long_doc", c), ("empty", d)]


SHAPES = {
    # a hot table of 12 rows, warm tiers of 16 rows on one "CU" (4 waves): tiers are kept on the small corpora
    "sliced": dict(sliced=1, hot_cap=12, warm_cap=16, warm_docs=6, warm_tiers_max=3, warm_min_fill_pct=40, warm_min_chunks_per_wave=3, sliced_waves=4,
                   tile_tokens=64),
    "sliced_no_warm": dict(sliced=1, hot_cap=40, warm_cap=0, warm_docs=2, warm_tiers_max=3, warm_min_fill_pct=40, warm_min_chunks_per_wave=3, sliced_waves=1024,
                           tile_tokens=64),
    "two_rows": dict(two_rows=1, tile_tokens=64, z_parts=4),
    "tile": dict(tile_tokens=23, z_parts=1),
    "pcgs": dict(pcgs=1, pcgs_waves=3, tile_tokens=64),          # 3 resident waves: 4..6 groups of 64 documents get the padded order
    "pcgs_wide": dict(pcgs=1, pcgs_waves=1024, tile_tokens=64),
}


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
    L["lines"] = {line.split()[0]: line for line in out.splitlines()}
    for k in ("kChunkDocs", "kSlotShift", "kWarmSlotShift", "kWarmDocSlots", "kPcgsMaxDocLen", "kSegTokens", "longest", "Cc", "Cs", "warm_tiers", "num_warm",
              "warm_rows_max", "Cw", "warm_chunks_max"):
        L[k] = int(L[k][0])
    return L


def doc_of_tokens(c):
    return np.repeat(np.arange(c.num_docs), np.diff(c.doc_ptr))


def check_chunks(c, tok, idx, docs, docslots, maxdocs, shift, word_of_value, seen):
    """A chunk list of 64 lanes per chunk: active lanes a prefix, <= maxdocs documents, each lane's slot names its token's
    document, each value its token's word; marks the tokens in `seen`."""
    doc_of = doc_of_tokens(c)
    nch = len(tok) // 64
    assert len(tok) == len(idx) == 64 * nch and len(docs) == nch * docslots
    for ch in range(nch):
        i = idx[64 * ch:64 * ch + 64]
        n = int((i >= 0).sum())
        assert 1 <= n <= 64
        assert (i[:n] >= 0).all() and (i[n:] == -1).all(), "active lanes are a prefix"
        t = tok[64 * ch:64 * ch + n]
        slot, value = t >> shift, t & ((1 << shift) - 1)
        d = docs[ch * docslots:(ch + 1) * docslots]
        assert slot.max() < maxdocs and len(np.unique(doc_of[i[:n]])) <= maxdocs
        assert (d[slot] == doc_of[i[:n]]).all(), "a lane's slot names its token's document"
        assert (word_of_value(value) == c.tokens[i[:n]]).all()
        assert (np.diff(t.astype(np.uint32).astype(np.int64)) >= 0).all(), "lanes in (document, row) order"
        seen[i[:n]] += 1


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
@pytest.mark.parametrize("sname", ["sliced", "sliced_no_warm"])
def test_sliced_lists(driver, tmp_path, cname, c, sname):
    shape = SHAPES[sname]
    L = run(driver, tmp_path, c, shape)
    N = c.num_tokens
    seen = np.zeros(N, np.int64)
    Cc, Cs = L["Cc"], L["Cs"]
    assert len(L["ct_tok"]) == 64 * Cs and len(L["c_docs"]) == L["kChunkDocs"] * Cs
    hot_words, warm_words = L["hot_words"], L["warm_words"]
    # hot words: the most frequent, at most hot_cap, no word of count 0
    freq = np.bincount(c.tokens, minlength=c.num_types)
    assert len(hot_words) <= shape["hot_cap"] and (freq[hot_words] > 0).all()
    if len(hot_words):
        rest = np.setdiff1d(np.arange(c.num_types), hot_words)
        assert freq[hot_words].min() >= (freq[rest].max() if len(rest) else 0)
    kd = L["kChunkDocs"]
    check_chunks(c, L["ct_tok"][:64 * Cc], L["ct_idx"][:64 * Cc], L["c_docs"][:kd * Cc], kd, kd, L["kSlotShift"], lambda v: v, seen)
    check_chunks(c, L["ct_tok"][64 * Cc:], L["ct_idx"][64 * Cc:], L["c_docs"][kd * Cc:], kd, kd, L["kSlotShift"], lambda v: hot_words[v], seen)
    # the same hot chunks in the packed form
    hp = L["ht_pack"].reshape(-1, 4)
    assert len(hp) == 64 * (Cs - Cc)
    hidx = L["ct_idx"][64 * Cc:]
    assert (hp[:, 1] == hidx).all() and (hp[:, 3] == 0).all()
    act = hidx >= 0
    assert (hp[act, 2] == L["inv"][hidx[act]]).all()
    ht = L["ct_tok"][64 * Cc:]
    assert (hp[act, 0] == ((ht[act] & ((1 << L["kSlotShift"]) - 1)) | ((ht[act] >> L["kSlotShift"]) << L["kWarmSlotShift"]))).all()
    assert len(L["h_docs"]) == L["kWarmDocSlots"] * (Cs - Cc)
    # place in the word-sorted order
    cact = L["ct_idx"] >= 0
    assert (L["ct_ip"][cact] == L["inv"][L["ct_idx"][cact]]).all()
    # warm tiers
    tiers, cap = L["warm_tiers"], shape["warm_cap"]
    if tiers:
        meta = L["warm_meta"]
        assert len(meta) == 2 * tiers + 1 and meta[0] == 0 and meta[tiers] == L["Cw"] and tiers <= shape["warm_tiers_max"]
        wp = L["wt_pack"].reshape(-1, 4)
        assert len(wp) == 64 * L["Cw"] and len(L["w_docs"]) == L["kWarmDocSlots"] * L["Cw"]
        for t in range(tiers):
            a, b = int(meta[t]), int(meta[t + 1])
            rows = int(meta[tiers + 1 + t])
            assert 1 <= rows <= cap
            words = warm_words[t * cap:t * cap + rows]
            before = seen.sum()
            check_chunks(c, wp[64 * a:64 * b, 0], wp[64 * a:64 * b, 1], L["w_docs"][L["kWarmDocSlots"] * a:L["kWarmDocSlots"] * b], L["kWarmDocSlots"],
                         shape["warm_docs"], L["kWarmSlotShift"], lambda v: words[v], seen)
            ntok, nch = seen.sum() - before, b - a
            # the keep rule: enough chunks per resident wave, chunks full enough
            assert nch >= shape["warm_min_chunks_per_wave"] * shape["sliced_waves"]
            assert ntok * 100 >= nch * 64 * shape["warm_min_fill_pct"]
            assert L["warm_chunks_max"] >= nch and L["warm_rows_max"] >= rows
        wact = wp[:, 1] >= 0
        assert (wp[wact, 2] == L["inv"][wp[wact, 1]]).all()
        assert L["num_warm"] == int(meta[tiers + 1:].sum())
        assert len(np.intersect1d(hot_words, warm_words[:L["num_warm"]])) == 0
    else:
        assert L["Cw"] == 0 and L["num_warm"] == 0
    assert (seen == 1).all(), "every token is in exactly one of the cold / hot / warm lists"
    if sname == "sliced" and cname in ("ragged", "many_docs", "long_doc"):
        assert tiers >= 1, "the case was meant to keep a warm tier"


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
def test_word_order_and_segments(driver, tmp_path, cname, c):
    L = run(driver, tmp_path, c, SHAPES["sliced"])
    N = c.num_tokens
    perm, inv = L["perm"], L["inv"]
    assert sorted(perm) == list(range(N)) and (inv[perm] == np.arange(N)).all()
    w = c.tokens[perm]
    assert (np.diff(w) >= 0).all()
    same = np.diff(w) == 0
    assert (np.diff(perm)[same] > 0).all(), "the sort is stable"
    sb, sw = L["seg_begin"], L["seg_word"]
    assert len(sb) == len(sw) + 1 and sb[-1] == N and (len(sw) == 0 or sb[0] == 0)
    for s in range(len(sw)):
        assert 0 < sb[s + 1] - sb[s] <= L["kSegTokens"] and (w[sb[s]:sb[s + 1]] == sw[s]).all()
    for s in range(len(L["hseg_word"])):
        a, b = L["hseg_begin"][s], L["hseg_end"][s]
        assert 0 < b - a <= L["kSegTokens"] and (w[a:b] == L["hseg_word"][s]).all()
    covered = sum(int(L["hseg_end"][s] - L["hseg_begin"][s]) for s in range(len(L["hseg_word"])))
    assert covered == int(np.isin(c.tokens, L["hot_words"]).sum())


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
def test_two_row_chunks(driver, tmp_path, cname, c):
    L = run(driver, tmp_path, c, SHAPES["two_rows"])
    N, ptr = c.num_tokens, c.doc_ptr
    pos = 0
    for s, d0, d1, cl in zip(L["cstart"], L["cdoc"], L["cdoc1"], L["clen"]):
        n, n0 = int(cl) & 255, int(cl) >> 8
        assert s == pos and 1 <= n <= 64 and 1 <= n0 <= n, "no gap, no overlap"
        assert ptr[d0] <= s and s + n0 <= ptr[d0 + 1], "the first n0 tokens are document d0's"
        if n0 < n:
            assert d1 > d0 and ptr[d1] == s + n0 and s + n <= ptr[d1 + 1], "the rest is ONE other document's, from its first token"
            assert (np.diff(ptr[d0 + 1:d1 + 1]) == 0).all(), "only empty documents between the two"
        else:
            assert d1 == d0
        if n < 64:
            assert s + n == N or s + n == ptr[d1 + 1], "a short chunk ends at a document's end"
        pos += n
    assert pos == N
    # the parts of the z step: whole documents, whole chunks, in order
    pd, pc = L["part_doc"], L["part_chunk"]
    assert pd[0] == 0 and pd[-1] == c.num_docs and pc[0] == 0 and pc[-1] == len(L["cstart"])
    assert (np.diff(pd) >= 0).all() and (np.diff(pc) >= 0).all() and len(pd) == len(pc)
    assert len(pd) - 1 == (4 if c.num_docs >= 64 * 4 else 1)
    for p in range(1, len(pd) - 1):
        assert (L["cdoc"][pc[p]:] >= pd[p]).all() and (L["cdoc"][:pc[p]] < pd[p]).all()


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
def test_tile_chunks(driver, tmp_path, cname, c):
    T = SHAPES["tile"]["tile_tokens"]
    L = run(driver, tmp_path, c, SHAPES["tile"])
    ptr = c.doc_ptr
    assert len(L["cdoc1"]) == 0 and (np.diff(L["cdoc"]) >= 0).all()
    for d in range(c.num_docs):
        m = L["cdoc"] == d
        n = int(ptr[d + 1] - ptr[d])
        assert int(m.sum()) == -(-n // T)
        if n:
            lens, starts = L["clen"][m], L["cstart"][m]
            assert lens.sum() == n and lens.max() <= T and lens.max() - lens.min() <= 1
            assert starts[0] == ptr[d] and (starts[1:] == starts[:-1] + lens[:-1]).all()


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
@pytest.mark.parametrize("sname", ["pcgs", "pcgs_wide"])
def test_pcgs_order(driver, tmp_path, cname, c, sname):
    W = SHAPES[sname]["pcgs_waves"]
    L = run(driver, tmp_path, c, SHAPES[sname])
    order, D = L["order"], c.num_docs
    lens = np.diff(c.doc_ptr)
    assert L["longest"] == lens.max()
    assert (L["longest"] > L["kPcgsMaxDocLen"]) == (cname == "long_doc")
    named = order[order >= 0]
    assert sorted(named) == list(range(D)), "the (padded) order names every document once"
    groups = -(-D // 64)
    if W < groups <= 2 * W:
        assert len(order) == 2 * W * 64 and (order[order < 0] == -1).all()
        # a wave's two groups: a long one and a short one, the longest groups alone
        first, second = order[:W * 64].reshape(W, 64), order[W * 64:].reshape(W, 64)
        m = groups - W
        assert (second[:W - m] == -1).all() and (second[W - m:, 0] >= 0).all()
        assert (np.diff(lens[first[first >= 0]]) <= 0).all()
    else:
        assert len(order) == D and (np.diff(lens[order]) <= 0).all(), "longest first"
        assert (np.diff(order)[np.diff(lens[order]) == 0] > 0).all(), "equal lengths in document order"


COUNT_LISTS = ("perm", "inv", "seg_word", "seg_begin")
CHUNK_TABLE = ("cstart", "cdoc", "clen", "cdoc1", "part_doc", "part_chunk")
SLICED_LISTS = ("hot_words", "hseg_word", "hseg_begin", "hseg_end", "ct_tok", "ct_idx", "ct_ip", "c_docs", "Cc", "Cs", "ht_pack", "h_docs", "warm_tiers", "num_warm",
                "warm_rows_max", "Cw", "warm_chunks_max", "wt_pack", "w_docs", "warm_words", "warm_meta")


def absent(L, names):
    return all(np.size(L[k]) == 0 if isinstance(L[k], np.ndarray) else L[k] == 0 for k in names)


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
def test_one_list_family_per_shape(driver, tmp_path, cname, c):
    """A shape builds the lists of ONE z step and, always, what the count rebuild reads."""
    Ls = {name: run(driver, tmp_path, c, shape) for name, shape in SHAPES.items()}
    for name, L in Ls.items():
        for k in COUNT_LISTS:
            assert np.array_equal(L[k], Ls["tile"][k]), (name, k)
    for name in ("pcgs", "pcgs_wide"):
        L = Ls[name]
        assert absent(L, CHUNK_TABLE) and absent(L, SLICED_LISTS), "no chunk table, no z parts, no sliced lists"
        assert len(L["order"]) >= c.num_docs and L["longest"] == np.diff(c.doc_ptr).max()
    for name in ("sliced", "sliced_no_warm"):
        L = Ls[name]
        assert absent(L, CHUNK_TABLE) and absent(L, ("order", "longest")), "no tile / streaming chunk table, no document order"
        assert (L["Cs"] > 0) == (c.num_tokens > 0)
    for name in ("tile", "two_rows"):
        L = Ls[name]
        assert absent(L, SLICED_LISTS) and absent(L, ("order", "longest"))
        assert (len(L["cstart"]) > 0) == (c.num_tokens > 0) and len(L["part_doc"]) == len(L["part_chunk"]) >= 2


# sha256 of the driver's SLICED_LISTS lines as the commit before a shape built one family of z lists printed them (the corpora are seeded)
SLICED_PINS = {
    ("ragged", "sliced"): "e6194a599369ab67b1c91086a49f977f248e8b0a0d0fb61b9e79304621964276",
    ("ragged", "sliced_no_warm"): "b6eb8672e8c818e18cd76ef75e0329208823099ca1fd1ad7fae3bcca1a59269d",
    ("many_docs", "sliced"): "2d60f4e86922c7d6273604b7c89ba14a2e7bb6579f43f987679ed3b0b30eff65",
    ("many_docs", "sliced_no_warm"): "582918b393c23376f2d89ae3ee0902750a6519a815d4db553485f318a549b10b",
    ("long_doc", "sliced"): "99a04ccf7fa89e67544444bda0a9872fcdecd00ba84fbbef1809f5bd2ae8073f",
    ("long_doc", "sliced_no_warm"): "979425a12860cd56454817a276c7aea65a918133dc34d6ae2f72a288b36749ea",
    ("empty", "sliced"): "61b0c45d0f5eaefe75d37f827156c0171d194eed4f6f6fd8365c076e9d17b8dd",
    ("empty", "sliced_no_warm"): "61b0c45d0f5eaefe75d37f827156c0171d194eed4f6f6fd8365c076e9d17b8dd",
}


@pytest.mark.parametrize("cname,c", corpora(), ids=[n for n, _ in corpora()])
@pytest.mark.parametrize("sname", ["sliced", "sliced_no_warm"])
def test_sliced_lists_unchanged(driver, tmp_path, cname, c, sname):
    L = run(driver, tmp_path, c, SHAPES[sname])
    text = "".join(L["lines"][k] + "\n" for k in SLICED_LISTS)
    assert hashlib.sha256(text.encode()).hexdigest() == SLICED_PINS[cname, sname]
