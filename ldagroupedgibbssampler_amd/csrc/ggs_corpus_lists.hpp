// ggs_corpus_lists.hpp -- the host half of ggs_set_corpus that touches no GPU: from a corpus and the few numbers the
// launch plan fixes, every list the handle's kernels read: the count rebuild's (word-sorted permutation, count segments) and
// those of the ONE z step the plan launches (chunk table and the parts of the z step, or the cold / hot / warm chunk lists
// and their packed forms, or the pcgs document order).  Plain C++: no HIP header, so a
// host compiler builds it and tests/test_corpus_lists_cpu.py checks it without a GPU.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "ggs_layout.hpp"

namespace ggs {

// What the lists depend on besides the corpus.  One family of z-step lists per handle: `pcgs` goes before `sliced`, and
// with neither the chunk table of the tile and streaming kernels is built.
struct CorpusShape {
  int32_t V = 0;
  bool pcgs = false;                 // the document order of the pcgs kernels, and no other z list
  bool sliced = false;               // the cold / hot / warm chunk lists of the score-register kernels and the hot words' count segments
  bool two_rows = false;             // chunk table: 64 consecutive tokens across at most one document boundary
  int32_t tile_tokens = 64;          // ... otherwise near-equal cuts of single documents, this many tokens at most
  int32_t z_parts = 1;               // parts of consecutive documents the z step is cut into
  int32_t hot_cap = 0, warm_cap = 0, warm_docs = 0;   // rows of the hot table, of a warm tier's; documents per warm chunk
  int32_t warm_tiers_max = 0, warm_min_fill_pct = 0, warm_min_chunks_per_wave = 0;
  bool hot_pairs = false;            // sliced: the hot words' pair-chunks as well (z_pairs_kernel takes them where z_hot_kernel took the hot chunks)
  int64_t sliced_waves = 0;          // resident waves of a table kernel (CUs x kSlicedWaves)
  int64_t pcgs_waves = 0;            // resident waves of the lane-per-document pcgs kernel
};

struct CorpusLists {
  int64_t D = 0, N = 0;
  // chunk table of the tile and streaming kernels; two_rows: clen = tokens | tokens of the first document << 8, cdoc1 the second document
  std::vector<int64_t> cstart;
  std::vector<int32_t> cdoc, clen, cdoc1;
  std::vector<int64_t> part_doc, part_chunk;           // [parts + 1] boundaries of the z step's parts (with the chunk table)
  // tokens sorted by word (stable) and its inverse; each word's run cut into segments; the hot words' segments once more
  std::vector<int32_t> perm, inv, seg_word, seg_begin, hot_words, hseg_word, hseg_begin, hseg_end;
  // pcgs: documents longest first, or the padded two-round list (-1 = no document)
  std::vector<int32_t> order;
  int64_t longest = 0;
  // sliced: cold chunks then hot chunks, 64 lanes each: token word, token index (-1: idle lane), its place in the
  // word-sorted order; kChunkDocs document ids per chunk
  std::vector<int32_t> ct_tok, ct_idx, ct_ip, c_docs;
  int64_t Cc = 0, Cs = 0;                              // cold chunks, cold + hot
  std::vector<int32_t> ht_pack, h_docs;                // the hot chunks in the packed form of the warm tiers (four int32 per lane, kWarmDocSlots ids per chunk)
  // the warm tiers kept, tier after tier; meta = [tiers + 1] first chunk of a tier, then [tiers] rows of its table
  int32_t warm_tiers = 0, num_warm = 0, warm_rows_max = 0;
  int64_t Cw = 0, warm_chunks_max = 0;
  std::vector<int32_t> wt_pack, w_docs, warm_words;
  std::vector<int64_t> warm_meta;
  // the hot words once more, as pair-chunks (CorpusShape::hot_pairs): hp_pair = 64 lanes per chunk, a distinct (document, table
  // row) pair each: row | (document slot) << kWarmSlotShift, in (document, row) order (idle lanes 0); hp_docs = kWarmDocSlots
  // words per chunk: its kHotPairDocs documents (unused slots repeat the first), then at kHotPairTokSlot its tokens, its
  // pairs and its first token round; hp_tok = the tokens of the chunk's pairs in whole rounds of 64 lanes, in pair order, four
  // int32 per lane: the pair's word | (lane of the pair) << kHotPairLaneShift, token index (-1: idle lane), its place in the
  // word-sorted order, 0.  A pair's tokens are in one chunk; a pair of more than kHotPairTokenCap tokens is entered once per
  // kHotPairTokenCap of them, each entry in a chunk of its own.
  std::vector<int32_t> hp_pair, hp_docs, hp_tok;
  int64_t Cp = 0;                                      // pair-chunks
};

namespace lists_detail {

// The chunks of one list: walk the documents in order and deal tokens to the open chunk; a chunk closes at 64 tokens or
// when one document more than `maxdocs` would enter it.  (Documents are visited in order, so a token's document is
// always the chunk's newest: slot = documents so far - 1.)
struct ChunkBuilder {
  int maxdocs = kChunkDocs, docslots = kChunkDocs, shift = kSlotShift;   // documents a chunk may draw from; ids stored per chunk
  std::vector<int32_t> tok, idx, docs;
  int fill = 64, ndocs = 0, last = -1;
  int64_t tokens = 0;
  void add(int32_t value, int32_t token, int32_t doc) {
    if (fill == 64 || (doc != last && ndocs == maxdocs)) {
      tok.resize(tok.size() + 64, 0); idx.resize(idx.size() + 64, -1);
      docs.insert(docs.end(), (size_t)docslots, doc);
      fill = 0; ndocs = 1; last = doc;
    } else if (doc != last) {
      docs[docs.size() - (size_t)docslots + (size_t)ndocs] = doc; ++ndocs; last = doc;
    }
    const size_t at = tok.size() - 64 + (size_t)fill;
    tok[at] = value | ((ndocs - 1) << shift); idx[at] = token;
    ++fill; ++tokens;
  }
  int64_t chunks() const { return (int64_t)(tok.size() / 64); }
  // Lanes of a chunk in (document, row) order: the 16 lanes one LDS pass serves then mostly read the same theta row
  // and, in hot chunks, few distinct table rows (tokens of one word share a row: a broadcast, not a bank conflict).
  void sort_lanes() {
    std::vector<std::pair<uint32_t, int32_t>> tmp(64);
    for (size_t c0 = 0; c0 < tok.size(); c0 += 64) {
      int n = 0;
      while (n < 64 && idx[c0 + (size_t)n] >= 0) ++n;                 // active lanes are a prefix
      for (int j = 0; j < n; ++j) tmp[(size_t)j] = {(uint32_t)tok[c0 + (size_t)j], idx[c0 + (size_t)j]};
      std::sort(tmp.begin(), tmp.begin() + n);
      for (int j = 0; j < n; ++j) { tok[c0 + (size_t)j] = (int32_t)tmp[(size_t)j].first; idx[c0 + (size_t)j] = tmp[(size_t)j].second; }
    }
  }
};

// z-kernel work items.  two_rows: 64 consecutive tokens per chunk, across at most one document boundary; otherwise each
// document is cut into ceil(len/T) near-equal chunks of <= T tokens.
inline void chunk_table(const CorpusShape &s, const int64_t D, const int64_t *doc_ptr, CorpusLists &L) {
  const int64_t N = L.N;
  L.cstart.reserve((size_t)(N / 48 + D)); L.cdoc.reserve(L.cstart.capacity()); L.clen.reserve(L.cstart.capacity());
  if (s.two_rows) {
    int64_t pos = 0, d = 0;
    while (pos < N) {
      while (doc_ptr[d + 1] <= pos) ++d;                            // the document of token `pos` (empty documents hold none)
      const int64_t take0 = std::min<int64_t>(64, doc_ptr[d + 1] - pos);
      int64_t len = take0, d1 = d;
      if (take0 < 64 && pos + take0 < N) {                          // room left: the next non-empty document joins
        d1 = d + 1;
        while (doc_ptr[d1 + 1] <= pos + take0) ++d1;
        len += std::min<int64_t>(64 - take0, doc_ptr[d1 + 1] - (pos + take0));
      }
      L.cstart.push_back(pos); L.cdoc.push_back((int32_t)d); L.cdoc1.push_back((int32_t)d1);
      L.clen.push_back((int32_t)(len | (take0 << 8)));
      pos += len;
    }
    return;
  }
  for (int64_t d = 0; d < D; ++d) {
    const int64_t len = doc_ptr[d + 1] - doc_ptr[d];
    if (len == 0) continue;
    const int64_t T = s.tile_tokens, n = (len + T - 1) / T, base = len / n, rem = len % n;
    int64_t at = doc_ptr[d];
    for (int64_t j = 0; j < n; ++j) {
      const int64_t l = base + (j < rem ? 1 : 0);
      L.cstart.push_back(at); L.cdoc.push_back((int32_t)d); L.clen.push_back((int32_t)l);
      at += l;
    }
  }
}

// The parts of the z step: consecutive documents with about equal token counts, and their chunk ranges; a corpus of fewer
// than 64 documents per part goes in one.
inline void z_parts(const CorpusShape &s, const int64_t D, const int64_t *doc_ptr, CorpusLists &L) {
  const int32_t P = (s.z_parts > 1 && D >= 64 * s.z_parts) ? s.z_parts : 1;
  const int64_t C = (int64_t)L.cstart.size();
  L.part_doc.assign((size_t)P + 1, D); L.part_chunk.assign((size_t)P + 1, C);
  L.part_doc[0] = 0; L.part_chunk[0] = 0;
  int64_t d = 0;
  size_t c = 0;
  for (int32_t p = 1; p < P; ++p) {
    const int64_t want = L.N * p / P;
    while (d < D && doc_ptr[d] < want) ++d;
    while (c < L.cdoc.size() && L.cdoc[c] < d) ++c;
    L.part_doc[(size_t)p] = d; L.part_chunk[(size_t)p] = (int64_t)c;
  }
}

// Count-kernel work items: tokens sorted by word (counting sort, stable), each word's run cut into segments of at most
// kSegTokens entries (a segment ends where the next begins, or at the end of its word's run).  sliced: the hot-word
// table = the hot_cap most frequent words of THIS corpus, and behind them the candidates of the warm tiers (returned).
inline std::vector<int32_t> word_order(const CorpusShape &s, const int32_t *tokens, CorpusLists &L) {
  const int64_t N = L.N;
  std::vector<int32_t> warm_cand;
  L.perm.resize((size_t)N); L.inv.resize((size_t)N);
  std::vector<int64_t> wptr((size_t)s.V + 1, 0);
  for (int64_t i = 0; i < N; ++i) wptr[(size_t)tokens[i] + 1]++;
  for (int32_t w = 0; w < s.V; ++w) wptr[(size_t)w + 1] += wptr[(size_t)w];
  for (int32_t w = 0; w < s.V; ++w)
    for (int64_t b = wptr[(size_t)w]; b < wptr[(size_t)w + 1]; b += kSegTokens) { L.seg_word.push_back(w); L.seg_begin.push_back((int32_t)b); }
  L.seg_begin.push_back((int32_t)N);
  std::vector<int64_t> cur(wptr.begin(), wptr.end() - 1);
  for (int64_t i = 0; i < N; ++i) L.perm[(size_t)cur[(size_t)tokens[i]]++] = (int32_t)i;
  for (int64_t i = 0; i < N; ++i) L.inv[(size_t)L.perm[(size_t)i]] = (int32_t)i;
  if (s.sliced && !s.pcgs && s.hot_cap > 0) {
    std::vector<int32_t> order((size_t)s.V);
    for (int32_t w = 0; w < s.V; ++w) order[(size_t)w] = w;
    const size_t nh = (size_t)std::min<int32_t>(s.hot_cap, s.V);
    const size_t nw = std::min<size_t>((size_t)s.V, nh + (size_t)s.warm_tiers_max * (size_t)s.warm_cap);
    auto freq = [&](int32_t w) { return wptr[(size_t)w + 1] - wptr[(size_t)w]; };
    std::partial_sort(order.begin(), order.begin() + nw, order.end(), [&](int32_t a, int32_t b) { return freq(a) != freq(b) ? freq(a) > freq(b) : a < b; });
    for (size_t r = 0; r < nh && freq(order[r]) > 0; ++r) L.hot_words.push_back(order[r]);
    for (size_t r = nh; r < nw && freq(order[r]) > 0; ++r) warm_cand.push_back(order[r]);
    for (int32_t w : L.hot_words)
      for (int64_t b = wptr[(size_t)w]; b < wptr[(size_t)w + 1]; b += kSegTokens) {
        L.hseg_word.push_back(w); L.hseg_begin.push_back((int32_t)b); L.hseg_end.push_back((int32_t)std::min(b + kSegTokens, wptr[(size_t)w + 1]));
      }
  }
  return warm_cand;
}

// pcgs: documents longest first, so that the 64 of a wave are equally long.  A wave takes the groups w, w + W, ... of this
// list (W = the resident waves).  With between one and two rounds of groups (the benchmark corpus: 1 563 groups for 1 024
// waves) the plain order would give the waves of the 539 LONGEST groups a second one: 420 steps against 205 for the rest.
// Instead the W - m longest groups run alone and the 2m shortest are paired long-with-short on the last m waves (-1 = no
// document): 360 steps at most.
inline void pcgs_order(const CorpusShape &s, const int64_t D, const int64_t *doc_ptr, CorpusLists &L) {
  std::vector<int32_t> &order = L.order;
  order.resize((size_t)D);
  for (int64_t d = 0; d < D; ++d) { order[(size_t)d] = (int32_t)d; L.longest = std::max(L.longest, doc_ptr[d + 1] - doc_ptr[d]); }
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return doc_ptr[a + 1] - doc_ptr[a] > doc_ptr[b + 1] - doc_ptr[b]; });
  const int64_t n_groups = (D + 63) / 64, W = s.pcgs_waves;
  if (n_groups > W && n_groups <= 2 * W) {
    const int64_t m = n_groups - W;
    std::vector<int32_t> padded((size_t)(2 * W * 64), -1);
    auto put = [&](int64_t position, int64_t group) {
      for (int64_t j = 0; j < 64 && group * 64 + j < D; ++j) padded[(size_t)(position * 64 + j)] = order[(size_t)(group * 64 + j)];
    };
    for (int64_t g = 0; g < W; ++g) put(g, g);
    for (int64_t j = 0; j < m; ++j) put(W + (W - m + j), n_groups - 1 - j);
    order.swap(padded);
  }
}

// four int32 per lane: token word, token index, its place in the word-sorted order, 0
inline std::vector<int32_t> pack_lanes(const std::vector<int32_t> &tok, const std::vector<int32_t> &idx, const std::vector<int32_t> &inv) {
  std::vector<int32_t> pack(4 * idx.size(), 0);
  for (size_t j = 0; j < idx.size(); ++j) {
    pack[4 * j] = tok[j]; pack[4 * j + 1] = idx[j];
    if (idx[j] >= 0) pack[4 * j + 2] = inv[(size_t)idx[j]];
  }
  return pack;
}

// The hot words' pair-chunks (CorpusLists::hp_*).  A chunk closes at 64 pairs, when a pair's tokens would take it past
// kHotPairTokenCap (so that a chunk is at most kHotPairRounds token rounds) or when one document more than kHotPairDocs would
// enter it.  Counted on the benchmark corpus with its 79-row table (10.63 M hot tokens, 3.69 M pairs): 66 238 chunks of 55.7
// pairs and 160 tokens on average, 2.99 token rounds per chunk, 84 % of their lanes in use -- against 166 152 hot chunks of 64
// tokens.  `row_of`: a word's row of the hot table, negative for every other word.
inline void hot_pair_lists(const int64_t D, const int64_t *doc_ptr, const int32_t *tokens, const std::vector<int32_t> &row_of, CorpusLists &L) {
  std::vector<std::pair<int32_t, int32_t>> dt;                       // a document's hot tokens: (row, token)
  std::vector<int32_t> ctok;                                         // the open chunk's token entries
  int npairs = 0, ndocs = 0, ntok = 0, last = -1;
  bool open = false;
  auto close_chunk = [&]() {
    if (!open) return;
    int32_t *meta = &L.hp_docs[L.hp_docs.size() - (size_t)kWarmDocSlots];
    meta[kHotPairTokSlot] = ntok; meta[kHotPairCountSlot] = npairs; meta[kHotPairRoundSlot] = (int32_t)(L.hp_tok.size() / (4 * 64));
    L.hp_tok.insert(L.hp_tok.end(), ctok.begin(), ctok.end());
    for (int j = ntok; j % 64 != 0; ++j) { const int32_t idle[4] = {0, -1, 0, 0}; L.hp_tok.insert(L.hp_tok.end(), idle, idle + 4); }
    ctok.clear();
    open = false;
  };
  for (int64_t d = 0; d < D; ++d) {
    dt.clear();
    for (int64_t i = doc_ptr[d]; i < doc_ptr[d + 1]; ++i)
      if (row_of[(size_t)tokens[i]] >= 0) dt.push_back({row_of[(size_t)tokens[i]], (int32_t)i});
    std::sort(dt.begin(), dt.end());
    for (size_t a = 0; a < dt.size();) {
      size_t b = a;
      while (b < dt.size() && dt[b].first == dt[a].first) ++b;
      for (; a < b; a += (size_t)kHotPairTokenCap) {                 // one entry, unless the pair alone passes the cap
        const int m = (int)std::min<size_t>(b - a, (size_t)kHotPairTokenCap);
        if (!open || npairs == 64 || ntok + m > kHotPairTokenCap || ((int32_t)d != last && ndocs == kHotPairDocs)) {
          close_chunk();
          L.hp_pair.resize(L.hp_pair.size() + 64, 0);
          L.hp_docs.insert(L.hp_docs.end(), (size_t)kWarmDocSlots, 0);
          for (int r = 0; r < kHotPairDocs; ++r) L.hp_docs[L.hp_docs.size() - (size_t)kWarmDocSlots + (size_t)r] = (int32_t)d;
          open = true; npairs = 0; ndocs = 1; ntok = 0; last = (int32_t)d;
        } else if ((int32_t)d != last) {
          L.hp_docs[L.hp_docs.size() - (size_t)kWarmDocSlots + (size_t)ndocs] = (int32_t)d; ++ndocs; last = (int32_t)d;
        }
        const int32_t word = dt[a].first | ((ndocs - 1) << kWarmSlotShift);
        L.hp_pair[L.hp_pair.size() - 64 + (size_t)npairs] = word;
        for (int j = 0; j < m; ++j) {
          const int32_t i = dt[a + (size_t)j].second;
          const int32_t e[4] = {word | (npairs << kHotPairLaneShift), i, L.inv[(size_t)i], 0};
          ctok.insert(ctok.end(), e, e + 4);
        }
        ++npairs; ntok += m;
      }
      a = b;
    }
  }
  close_chunk();
  L.Cp = (int64_t)(L.hp_pair.size() / 64);
}

// Chunk lists of the sliced kernels: every token goes to the open cold chunk, the open hot chunk or the open chunk of its
// warm tier.
// The warm tiers: tier t = candidates [t*warm_cap, (t+1)*warm_cap).  A tier is kept while its chunks (64 lanes, up to
// warm_docs documents) are reasonably full -- a token in a half-empty chunk costs what two cost -- and numerous enough
// to pay for the tier's table load, its two barriers and the ragged end of its chunk list; tiers are kept in order: the
// first one that falls short ends the list, its words and all later ones stay cold.  Measured with the table kernels'
// hand-counted loads (profiles/r04_warm_tier_sweep.txt; before them a tier wanted 10 chunks per wave), sweep in ms with
// 0 / 1 / 2 / 3 tiers: the benchmark corpus (20 M tokens; 14.4, 11.7, 10.7 chunks per wave) 1.517 / 1.494 / 1.461 /
// 1.471 (4, 5, 6 tiers: 1.464 / 1.471 / 1.472, 8: 1.513); half of it (rank 0 of 2: 7 chunks per wave in the first tier)
// 0.887 / 0.873 / 0.870 / 0.864; a quarter 0.552 / 0.547 / 0.543 / 0.545; an eighth (under 2 chunks per wave) 0.376 /
// 0.378 / 0.380 / 0.394 -- there a tier's table load and barriers cost what its tokens save.
inline void sliced_lists(const CorpusShape &s, const int64_t D, const int64_t *doc_ptr, const int32_t *tokens, std::vector<int32_t> warm_cand, CorpusLists &L) {
  ChunkBuilder cold, hot;
  std::vector<int32_t> row_of((size_t)s.V, -1);
  for (size_t r = 0; r < L.hot_words.size(); ++r) row_of[(size_t)L.hot_words[r]] = (int32_t)r;
  std::vector<ChunkBuilder> warm;
  int32_t tiers = 0;
  if (s.warm_cap > 0 && L.hot_words.size() == (size_t)s.hot_cap && !warm_cand.empty()) {
    const int32_t cand_tiers = (int32_t)((warm_cand.size() + (size_t)s.warm_cap - 1) / (size_t)s.warm_cap);
    warm.resize((size_t)cand_tiers);
    for (ChunkBuilder &b : warm) { b.maxdocs = s.warm_docs; b.docslots = kWarmDocSlots; b.shift = kWarmSlotShift; }
    std::vector<int32_t> warm_of((size_t)s.V, -1);
    for (size_t r = 0; r < warm_cand.size(); ++r) warm_of[(size_t)warm_cand[r]] = (int32_t)r;
    for (int64_t d = 0; d < D; ++d)
      for (int64_t i = doc_ptr[d]; i < doc_ptr[d + 1]; ++i) {
        const int32_t r = warm_of[(size_t)tokens[i]];
        if (r >= 0) warm[(size_t)(r / s.warm_cap)].add(r % s.warm_cap, (int32_t)i, (int32_t)d);
      }
    const int64_t min_chunks = (int64_t)s.warm_min_chunks_per_wave * s.sliced_waves;
    while (tiers < cand_tiers && warm[(size_t)tiers].tokens > 0 && warm[(size_t)tiers].chunks() >= min_chunks &&
           warm[(size_t)tiers].tokens * 100 >= warm[(size_t)tiers].chunks() * 64 * s.warm_min_fill_pct)
      ++tiers;
    warm.resize((size_t)tiers);
    warm_cand.resize(std::min(warm_cand.size(), (size_t)tiers * (size_t)s.warm_cap));
    for (int32_t w : warm_cand) row_of[(size_t)w] = -2;              // in a kept tier: neither cold nor hot
  }
  for (int64_t d = 0; d < D; ++d)
    for (int64_t i = doc_ptr[d]; i < doc_ptr[d + 1]; ++i) {
      const int32_t r = row_of[(size_t)tokens[i]];
      if (r >= 0) hot.add(r, (int32_t)i, (int32_t)d);
      else if (r == -1) cold.add(tokens[i], (int32_t)i, (int32_t)d);
    }
  if (s.hot_pairs) hot_pair_lists(D, doc_ptr, tokens, row_of, L);
  cold.sort_lanes();
  hot.sort_lanes();
  for (ChunkBuilder &b : warm) b.sort_lanes();
  L.Cc = cold.chunks();
  L.Cs = L.Cc + hot.chunks();
  {
    // z_hot_kernel reads its chunks in the packed form of the warm tiers: the chunk's documents in kWarmDocSlots slots, the
    // document slot at kWarmSlotShift
    std::vector<int32_t> htok(hot.tok.size());
    for (size_t j = 0; j < htok.size(); ++j) {
      const uint32_t t = (uint32_t)hot.tok[j];
      htok[j] = (int32_t)((t & ((1u << kSlotShift) - 1)) | ((t >> kSlotShift) << kWarmSlotShift));
    }
    L.ht_pack = pack_lanes(htok, hot.idx, L.inv);
    L.h_docs.assign((size_t)hot.chunks() * (size_t)kWarmDocSlots, 0);
    for (size_t c = 0; c < (size_t)hot.chunks(); ++c)
      for (int r = 0; r < kWarmDocSlots; ++r) L.h_docs[c * (size_t)kWarmDocSlots + (size_t)r] = hot.docs[(size_t)kChunkDocs * c + (size_t)std::min(r, kChunkDocs - 1)];
  }
  L.ct_tok = std::move(cold.tok); L.ct_idx = std::move(cold.idx); L.c_docs = std::move(cold.docs);
  L.ct_tok.insert(L.ct_tok.end(), hot.tok.begin(), hot.tok.end());
  L.ct_idx.insert(L.ct_idx.end(), hot.idx.begin(), hot.idx.end());
  L.c_docs.insert(L.c_docs.end(), hot.docs.begin(), hot.docs.end());
  L.ct_ip.assign(L.ct_idx.size(), 0);
  for (size_t j = 0; j < L.ct_ip.size(); ++j)
    if (L.ct_idx[j] >= 0) L.ct_ip[j] = L.inv[(size_t)L.ct_idx[j]];
  L.warm_tiers = tiers; L.num_warm = (int32_t)warm_cand.size();
  if (tiers > 0) {
    std::vector<int32_t> wtok, widx;
    L.warm_words.assign((size_t)tiers * (size_t)s.warm_cap, 0);
    L.warm_meta.assign((size_t)(2 * tiers + 1), 0);
    for (int32_t t = 0; t < tiers; ++t) {
      const ChunkBuilder &b = warm[(size_t)t];
      L.warm_meta[(size_t)t] = (int64_t)(wtok.size() / 64);
      const int32_t rows = (int32_t)std::min<size_t>((size_t)s.warm_cap, warm_cand.size() - (size_t)t * (size_t)s.warm_cap);
      L.warm_meta[(size_t)(tiers + 1 + t)] = rows;
      L.warm_rows_max = std::max(L.warm_rows_max, rows);
      L.warm_chunks_max = std::max(L.warm_chunks_max, b.chunks());
      wtok.insert(wtok.end(), b.tok.begin(), b.tok.end());
      widx.insert(widx.end(), b.idx.begin(), b.idx.end());
      L.w_docs.insert(L.w_docs.end(), b.docs.begin(), b.docs.end());
      for (int32_t r = 0; r < rows; ++r) L.warm_words[(size_t)t * (size_t)s.warm_cap + (size_t)r] = warm_cand[(size_t)t * (size_t)s.warm_cap + (size_t)r];
    }
    L.warm_meta[(size_t)tiers] = (int64_t)(wtok.size() / 64);
    L.Cw = L.warm_meta[(size_t)tiers];
    L.wt_pack = pack_lanes(wtok, widx, L.inv);
  }
}

}  // namespace lists_detail

// The corpus is taken as valid (ggs_set_corpus has checked it): doc_ptr[0] = 0, non-decreasing, tokens in [0, V).
inline CorpusLists build_corpus_lists(const CorpusShape &s, const int64_t D, const int64_t *doc_ptr, const int32_t *tokens) {
  CorpusLists L;
  L.D = D; L.N = doc_ptr[D];
  std::vector<int32_t> warm_cand = lists_detail::word_order(s, tokens, L);   // every handle: the count rebuild's
  if (s.pcgs) {
    lists_detail::pcgs_order(s, D, doc_ptr, L);
  } else if (s.sliced) {
    lists_detail::sliced_lists(s, D, doc_ptr, tokens, std::move(warm_cand), L);
  } else {
    lists_detail::chunk_table(s, D, doc_ptr, L);
    lists_detail::z_parts(s, D, doc_ptr, L);
  }
  return L;
}

}  // namespace ggs
