// Driver of tests/test_hot_pair_lists_cpu.py: the lists of ggs_corpus_lists.hpp for one corpus, built twice with a host compiler
// -- with and without the hot words' pair-chunks (CorpusShape::hot_pairs) -- and printed: the pair-chunk lists of the first
// build, and whether every other list of the two builds is the same.  usage: driver CORPUS.bin key=value ...  (CORPUS.bin as
// tests/corpus_lists_driver.cpp reads it; the keys are fields of ggs::CorpusShape)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ggs_corpus_lists.hpp"

template <typename T>
static void put(const char *name, const std::vector<T> &v) {
  std::printf("%s %zu", name, v.size());
  for (const T &x : v) std::printf(" %lld", (long long)x);
  std::printf("\n");
}
static void put(const char *name, long long x) { std::printf("%s 1 %lld\n", name, x); }

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t D = 0, N = 0;
  if (std::fread(&D, 8, 1, f) != 1 || std::fread(&N, 8, 1, f) != 1) return 2;
  std::vector<int64_t> doc_ptr((size_t)D + 1);
  std::vector<int32_t> tokens((size_t)N);
  if (std::fread(doc_ptr.data(), 8, doc_ptr.size(), f) != doc_ptr.size() || std::fread(tokens.data(), 4, tokens.size(), f) != tokens.size()) return 2;
  std::fclose(f);
  ggs::CorpusShape s;
  s.sliced = true;
  bool quiet = false;
  for (int i = 2; i < argc; ++i) {
    const char *eq = std::strchr(argv[i], '=');
    if (!eq) return 2;
    const std::string key(argv[i], (size_t)(eq - argv[i]));
    const long long v = std::atoll(eq + 1);
    if (key == "V") s.V = (int32_t)v;
    else if (key == "hot_cap") s.hot_cap = (int32_t)v;
    else if (key == "warm_cap") s.warm_cap = (int32_t)v;
    else if (key == "warm_docs") s.warm_docs = (int32_t)v;
    else if (key == "warm_tiers_max") s.warm_tiers_max = (int32_t)v;
    else if (key == "warm_min_fill_pct") s.warm_min_fill_pct = (int32_t)v;
    else if (key == "warm_min_chunks_per_wave") s.warm_min_chunks_per_wave = (int32_t)v;
    else if (key == "sliced_waves") s.sliced_waves = v;
    else if (key == "quiet") quiet = v != 0;                 // the sizes only (a large corpus)
    else return 2;
  }
  s.hot_pairs = true;
  const ggs::CorpusLists L = ggs::build_corpus_lists(s, D, doc_ptr.data(), tokens.data());
  s.hot_pairs = false;
  const ggs::CorpusLists P = ggs::build_corpus_lists(s, D, doc_ptr.data(), tokens.data());
  const bool same = L.perm == P.perm && L.inv == P.inv && L.seg_word == P.seg_word && L.seg_begin == P.seg_begin && L.hot_words == P.hot_words &&
                    L.hseg_word == P.hseg_word && L.hseg_begin == P.hseg_begin && L.hseg_end == P.hseg_end && L.ct_tok == P.ct_tok && L.ct_idx == P.ct_idx &&
                    L.ct_ip == P.ct_ip && L.c_docs == P.c_docs && L.Cc == P.Cc && L.Cs == P.Cs && L.ht_pack == P.ht_pack && L.h_docs == P.h_docs &&
                    L.warm_tiers == P.warm_tiers && L.num_warm == P.num_warm && L.warm_rows_max == P.warm_rows_max && L.Cw == P.Cw &&
                    L.warm_chunks_max == P.warm_chunks_max && L.wt_pack == P.wt_pack && L.w_docs == P.w_docs && L.warm_words == P.warm_words &&
                    L.warm_meta == P.warm_meta;
  put("old_lists_same", same ? 1 : 0);
  put("absent_without", (P.hp_pair.empty() && P.hp_docs.empty() && P.hp_tok.empty() && P.Cp == 0) ? 1 : 0);
  put("kHotPairDocs", ggs::kHotPairDocs); put("kHotPairTokenCap", ggs::kHotPairTokenCap); put("kHotPairLaneShift", ggs::kHotPairLaneShift);
  put("kWarmSlotShift", ggs::kWarmSlotShift); put("kWarmDocSlots", ggs::kWarmDocSlots);
  put("kHotPairTokSlot", ggs::kHotPairTokSlot); put("kHotPairCountSlot", ggs::kHotPairCountSlot); put("kHotPairRoundSlot", ggs::kHotPairRoundSlot);
  put("Cp", L.Cp); put("Cs", L.Cs); put("Cc", L.Cc);
  if (quiet) {
    long long pairs = 0, toks = 0;
    for (int64_t c = 0; c < L.Cp; ++c) { pairs += L.hp_docs[(size_t)(c * ggs::kWarmDocSlots + ggs::kHotPairCountSlot)]; toks += L.hp_docs[(size_t)(c * ggs::kWarmDocSlots + ggs::kHotPairTokSlot)]; }
    put("pairs", pairs); put("hot_tokens", toks); put("rounds", (long long)(L.hp_tok.size() / 256));
    return 0;
  }
  put("inv", L.inv); put("hot_words", L.hot_words);
  put("hp_pair", L.hp_pair); put("hp_docs", L.hp_docs); put("hp_tok", L.hp_tok);
  return 0;
}
