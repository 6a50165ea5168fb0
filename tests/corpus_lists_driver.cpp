// Driver of tests/test_corpus_lists_cpu.py: builds the lists of ggs_corpus_lists.hpp for one corpus with a host compiler
// and prints them.  usage: driver CORPUS.bin key=value ...   (CORPUS.bin: int64 D, int64 N, int64 doc_ptr[D + 1],
// int32 tokens[N]; the keys are the fields of ggs::CorpusShape)
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
  for (int i = 2; i < argc; ++i) {
    const char *eq = std::strchr(argv[i], '=');
    if (!eq) return 2;
    const std::string key(argv[i], (size_t)(eq - argv[i]));
    const long long v = std::atoll(eq + 1);
    if (key == "V") s.V = (int32_t)v;
    else if (key == "pcgs") s.pcgs = v != 0;
    else if (key == "sliced") s.sliced = v != 0;
    else if (key == "two_rows") s.two_rows = v != 0;
    else if (key == "tile_tokens") s.tile_tokens = (int32_t)v;
    else if (key == "z_parts") s.z_parts = (int32_t)v;
    else if (key == "hot_cap") s.hot_cap = (int32_t)v;
    else if (key == "warm_cap") s.warm_cap = (int32_t)v;
    else if (key == "warm_docs") s.warm_docs = (int32_t)v;
    else if (key == "warm_tiers_max") s.warm_tiers_max = (int32_t)v;
    else if (key == "warm_min_fill_pct") s.warm_min_fill_pct = (int32_t)v;
    else if (key == "warm_min_chunks_per_wave") s.warm_min_chunks_per_wave = (int32_t)v;
    else if (key == "sliced_waves") s.sliced_waves = v;
    else if (key == "pcgs_waves") s.pcgs_waves = v;
    else return 2;
  }
  const ggs::CorpusLists L = ggs::build_corpus_lists(s, D, doc_ptr.data(), tokens.data());
  put("kChunkDocs", ggs::kChunkDocs); put("kSlotShift", ggs::kSlotShift); put("kWarmSlotShift", ggs::kWarmSlotShift);
  put("kWarmDocSlots", ggs::kWarmDocSlots); put("kPcgsMaxDocLen", ggs::kPcgsMaxDocLen); put("kSegTokens", ggs::kSegTokens);
  put("cstart", L.cstart); put("cdoc", L.cdoc); put("clen", L.clen); put("cdoc1", L.cdoc1);
  put("part_doc", L.part_doc); put("part_chunk", L.part_chunk);
  put("perm", L.perm); put("inv", L.inv); put("seg_word", L.seg_word); put("seg_begin", L.seg_begin);
  put("hot_words", L.hot_words); put("hseg_word", L.hseg_word); put("hseg_begin", L.hseg_begin); put("hseg_end", L.hseg_end);
  put("order", L.order); put("longest", L.longest);
  put("ct_tok", L.ct_tok); put("ct_idx", L.ct_idx); put("ct_ip", L.ct_ip); put("c_docs", L.c_docs); put("Cc", L.Cc); put("Cs", L.Cs);
  put("ht_pack", L.ht_pack); put("h_docs", L.h_docs);
  put("warm_tiers", L.warm_tiers); put("num_warm", L.num_warm); put("warm_rows_max", L.warm_rows_max); put("Cw", L.Cw);
  put("warm_chunks_max", L.warm_chunks_max);
  put("wt_pack", L.wt_pack); put("w_docs", L.w_docs); put("warm_words", L.warm_words); put("warm_meta", L.warm_meta);
  return 0;
}
