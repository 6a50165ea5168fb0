// ggs_layout.hpp -- what the kernels and the host code that feeds them must agree on, and what the plain C++ host code
// (ggs_corpus_lists.hpp) needs of it: the constants of the chunk lists' packed words and the LDS allocation rules of a
// CU.  No HIP header: a host compiler reads this file too.  The LDS layout of a kernel is a function beside that kernel.
#pragma once
#include <stdint.h>

namespace ggs {

constexpr int imax(const int a, const int b) { return a > b ? a : b; }
constexpr int imin(const int a, const int b) { return a < b ? a : b; }
constexpr int round_up(const int x, const int unit) { return (x + unit - 1) / unit * unit; }

// ---- LDS of a CU
constexpr int kMaxLdsBytes = 160 * 1024;
// LDS is handed out in granules (measured: 6 x 26,912 B do not fit a CU although the occupancy API says they do) ...
constexpr int kLdsGranule = 2048;
constexpr int lds_alloc_of(const int bytes) { return round_up(bytes, kLdsGranule); }
// ... and a CU cannot be filled to the last granule: measured, 5 x 32 KiB and 4 x 40 KiB leave one workgroup waiting for a
// second round (z at K = 1024: 18.6 ms with 5 waves of 32 KiB requested, 12.7 ms with 4).  Persistent grids are sized by
// this: the workgroups of `bytes` LDS each that are truly co-resident on a CU, `cap` at most.
constexpr int lds_workgroups_per_cu(const int bytes, const int cap) { return imax(1, imin(cap, (kMaxLdsBytes - kLdsGranule) / lds_alloc_of(bytes))); }

// ---- chunk lists (ggs_z_sliced.hpp reads them, ggs_corpus_lists.hpp writes them)
constexpr int kSlicedWaves = 4;           // waves per workgroup (one per SIMD), sharing the hot-word table
constexpr int kChunkDocs = 2;             // documents a chunk may draw tokens from
constexpr int kSlotShift = 30;            // chunk token word: value | (which of the chunk's documents) << 30
constexpr int kWarmMaxTiers = 8;
constexpr int kWarmSlotShift = 16;        // warm chunk token word: table row | (which of the chunk's documents) << 16
constexpr int kWarmDocSlots = 8;          // document ids stored per warm chunk (one 32-byte scalar load), whatever warm_docs_for() says
// the hot words' pair-chunks (z_pairs_kernel): up to 64 distinct (document, table row) pairs of at most kHotPairDocs consecutive
// documents, and the tokens of exactly those pairs in rounds of 64 lanes
constexpr int kHotPairDocs = 2;           // 2 keeps the theta rows of the next chunk in 8 registers (16 at KMAX > 128): 55.7 pairs per chunk on the benchmark corpus.  4 would fill the 64 pairs, but takes twice the registers (z_pairs_kernel<160> then spills) and two theta rows more of LDS per wave; profiles/hot_pairs_ab.txt has the comparison
constexpr int kHotPairRounds = 4;         // token rounds of a pair-chunk at most: the token entries of the next chunk travel through registers
constexpr int kHotPairTokenCap = 64 * kHotPairRounds;
constexpr int kHotPairLaneShift = 24;     // pair-chunk token word: table row | (document slot) << kWarmSlotShift | (lane of its pair) << 24
constexpr int kHotPairTokSlot = 4, kHotPairCountSlot = 5, kHotPairRoundSlot = 6;   // a pair-chunk's kWarmDocSlots words: its documents, then tokens, pairs, first token round
constexpr int kPcgsMaxDocLen = 32767;     // the lane-per-document pcgs kernels count in int16
constexpr int64_t kSegTokens = 4096;      // count kernel: a word's run of the word-sorted tokens is cut into segments of at most this

}  // namespace ggs
