// ggs_host_state.hpp -- what every other host header stands on: the GGS_DEBUG_* knob reader, the scheme table (kSchemes) and its
// predicates, the launch plan's types, the sweep's event ring, struct ggs_handle, and the handle's own primitives: errors, device
// memory, events and streams (each recorded in the handle, so that ggs_destroy frees by walking the records), the persistent
// launch, the status word, the copy out.  The ggs_host_*.hpp are parts of ONE translation unit, ggs_api.hip, and of no other: this one includes every kernel header and says `using namespace ggs`.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ggs_kernels.hpp"
#include "ggs_z_sliced.hpp"
#include "ggs_z_stream.hpp"
#include "ggs_exact_sum.hpp"
#include "ggs_z_pcgs.hpp"
#include "ggs_z_pcgs_wave.hpp"
#include "ggs_z_collapsed.hpp"
#include "ggs_phi_poisson.hpp"
#include "ggs_alias.hpp"
#include "ggs_z_spalias.hpp"
#include "ggs_z_polyaurn_sparse.hpp"
#include "ggs_phi_vs.hpp"
#include "ggs_z_lightpc.hpp"
#include "ggs_z_lightcollapsed.hpp"
#include "ggs_z_lightpcw2.hpp"
#include "ggs_z_adlda.hpp"
#include "ggs_loglik.hpp"
#include "ggs_heldout.hpp"
#include "ggs_exchange.hpp"
#include "ggs_corpus_lists.hpp"
#include "ggs_distances.hpp"
#include "ggs_topic_summaries.hpp"
#include "ggs_topic_diagnostics.hpp"
#include "ggs_hyper_hist.hpp"

using namespace ggs;

namespace {
// The GGS_DEBUG_* variables select kernels, scale proof margins and switch overlaps off: experiments and tests.  A
// production process must not pick one up by accident, so they are only read when GGS_DEBUG=1 is set as well.
// DESIGN.md section 8 lists them all.
const char *debug_env(const char *name) {
  static const bool enabled = [] { const char *e = std::getenv("GGS_DEBUG"); return e && std::atoi(e) == 1; }();
  return enabled ? std::getenv(name) : nullptr;
}
// A size that a test may shrink: the knob's value clamped to [1, built_in], the built-in constant without it.  Read at every
// call, as GGS_DEBUG_HELDOUT_CELLS is: pieces, groups and bands only get smaller, no result changes.
int64_t debug_shrunk(const char *name, int64_t built_in) {
  const char *e = debug_env(name);
  return e ? std::max<int64_t>(1, std::min<int64_t>(built_in, std::atoll(e))) : built_in;
}

// The knobs ggs_create reads, all at its top: what the launch planner takes instead of an environment, and the handle's
// own switches.  (The knobs of other entry points are read there: the exchange's at its set-up, GGS_DEBUG_SPALIAS_WPC at
// ggs_set_corpus, GGS_DEBUG_PHICOLS at a Phi draw, GGS_DEBUG_HELDOUT_CELLS at every held-out call, GGS_DEBUG_TD_PIECE_BYTES
// at every topic-diagnostics call, GGS_DEBUG_DIST_PIECE_BYTES and GGS_DEBUG_DIST_BAND_TILES at every distance call: the last
// three through debug_shrunk, which can only make a piece, a group or a band smaller.)
struct Knob {
  bool set = false;
  int v = 0;
  double f = 0;
  explicit Knob(const char *name) { if (const char *e = debug_env(name)) { set = true; v = std::atoi(e); f = std::atof(e); } }
  bool is(int x) const { return set && v == x; }
};
struct Knobs {
  // the planner's
  Knob zkernel{"GGS_DEBUG_ZKERNEL"}, group{"GGS_DEBUG_GROUP"}, regck{"GGS_DEBUG_REGCK"}, tworows{"GGS_DEBUG_TWOROWS"}, wpc{"GGS_DEBUG_WPC"};
  Knob phi64{"GGS_DEBUG_PHI64"}, split{"GGS_DEBUG_SPLIT"}, hot{"GGS_DEBUG_HOT"}, tile{"GGS_DEBUG_TILE"};
  Knob hot_pairs{"GGS_DEBUG_HOT_PAIRS"}, warm{"GGS_DEBUG_WARM"}, warm_rows{"GGS_DEBUG_WARM_ROWS"}, warm_fill{"GGS_DEBUG_WARM_FILL"}, warm_cpw{"GGS_DEBUG_WARM_CPW"};
  Knob theta_b{"GGS_DEBUG_THETA_B"}, theta_wgs{"GGS_DEBUG_THETA_WGS"}, zparts{"GGS_DEBUG_ZPARTS"}, beside{"GGS_DEBUG_BESIDE"};
  Knob pcgs_wave{"GGS_DEBUG_PCGS_WAVE"}, pcgs_stream{"GGS_DEBUG_PCGS_STREAM"};
  // the handle's
  Knob margin{"GGS_DEBUG_MARGIN"}, replays{"GGS_DEBUG_REPLAYS"}, chain{"GGS_DEBUG_CHAIN"}, guided{"GGS_DEBUG_GUIDED"};
  Knob no_overlap{"GGS_DEBUG_NO_OVERLAP"}, theta_main{"GGS_DEBUG_THETA_MAIN"}, gamma_queue{"GGS_DEBUG_GAMMA_QUEUE"};
  Knob num_cus{"GGS_DEBUG_NUM_CUS"}, vs_global{"GGS_DEBUG_VS_GLOBAL"};
};

constexpr int kThetaBlock = 256;

// What a handle samples and how: derived once from ggs_config::flags (scheme_of).  Every scheme but ggs runs the pcgs
// machinery: no theta in the chain, a document order instead of chunk lists, the plan's lane / wave / ... entries.  What a
// scheme is stands in its row of kSchemes, below the launch plan.
enum class Scheme { ggs, pcgs, collapsed, polyaurn, spalias, lightpclda, polyaurn_sparse, lightcollapsed, nzvsspalias, adlda, lightpcldaw2 };

// One kernel as a handle launches it: the function, its workgroup, its dynamic LDS and the workgroups per CU of its
// persistent grid.  The table kernels' LDS is given without table rows (they differ by corpus).
struct KernelLaunch {
  const void *fn = nullptr;
  int block = 64, lds = 0, per_cu = 0;
};
// The launches a handle can make and the few numbers the corpus step needs: decided once, by plan_launches() from
// (K, V, scheme, CUs, knobs): the ggs entries for scheme ggs only, the pcgs entries for the pcgs family only.  What
// depends on the corpus (a long document, D against V, the timed split) chooses BETWEEN these entries.
struct LaunchPlan {
  int32_t kernel = 0;                  // the ggs z kernel, as ggs_get_z_form numbers it: 0 whole-row tiles, 1 score registers (sliced), 2 streaming in one pass, 3 in two; the pcgs family leaves it 0
  bool sliced() const { return kernel == 1; }
  bool stream() const { return kernel >= 2; }
  KernelLaunch z;                      // the tile kernel or the streaming kernel
  int32_t tile_tokens = 64;            // tokens of a chunk of its table at most
  bool two_rows = false;               // streaming: two theta rows per wave, chunks may run across one document boundary (K <= 512)
  // sliced: the cold chunks' kernel (from phiT32 unless GGS_DEBUG_PHI64=1; in the fused form it takes the hot chunks too, the
  // table behind its rings), the hot chunks' and the warm tiers' table kernels
  KernelLaunch cold, hot, warm;
  // the split form's hot words by pair-chunks (z_pairs_kernel) in z_hot_kernel's place; GGS_DEBUG_HOT_PAIRS=0: z_hot_kernel, as the fused form's cold kernel takes them
  KernelLaunch pairs;
  bool hot_pairs = false;
  int32_t pairs_wave_lds = 0;
  bool f32 = false;
  bool split = true, split_forced = false;   // GGS_DEBUG_SPLIT=0: the fused form only; 2: the split form without the timed comparison
  int32_t wave_lds = 0, ring_base = 0, hot_wave_lds = 0, warm_wave_lds = 0, hot_pitch = 0, Kp32 = 0;   // ZParams of the three
  int32_t hot_cap = 0, warm_cap = 0, warm_docs = 0;   // rows of the hot table, of a warm tier's table; documents per warm chunk
  // What a tier must bring (measured on the benchmark corpus and its halves, ggs_corpus_lists.hpp): chunks at least 40 % full, at
  // least 3 of them per resident wave, three tiers at most -- GGS_DEBUG_WARM / GGS_DEBUG_WARM_FILL / GGS_DEBUG_WARM_CPW
  int32_t warm_tiers_max = 3, warm_min_fill_pct = 40, warm_min_chunks_per_wave = 3;
  // The theta draw and the z waves beside it, in the two configurations of the K > 192 path: with the z step cut into
  // parts of consecutive documents (the NEXT theta of a part is drawn on the side stream while the following parts are
  // sampled: the streaming z kernel waits on memory, the theta draw on the VALU) or in one piece.  Chosen per corpus.
  struct ZCfg { int32_t parts = 1, z_per_cu = 0, theta_docs = 0, theta_lds = 0, theta_lds_beside_z = 0; } cfg_plain, cfg_parts;
  bool parts_forced = false;
  KernelLaunch theta;                  // its LDS and documents per workgroup: the configuration's, or ...
  int32_t theta_docs_main = 0, theta_lds_main = 0;   // ... where the theta draw is the critical leg (theta_main)
  // scheme pcgs / collapsed / polyaurn: a lane or a wave per document; spalias: the table build and the sparse walk (LDS per corpus);
  // lightpclda: the same table build and the Metropolis-Hastings step; polyaurn_sparse: the table build, the words' lists and
  // the doubly sparse walk (LDS per corpus); lightcollapsed: the lists and tables over the counts and its Metropolis-Hastings step;
  // lightpcldaw2: the same build and its own Metropolis-Hastings step over Phi
  KernelLaunch lane, wave, alias, spalias, lightpc, serial, wordlist, pusparse, countalias, lightcol, lightpcw2;
  // nzvsspalias (ggs_phi_vs.hpp): the indicator chain's three kernels (its LDS comes with V), the list build from the drawn
  // cells (wordlist stays the build from phi != 0.0, after ggs_set_phi) and the z step
  KernelLaunch vsbits, vschain, wordmask, nzvs;
  // adlda (ggs_z_adlda.hpp): the sweep head (den0 and S0; the words' lists of the counts) and the bucket z step (LDS per corpus)
  KernelLaunch adhead, adlists, adlda;
  // every scheme (ggs_hyper_hist.hpp): the two histograms of the hyperparameter step; dochist.fn is null where K counts per wave pass the LDS
  KernelLaunch dochist, cellhist;
  bool wave_forced = false;            // ... because of K; otherwise per corpus (a document of 32 768 tokens or more)
  int32_t alias_wpb = 0;
  std::vector<const KernelLaunch *> all() const { return {&z, &cold, &hot, &pairs, &warm, &theta, &lane, &wave, &alias, &spalias, &lightpc, &serial, &wordlist, &pusparse, &countalias, &lightcol, &lightpcw2, &vsbits, &wordmask, &nzvs, &adlda, &dochist, &cellhist}; }   // not vschain: it has static LDS, and its dynamic LDS stays below the default cap
};

// One row per scheme, indexed by the enum: everything the host code asks about a scheme that is not its own buffers or its own
// launches.  A new scheme is a row here, its kernel header (ggs_z_*.hpp), its plan entry (plan_launches, ggs_host_plan.hpp) and its own buffers (ggs_create, ggs_api.hip).
enum : uint32_t { kHasAlias = 1, kHasTables = 2, kCountForm = 4, kCountsOnly = 8, kHasWordLists = 16, kDoublySparse = 32, kSparseWalk = 64, kHasMh = 128,
                  kPoissonPhi = 256, kSparseStats = 512, kCountTables = 1024, kNoTheta = 2048 };   // SchemeRow::caps: what the predicates below the table ask
struct SchemeRow {
  const char *name;                       // as the documentation spells it; the flag is GGS_FLAG_<NAME>
  int32_t flag, refused;                  // its own bit of ggs_config::flags (ggs: none), the bits that are GGS_ERR_BAD_ARG beside it
  int32_t z_kernel;                       // as ggs_get_z_form numbers it; 0: chosen per handle (ggs: plan.kernel) or per corpus (4 lane, 5 wave)
  KernelLaunch LaunchPlan::*entry;        // the wave-per-document z kernel of its own (K <= kPcgsWaveMaxTopics, a wave per order entry), or null: plan.lane / plan.wave
  size_t (*corpus_lds)(int K, int cap);   // ... whose LDS comes with the corpus: lists of sp_cap entries; or null
  const char *invalid_topic;              // the reference's message for GGS_ERR_INVALID_TOPIC
  uint32_t caps;
};
constexpr const char *kGgsInvalidTopic = "LDAGroupedGibbsSampler: Topic sampled is invalid!";
constexpr int32_t kModelFlags = GGS_FLAG_COLLAPSED | GGS_FLAG_POLYAURN, kLightFlags = kModelFlags | GGS_FLAG_SPALIAS | GGS_FLAG_LIGHTPCLDA | GGS_FLAG_POLYAURN_SPARSE;
// `refused`: one z step per handle.  spalias, lightpclda, polyaurn_sparse and nzvsspalias run over the pcgs model only (GGS_FLAG_PCGS
// beside them is accepted); lightcollapsed and adlda are the collapsed model under a z step of their own: no older scheme's flag
// beside them.  (GGS_FLAG_POLYAURN | GGS_FLAG_COLLAPSED is polyaurn, refused by the Poisson check of scheme_of.)
constexpr SchemeRow kSchemes[] = {
    {"ggs", 0, 0, 0, nullptr, nullptr, kGgsInvalidTopic, 0},
    {"pcgs", GGS_FLAG_PCGS, 0, 0, nullptr, nullptr, kGgsInvalidTopic, 0},
    {"collapsed", GGS_FLAG_COLLAPSED, 0, 0, nullptr, nullptr, "SimpleLDA: New topic not sampled." /* MSLDA:216-218 */, kCountForm},
    {"polyaurn", GGS_FLAG_POLYAURN, 0, 0, nullptr, nullptr, kGgsInvalidTopic, kPoissonPhi},
    {"spalias", GGS_FLAG_SPALIAS, kModelFlags, 6, &LaunchPlan::spalias, spalias_lds_bytes, kGgsInvalidTopic, kHasAlias | kHasTables | kSparseWalk},
    {"lightpclda", GGS_FLAG_LIGHTPCLDA, kModelFlags | GGS_FLAG_SPALIAS, 7, &LaunchPlan::lightpc, nullptr, kGgsInvalidTopic, kHasAlias | kHasTables | kHasMh},
    {"polyaurn_sparse", GGS_FLAG_POLYAURN_SPARSE, kModelFlags | GGS_FLAG_SPALIAS | GGS_FLAG_LIGHTPCLDA, 8, &LaunchPlan::pusparse, spalias_lds_bytes, kGgsInvalidTopic,
     kHasAlias | kHasTables | kHasWordLists | kDoublySparse | kSparseWalk | kPoissonPhi | kSparseStats},
    {"lightcollapsed", GGS_FLAG_LIGHTCOLLAPSED, kLightFlags | GGS_FLAG_PCGS, 9, &LaunchPlan::lightcol, nullptr, "Collapsed Light-LDA: Sampled invalid topic." /* CollapsedLightLDA.java:957-959 */,
     kHasTables | kCountForm | kCountsOnly | kHasWordLists | kHasMh | kCountTables},
    {"nzvsspalias", GGS_FLAG_NZVSSPALIAS, kLightFlags | GGS_FLAG_LIGHTCOLLAPSED, 10, &LaunchPlan::nzvs, spalias_lds_bytes, kGgsInvalidTopic,
     kHasAlias | kHasTables | kHasWordLists | kDoublySparse | kSparseWalk | kSparseStats},
    {"adlda", GGS_FLAG_ADLDA, kLightFlags | GGS_FLAG_PCGS | GGS_FLAG_LIGHTCOLLAPSED | GGS_FLAG_NZVSSPALIAS, 11, &LaunchPlan::adlda, adlda_lds_bytes, "ADLDA: New topic not sampled." /* MyWorkerRunnable.java:332-336 */,
     kCountForm | kCountsOnly | kHasWordLists | kSparseStats},
    // the pcgs model (GGS_FLAG_PCGS beside it is accepted) under lightcollapsed's tables and a z step of its own: no other scheme's flag beside it
    {"lightpcldaw2", GGS_FLAG_LIGHTPCLDAW2, kLightFlags | GGS_FLAG_LIGHTCOLLAPSED | GGS_FLAG_NZVSSPALIAS | GGS_FLAG_ADLDA, 12, &LaunchPlan::lightpcw2, nullptr,
     "Light PC-LDA (Type topic proposal): Sampled invalid topic." /* LightPCLDAtypeTopicProposal.java:159-161 */, kHasTables | kHasWordLists | kHasMh | kCountTables | kNoTheta},
};
constexpr int kNumSchemes = (int)(sizeof(kSchemes) / sizeof(kSchemes[0]));
static_assert(kNumSchemes == (int)Scheme::lightpcldaw2 + 1, "one row per Scheme, in the enum's order");
constexpr const SchemeRow &row_of(Scheme s) { return kSchemes[(int)s]; }
constexpr bool has(Scheme s, uint32_t cap) { return (row_of(s).caps & cap) != 0; }
constexpr bool pcgs_family(Scheme s) { return row_of(s).flag != 0; }
constexpr bool has_alias(Scheme s) { return has(s, kHasAlias); }             // alias_build_kernel's tables over Phi
constexpr bool count_form(Scheme s) { return has(s, kCountForm); }           // no Phi, the model is the type-topic counts and tokensPerTopic; the sweep's merge is the (word, z) histogram
constexpr bool counts_only(Scheme s) { return has(s, kCountsOnly); }         // ... and the z step never reads a Phi-shaped matrix or a theta: neither is allocated
constexpr bool has_tables(Scheme s) { return has(s, kHasTables); }           // ps / a / type_norm [V][K]: over Phi, or (lightcollapsed) over the counts
constexpr bool has_word_lists(Scheme s) { return has(s, kHasWordLists); }    // d_nzw / d_nw: per word the ascending list of its topics
constexpr bool doubly_sparse(Scheme s) { return has(s, kDoublySparse); }     // sparse_wave_body<true>: the words' lists and the counters
constexpr bool sparse_walk(Scheme s) { return has(s, kSparseWalk); }         // sparse_wave_body: SpaliasParams
constexpr bool has_mh(Scheme s) { return has(s, kHasMh); }                   // d_mh: a Metropolis-Hastings z step
constexpr bool poisson_phi(Scheme s) { return has(s, kPoissonPhi); }         // Phi drawn as polyaurn draws it
constexpr bool has_sparse_stats(Scheme s) { return has(s, kSparseStats); }   // d_ps_stats: ggs_get_sparse_stats
constexpr bool count_tables(Scheme s) { return has(s, kCountTables); }       // count_alias_build_kernel at the head of the z step: lists, tables, d_tpt over the sweep-start counts
constexpr bool no_theta(Scheme s) { return has(s, kNoTheta); }               // a Phi scheme that keeps no theta: the diagnostics that draw one allocate it (ensure_diag_theta)
constexpr bool wave_only(Scheme s) { return row_of(s).entry != nullptr; }   // no lane-per-document form: K <= kPcgsWaveMaxTopics, a wave per order entry
// "F needs GGS_FLAG_A, GGS_FLAG_B or GGS_FLAG_C": the flags of the schemes with `cap`, for the getters that only they answer
std::string needs_flag(const char *fn, uint32_t cap) {
  std::vector<std::string> names;
  for (const SchemeRow &r : kSchemes)
    if (r.caps & cap) { names.push_back("GGS_FLAG_"); for (const char *c = r.name; *c; ++c) names.back() += (char)std::toupper((unsigned char)*c); }
  std::string msg = std::string(fn) + " needs ";
  for (size_t i = 0; i < names.size(); ++i) msg += (i == 0 ? "" : i + 1 == names.size() ? " or " : ", ") + names[i];
  return msg;
}

// The phase events of one sweep.  Sweeps are settled (waited for, checked, timed) in batches, so a ring of them:
// sweep i records into slot i % kEvRing; the theta drawn ahead for sweep i + 1 records th0/th1 of THAT slot.
constexpr int kEvRing = 8;
struct Events {
  hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t x[3] = {nullptr, nullptr, nullptr};   // with an exchange: after the count reduce-scatter, after the slice's Phi draw, after the last all-gather (both halves in)
  hipEvent_t th0 = nullptr, th1 = nullptr;   // side-stream theta draw consumed by this sweep
  bool used_ahead = false, exchanged = false;
  bool e4_is_e3 = false;        // a whole sweep (ggs_sweep): nothing happens between the end of the count rebuild and the start of the Phi phase
  bool theta_on_main = false;   // the theta this sweep consumes was drawn on the handle's own stream, right behind the previous z step: no th0 (= that sweep's e[2])
  bool light = false;           // with an exchange: only e[1], e[2], e[5] were recorded; the span e[2]..e[5] is split as the last fully timed sweep's was
};
}  // namespace

struct ggs_handle {
  int32_t K = 0, V = 0, Kp = 0, pitch16 = 0, device = 0;
  double beta = 0;
  double beta_sum = 0;                                 // the Java field betaSum: beta * V until ggs_set_hyperparameters gives the learned value (MSLDA:897-901)
  std::vector<double> alpha;
  uint64_t seed = 0;
  int32_t flags = 0, phi_burn_in = 0, phi_thin = 1;   // flags: as the caller passed them
  Scheme scheme = Scheme::ggs;
  int32_t iteration = 0;
  int32_t n_sampled_phi = 0;

  int64_t D = 0, N = 0, C = 0, S = 0, doc_base = 0, tok_base = 0, global_tokens = -1;
  bool have_corpus = false, have_phi = false, in_sweep = false;
  bool have_z = false;                                 // ggs_init_z_java_lcg or ggs_set_z since the last ggs_set_corpus (read by ggs_host_similarity.hpp only)
  int32_t num_cus = 0;
  LaunchPlan plan;                                     // every launch this handle can make (plan_launches, at ggs_create)
  const LaunchPlan::ZCfg *cfg = nullptr;               // of the current corpus: plan.cfg_parts or plan.cfg_plain
  int32_t *d_chunk_doc1 = nullptr;
  double margin_scale = 1.0;   // GGS_DEBUG_MARGIN, clamped to >= 1: scales the fp64 certainty margins (tests force the exact replays)
  double margin_scale32 = 1.0; // ... clamped to >= 0: z_sliced32_kernel's margin (below 1 only to show the tests can fail)

  hipStream_t stream = nullptr;
  // device buffers
  int64_t *d_doc_ptr = nullptr, *d_chunk_start = nullptr;
  int32_t *d_tok = nullptr, *d_z = nullptr, *d_chunk_doc = nullptr, *d_chunk_len = nullptr;
  // sliced z kernel (ggs_z_sliced.hpp): its chunk lists (cold chunks first), the hot-word table's word ids
  int32_t *d_ct_tok = nullptr, *d_ct_idx = nullptr, *d_ct_ip = nullptr, *d_c_docs = nullptr, *d_hot_words = nullptr;
  int64_t Cs = 0, Cc = 0;                              // sliced chunks in all, cold ones
  int32_t *d_order = nullptr;                          // scheme=pcgs: local documents, longest first
  int64_t pcgs_order_len = 0;                          // entries of d_order (documents, or the padded two-round list)
  bool pcgs_wave = false;                              // of the current corpus: plan.wave (wide rows, or a document of 32 768 tokens or more) instead of plan.lane
  KernelLaunch pcgs_z;                                 // the plan entry launch_pcgs_z launches (pcgs_entry; spalias: with the LDS of lists of sp_cap entries) ...
  int64_t pcgs_items = 0;                              // ... over this many work items: entries of d_order, or groups of 64 of them (plan.lane)
  // scheme=polyaurn (ggs_phi_poisson.hpp): the pcgs z loop with its two uniform-draw rules, Phi drawn as Poisson counts
  int32_t pa_L = 0;                                    // alias_poisson_threshold
  double pa_t00 = 0;                                   // T_0[0]
  double *d_pa_table = nullptr;                        // [L][2L]
  unsigned long long *d_pa_acc = nullptr;              // [K][kPoissonAccStride]: the draw's integer totals
  // scheme=spalias (ggs_alias.hpp, ggs_z_spalias.hpp): the pcgs model, the z step split into an alias draw and a sparse walk
  bool alias_stale = true;                             // Phi has changed since the tables were built
  double *d_alias_ps = nullptr, *d_alias_tn = nullptr; // [V][K], [V]
  int32_t *d_alias_a = nullptr;                        // [V][K]
  int32_t sp_cap = 0;                                  // of the current corpus: entries of a document's list of non-zero topics
  // topic priors (ggs_set_topic_priors, spalias only): everything here is planned and allocated by that call
  bool have_priors = false;
  int32_t pr_pitch = 0;                                // uint32 words per vocabulary row of the bit mask: ceil(K / 32)
  std::vector<uint32_t> pr_mask;                       // [V][pr_pitch], bit k & 31 of word k >> 5 set = cell (k, v) is zero (the host's copy: ggs_set_phi's check)
  uint32_t *d_pr_mask = nullptr;
  double *d_pr_sum_phi = nullptr;                      // [K] index-order column sums of the old phiT (sum_phi of the conditional draw)
  double *d_pr_pref = nullptr, *d_pr_fn = nullptr;     // that sum's own guess and segment functions: d_sum_pref stays the magnitudes'
  // scheme=lightpclda (ggs_z_lightpc.hpp): the pcgs model and spalias's tables, a Metropolis-Hastings z step
  double alpha_sum = 0;                                // the k-order sum of alpha
  bool alpha_symmetric = false;                        // every alpha[k] has the bits of alpha[0]: the theta draw's count-0 cells share their gamma constants per document
  unsigned long long *d_mh = nullptr;                  // [3]: ggs_get_mh_stats, zeroed by ggs_set_corpus
  double *d_ad_den0 = nullptr, *d_ad_s0 = nullptr;     // scheme=adlda (ggs_z_adlda.hpp): [K] den0 and [1] S0 of the sweep-start counts
  int32_t *d_tpt = nullptr;                            // scheme=lightcollapsed, lightpcldaw2 (count_alias_build_kernel): [V] tokensPerType of the sweep-start counts
  // scheme=polyaurn_sparse (ggs_z_polyaurn_sparse.hpp): polyaurn's Phi, spalias's tables and document lists, and per word the
  // ascending list of its topics with phi != 0, rebuilt with the tables
  uint16_t *d_nzw = nullptr;                           // [V][K]
  int32_t *d_nw = nullptr;                             // [V]
  unsigned long long *d_ps_stats = nullptr;            // [4]: ggs_get_sparse_stats, zeroed by ggs_set_corpus
  // scheme=nzvsspalias (ggs_phi_vs.hpp): the pcgs model under the variable-selection Phi draw and the doubly sparse z step
  double vs_pi = 0.5;                                  // ggs_set_variable_selection_prior
  bool vs_global = false;                              // the chain's rows in global scratch: V > kVsLdsMaxV, or GGS_DEBUG_VS_GLOBAL=1
  int32_t vs_W = 0, vs_pitch = 0;                      // words of a topic's bit row: ceil(V / 32); of a word's mask row: ceil(K / 32)
  uint32_t *d_vs_cz = nullptr, *d_vs_pz = nullptr, *d_vs_und = nullptr;   // [K][vs_W]: count == 0, prevPhi == 0.0, the undrawn cells
  uint32_t *d_vs_mask = nullptr;                       // [V][vs_pitch]: the undrawn cells in zero_mask's layout
  int32_t *d_vs_work = nullptr, *d_vs_s_end = nullptr, *d_vs_rounds = nullptr;   // [K][2][vs_W] (vs_global only), [K], [K]
  unsigned long long *d_vs_zero = nullptr;             // [1] ggs_get_vs_stats's count of zero cells
  enum class VsLists { empty, drawn, nonzero } vs_lists = VsLists::empty;   // what the words' lists hold: nothing (the initial Phi), the last draw's drawn cells, phi != 0.0 (ggs_set_phi)
  bool vs_drawn = false;                               // a variable-selection draw has run: d_vs_und, d_vs_rounds are its
  uint64_t *d_lcg = nullptr;                           // ggs_collapsed_serial_sweep: the java.util.Random state
  bool lcg_ready = false;
  int32_t num_hot = 0;
  int32_t *d_perm = nullptr, *d_inv_perm = nullptr, *d_zw = nullptr, *d_seg_word = nullptr, *d_seg_begin = nullptr;
  // theta of the current / last z step, and the buffer the next iteration's theta is drawn into
  // on the side stream while this iteration's counts and Phi are computed (theta_{t+1} depends
  // on z_t only, GGS:57-72)
  double *d_theta_next = nullptr;
  hipStream_t side = nullptr;
  hipStream_t side_hot = nullptr;                      // z_hot_kernel runs here, beside z_sliced_kernel on the main stream
  hipEvent_t ev_hot_fork = nullptr, ev_hot_join = nullptr;
  // Whole sweeps on one GPU (ggs_sweep, K <= 160): the next theta is the LONGER of the two legs behind the z step (0.61 ms
  // against 0.50 for the counts and the Phi chain), and a dependency across streams takes 10-25 us to resolve -- so the
  // long leg stays on the handle's stream, directly between two z steps, and the short one (count rebuild + Phi chain)
  // goes to the high-priority stream the hot chunks used during the z step.  GGS_DEBUG_THETA_MAIN=0: the other way round.
  bool theta_main = true, chain_on_side = false, theta_main_always = false;   // GGS_DEBUG_THETA_MAIN=2: whatever D and V are (tests)
  bool whole_sweep = false;                            // inside ggs_sweep: z phase and Phi phase are enqueued back to back
  hipEvent_t hot_fork_from = nullptr;                  // an event already on the handle's stream that the hot kernel's stream may wait for instead of a fork event of its own
  hipEvent_t ev_chain_done = nullptr;
  bool z_split = true, z_split_tried = false;          // of the current corpus: cold and hot chunks beside each other; the first z step times both forms and keeps the faster
  // the warm tiers (z_warm_kernel): tables of the words next in frequency after the hot table's, chunks of up to plan.warm_docs documents
  int32_t warm_tiers = 0, num_warm = 0, warm_rows_max = 0;  // of the current corpus: tiers kept, their words in all, the largest table
  int64_t Cw = 0, warm_chunks_max = 0;                      // warm chunks in all, of the largest tier
  int32_t *d_wt_pack = nullptr, *d_w_docs = nullptr, *d_warm_words = nullptr;   // d_wt_pack: four int32 per lane (ZParams::wt_pack)
  int32_t *d_ht_pack = nullptr, *d_h_docs = nullptr;        // the hot chunks in the same packed form (z_hot_kernel)
  int64_t *d_warm_meta = nullptr;
  int32_t *d_hp_pair = nullptr, *d_hp_docs = nullptr, *d_hp_tok = nullptr;   // the hot words' pair-chunks (plan.hot_pairs; ZParams::hp_*)
  int64_t Cp = 0, hp_pairs = 0, hp_tokens = 0;              // ... of the current corpus: chunks, pairs, tokens
  bool overlap_theta = true;
  int32_t gamma_queue_cap = 1 << 20;   // GGS_DEBUG_GAMMA_QUEUE: a tiny queue sends the leftovers of the first try down the on-the-spot path
  std::vector<int64_t> part_doc, part_chunk;           // [parts + 1] boundaries of the z step's parts (plan.cfg_parts; the last part's theta runs beside the Phi phase)
  hipEvent_t ev_part[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t theta_ahead_iter = INT64_MIN;     // iteration the side-stream theta was drawn for, or none
  float *d_phiT32 = nullptr;                           // the float32 shadow of phiT the cold chunks gather (plan.f32), rows of plan.Kp32
  unsigned long long *d_replays = nullptr;             // GGS_DEBUG_REPLAYS: tokens z_sliced_kernel<KMAX, true> replayed, and its launches
  int64_t z_f32_launches = 0;
  double *d_alpha = nullptr, *d_theta = nullptr, *d_phiT = nullptr, *d_mag = nullptr, *d_tot = nullptr, *d_phi_mean = nullptr;
  int32_t *d_n_wk = nullptr, *d_n_k = nullptr;
  double *d_sum_pref = nullptr, *d_sum_fn = nullptr;   // work space of the exact parallel column sums (ggs_exact_sum.hpp)
  int32_t sum_nseg = 0;
  bool exact_sum = true;                               // GGS_DEBUG_CHAIN=1: the element-by-element column_chain_kernel instead
  bool sum_guided = true;                              // GGS_DEBUG_GUIDED=0: every magnitude sum makes its own guess (seg + prefix launches)
  const void *guess_src = nullptr;                     // d_sum_pref = the exact running sums of the last magnitude sum over this buffer ...
  int32_t guess_cols = 0;                              // ... and this many columns: a good guess for the next one
  uint32_t *d_status = nullptr;
  // test set of the held-out estimator (ggs_heldout.hpp)
  int64_t *d_test_ptr = nullptr;
  int32_t *d_test_tok = nullptr, *d_test_docs = nullptr;       // d_test_docs: ids of the documents of <= 255 tokens, then of those up to 65 535, then of the longer ones
  std::vector<int32_t> test_short, test_long, test_huge;
  void *d_heldout_spill = nullptr;
  size_t heldout_spill_bytes = 0;
  double *d_test_ll = nullptr;
  std::vector<int64_t> test_ptr;
  int64_t test_doc_base = 0;
  bool have_test = false;
  void *d_scratch = nullptr;
  size_t scratch_bytes = 0;

  // multi-GPU exchange (ggs_exchange.hpp).  Without one: Ks = Ksm = K, k0 = 0 and the counts live in d_n_wk.
  Exchange *xg = nullptr;
  hipStream_t own_stream = nullptr;                    // with an exchange the handle leaves the legacy default stream
  int32_t Ks = 0, Ksm = 0, k0 = 0;                     // this rank's topic slice [k0, k0 + Ks), widest slice Ksm
  int64_t *d_koff = nullptr;                           // [K] column of topic k in the slice-major arrays
  int32_t *d_cnt_send = nullptr, *d_cnt_own = nullptr, *d_cnt_all = nullptr, *d_n_k_own = nullptr;
  // the rank's unnormalised gammas [V][Ksm] and, behind them, their Ksm column sums; gathered in two halves (rows below /
  // from v_split), the first half's all-gather on `comm_stream` under the second half's draw, the sums riding with the second
  double *d_phi_own = nullptr, *d_phi_all0 = nullptr, *d_phi_all1 = nullptr, *d_mag_own = nullptr;
  int32_t *d_krank = nullptr, *d_kcol = nullptr;      // [K] owner rank and column in its slice, for the repack
  int32_t seg_split = 0, v_split = 0;                  // first segment / row of the second half (0: one all-gather)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_half_drawn = nullptr, ev_half_gathered = nullptr;
  int32_t *d_hseg_word = nullptr, *d_hseg_begin = nullptr, *d_hseg_end = nullptr;   // the hot words' count segments (the z kernels count the cold tokens themselves)
  int64_t HS = 0;
  // With an exchange every event packet on the handle's stream sits on the sweep's critical path (2.8 us each, 7.5 for two
  // back to back: scripts/probes/event_cost_probe.hip), and a fully timed sweep records five that only the phase split
  // needs (e[3], e[4], x[0..2]).  One sweep in kDetailEvery records them all; the others record the ends of the z step and
  // of the sweep and split the rest in the proportions of the last fully timed sweep (GGS_DEBUG_TIMING_EVERY=1: all).
  int32_t detail_every = 4;
  bool force_detail = false;                           // a z step that no Phi phase follows (ggs_sample_z_given_phi) is timed in full
  int64_t sweeps_enqueued = 0;
  bool have_frac = false;
  double frac[5] = {0, 0, 0, 0, 0};                    // of e[2]..e[5]: merge | reduce-scatter | slice draw | all-gather wait | repack
  // the SPARSE count exchange (ggs_set_count_exchange): (cell, count) pairs of the non-zero cells instead of the dense buffer
  int32_t count_mode = 0;                              // 0 by rule, 1 dense, 2 sparse
  bool counted_sparse = false;                         // the last count of this shard was pass A of the sparse form (the dense send buffer does not hold it)
  bool in_group = false;                               // a handle of ggs_group_create / ggs_group_adopt: its collectives are collected step by step, no host round trip inside
  int64_t *d_sp_count = nullptr;                       // [nranks] pairs per destination (pass A), then the write cursors of pass B
  int32_t *d_sp_cnt32 = nullptr, *d_sp_all = nullptr;  // [nranks] the same as int32 for the all-gather; [nranks][nranks] everybody's
  int32_t *d_sp_wg_count = nullptr;                    // [workgroups][nranks] pairs per workgroup and destination
  int64_t *d_sp_wg_off = nullptr;                      // ... and their exclusive prefix over the workgroups
  int64_t sp_wgs = 0;
  int32_t *d_sp_send = nullptr, *d_sp_recv = nullptr;
  size_t sp_send_cap = 0, sp_recv_cap = 0;             // elements
  int64_t sp_pairs_last = 0;
  bool hot_join_pending = false, hot_counted = false;   // launch_z(defer_join): the handle's stream has not yet waited for the hot chunks' stream; the hot words' count ran there
  bool z_counted = false;                              // this sweep's z step has already added its cells into d_cnt_send
  bool cnt_send_zeroed = false;                        // d_cnt_send is all zero (cleared behind the last reduce-scatter): what the z kernels' own count updates start from
  bool z_counts_forced = false;
  bool z_counts = true;                                // GGS_DEBUG_ZCOUNTS=0: the count kernel also with an exchange (the cross-check)
  SliceMap smap{};                                     // topic -> cell of the slice-major send buffer
  bool counts_global = true;                           // d_n_wk holds the corpus-wide counts
  bool cnt_own_valid = false;                          // d_cnt_own = reduce-scatter of the current d_cnt_send
  bool n_k_valid = false;                              // d_n_k follows d_n_wk
  std::vector<ggs_handle *> group;                     // ggs_group_create: the handles of the group, in rank order (rank 0 only)

  std::vector<void **> owned;                          // every device buffer dev_alloc has filled: what ggs_destroy frees
  std::vector<hipEvent_t> owned_events;                // ... every event make_event has created
  std::vector<hipStream_t> owned_streams;              // ... every stream make_stream has created
  Events evs[kEvRing];
  int ev_head = 0, ev_pending = 0;                     // slot of the sweep in progress; sweeps enqueued but not settled
  ggs_timings tm{};
  std::string err;
};

namespace {
int set_err(ggs_handle *h, int code, const std::string &msg) {
  if (h) h->err = msg;
  return code;
}

#define HIP_TRY(h, expr)                                                                       \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess)                                                                       \
      return set_err((h), GGS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));      \
  } while (0)

int bind_device(ggs_handle *h) {
  HIP_TRY(h, hipSetDevice(h->device));
  return GGS_OK;
}

// Every device buffer of a handle is allocated here and recorded, so that ggs_destroy frees it without a list of its own.
template <typename T>
int dev_alloc(ggs_handle *h, T **p, size_t count) {
  void **slot = reinterpret_cast<void **>(p);
  if (std::find(h->owned.begin(), h->owned.end(), slot) == h->owned.end()) h->owned.push_back(slot);
  if (*p) { (void)hipFree(*p); *p = nullptr; }
  HIP_TRY(h, hipMalloc(slot, std::max<size_t>(count, 1) * sizeof(T)));
  return GGS_OK;
}
// ... and zeroed (on the null stream)
template <typename T>
int dev_alloc_zeroed(ggs_handle *h, T **p, size_t count) {
  const int rc = dev_alloc(h, p, count);
  if (rc) return rc;
  HIP_TRY(h, hipMemset(*p, 0, sizeof(T) * count));
  return GGS_OK;
}
// ... and filled from the host (on the null stream)
template <typename T>
int upload(ggs_handle *h, T **p, const T *src, size_t count) {
  const int rc = dev_alloc(h, p, count);
  if (rc) return rc;
  if (count) HIP_TRY(h, hipMemcpy(*p, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return GGS_OK;
}
template <typename T>
int upload(ggs_handle *h, T **p, const std::vector<T> &v) { return upload(h, p, v.data(), v.size()); }
// The handle's events and streams are created here and recorded like its buffers: ggs_destroy walks the records.
int make_event(ggs_handle *h, hipEvent_t *ev, unsigned flags = hipEventDefault) {
  HIP_TRY(h, hipEventCreateWithFlags(ev, flags));
  h->owned_events.push_back(*ev);
  return GGS_OK;
}
int make_stream(ggs_handle *h, hipStream_t *st, int priority) {
  HIP_TRY(h, hipStreamCreateWithPriority(st, hipStreamNonBlocking, priority));
  h->owned_streams.push_back(*st);
  return GGS_OK;
}
// Events of one call (a timed comparison, a *_phases entry point): a fixed array, destroyed with the scope, whichever return ends it; make() past its end gives null, as a failed creation does.
template <int N>
struct ScopedEvents {
  hipEvent_t ev[N] = {};
  int n = 0;
  hipEvent_t make() { return n < N && hipEventCreate(&ev[n]) == hipSuccess ? ev[n++] : nullptr; }
  ~ScopedEvents() { for (int i = 0; i < n; ++i) (void)hipEventDestroy(ev[i]); }
};
// the ring slot of the sweep `back` sweeps before the one in progress (-1: the next one)
Events &ev_slot(ggs_handle *h, int back) { return h->evs[((h->ev_head - back) % kEvRing + kEvRing) % kEvRing]; }

// A plan entry on `st` over `items` work items, one per wave: the grid is persistent -- the workgroups that stay resident
// (CUs x per_cu), fewer where the items do not fill them -- and strides the rest.  `table_lds`: the rows of a Phi table.
hipError_t launch(const ggs_handle *h, const KernelLaunch &l, int64_t items, void **args, hipStream_t st, int table_lds = 0) {
  const int waves = l.block / 64;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((items + waves - 1) / waves, (int64_t)h->num_cus * l.per_cu));
  return hipLaunchKernel(l.fn, dim3((unsigned)grid), dim3((unsigned)l.block), args, (size_t)(l.lds + table_lds), st);
}

int ensure_scratch(ggs_handle *h, size_t bytes) {
  if (h->scratch_bytes >= bytes) return GGS_OK;
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  h->d_scratch = nullptr; h->scratch_bytes = 0;
  HIP_TRY(h, hipMalloc(&h->d_scratch, bytes));
  h->scratch_bytes = bytes;
  return GGS_OK;
}

int grid_for(int64_t n, int block, int per_thread = 1) {
  const int64_t want = (n + (int64_t)block * per_thread - 1) / ((int64_t)block * per_thread);
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, 256 * 8));  // grid-stride above ~8 blocks/CU
}

// Surfaces what the Java code throws from its worker threads.
int check_status(ggs_handle *h) {
  uint32_t st = 0;
  HIP_TRY(h, hipMemcpyAsync(&st, h->d_status, sizeof st, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (!st) return GGS_OK;
  HIP_TRY(h, hipMemsetAsync(h->d_status, 0, sizeof(uint32_t), h->stream));
  if (st & ST_INVALID_TOPIC) return set_err(h, GGS_ERR_INVALID_TOPIC, row_of(h->scheme).invalid_topic);
  if (st & ST_NEGATIVE_COUNT) return set_err(h, GGS_ERR_NEGATIVE_COUNT, "Negative count for topic (Invalid count!)");
  if (st & ST_BAD_SHAPE) return set_err(h, GGS_ERR_BAD_ARG, "alpha and beta must be strictly positive (gamma shape <= 0)");
  if (st & ST_INVARIANT) return set_err(h, GGS_ERR_INVARIANT, "Inconsistent Indicator probability");   // VSDirichlet.java:55
  return set_err(h, GGS_ERR_RNG_EXHAUSTED, "a gamma rejection loop exceeded GGS_MAX_BLOCKS Philox blocks");
}

int require_ready(ggs_handle *h, bool need_phi) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!h->have_corpus) return set_err(h, GGS_ERR_STATE, "no corpus: call ggs_set_corpus first");
  if (need_phi && !h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  return bind_device(h);
}

int copy_out(ggs_handle *h, void *dst, const void *src, size_t bytes) {
  if (!bytes) return GGS_OK;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GGS_OK;
}
}  // namespace
