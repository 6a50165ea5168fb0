// ggs_api.hip -- host side of libggs_hip.so: handle, launches, C-ABI (include/ggs_hip.h).
//
// Build (see Makefile): hipcc -O3 --offload-arch=gfx950 -ffp-contract=off -fPIC -shared
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
  Knob warm{"GGS_DEBUG_WARM"}, warm_rows{"GGS_DEBUG_WARM_ROWS"}, warm_fill{"GGS_DEBUG_WARM_FILL"}, warm_cpw{"GGS_DEBUG_WARM_CPW"};
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
  bool wave_forced = false;            // ... because of K; otherwise per corpus (a document of 32 768 tokens or more)
  int32_t alias_wpb = 0;
  std::vector<const KernelLaunch *> all() const { return {&z, &cold, &hot, &warm, &theta, &lane, &wave, &alias, &spalias, &lightpc, &serial, &wordlist, &pusparse, &countalias, &lightcol, &lightpcw2, &vsbits, &wordmask, &nzvs, &adlda}; }   // not vschain: it has static LDS, and its dynamic LDS stays below the default cap
};

// One row per scheme, indexed by the enum: everything the host code asks about a scheme that is not its own buffers or its own
// launches.  A new scheme is a row here, its kernel header, its plan entry (plan_launches) and its own buffers (ggs_create).
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
  std::vector<double> alpha;
  uint64_t seed = 0;
  int32_t flags = 0, phi_burn_in = 0, phi_thin = 1;   // flags: as the caller passed them
  Scheme scheme = Scheme::ggs;
  int32_t iteration = 0;
  int32_t n_sampled_phi = 0;

  int64_t D = 0, N = 0, C = 0, S = 0, doc_base = 0, tok_base = 0, global_tokens = -1;
  bool have_corpus = false, have_phi = false, in_sweep = false;
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

// A plan entry on `st` over `items` work items, one per wave: the grid is persistent -- the workgroups that stay resident
// (CUs x per_cu), fewer where the items do not fill them -- and strides the rest.  `table_lds`: the rows of a Phi table.
hipError_t launch(const ggs_handle *h, const KernelLaunch &l, int64_t items, void **args, hipStream_t st, int table_lds = 0) {
  const int waves = l.block / 64;
  const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((items + waves - 1) / waves, (int64_t)h->num_cus * l.per_cu));
  return hipLaunchKernel(l.fn, dim3((unsigned)grid), dim3((unsigned)l.block), args, (size_t)(l.lds + table_lds), st);
}

// scheme=polyaurn: the inverse-CDF tables of the Poisson draws with c < L (ggs_phi_poisson.hpp), row c for lambda = beta + c:
// p_0 = exp(-lambda), p_j = p_{j-1} * lambda / j for j < 2L (PoissonFixedCoeffSampler.java:31-50 keeps the same 2L terms),
// S_j = p_0 + ... + p_j left to right, T_c[j] = S_j / S_{2L-1} and T_c[2L-1] = 1.  fp64, in this order: the tests restate it.
void build_poisson_table(double beta, int32_t L, std::vector<double> &T) {
  const int n = 2 * L;
  T.assign((size_t)L * n, 0.0);
  std::vector<double> S((size_t)n);
  for (int32_t c = 0; c < L; ++c) {
    const double lambda = beta + (double)c;
    double pj = std::exp(-lambda), acc = 0.0;
    for (int j = 0; j < n; ++j) {
      if (j > 0) pj = pj * lambda / (double)j;
      acc += pj;
      S[(size_t)j] = acc;
    }
    for (int j = 0; j < n - 1; ++j) T[(size_t)c * n + j] = S[(size_t)j] / S[(size_t)n - 1];
    T[(size_t)c * n + n - 1] = 1.0;
  }
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

// after a host upload of z (document order): refresh the word-sorted copy the count kernel reads
int launch_permute_z(ggs_handle *h) {
  if (h->N > 0)
    hipLaunchKernelGGL(permute_z_kernel, dim3(grid_for(h->N, 256)), dim3(256), 0, h->stream, h->d_perm, h->d_z, h->d_zw, h->N);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// Does the next count exchange of this handle ship (cell, count) pairs?  Every input of the rule is the same on every rank.
bool use_sparse(const ggs_handle *h) {
  if (!h->xg || h->in_group || !h->xg->ops.all_to_all_v_i32 || h->xg->nranks > kSparseMaxRanks) return false;
  if ((int64_t)h->V * h->Ksm >= ((int64_t)1 << 31)) return false;       // a cell index is an int32
  if (h->count_mode == 1) return false;
  if (h->count_mode == 2) return true;
  if (h->global_tokens < 0) return false;              // the rule needs a figure all ranks share
  const int64_t cells = (int64_t)h->V * h->K;
  return cells >= ((int64_t)1 << 26) && h->global_tokens / h->xg->nranks < cells / 2;
}
SparseCountParams sparse_params(const ggs_handle *h) {
  SparseCountParams sp{};
  sp.zw = h->d_zw; sp.seg_word = h->d_seg_word; sp.seg_begin = h->d_seg_begin; sp.K = h->K; sp.num_segs = (int32_t)h->S; sp.nranks = h->xg->nranks;
  sp.ksm = h->Ksm; sp.rem = h->smap.rem; sp.size = h->smap.size; sp.m_size = h->smap.m_size; sp.m_size1 = h->smap.m_size1;
  return sp;
}
// pass A of the sparse form: how many pairs this rank has for every destination
int launch_sparse_count(ggs_handle *h) {
  const int n = h->xg->nranks;
  int rc;
  if (!h->d_sp_count && ((rc = dev_alloc(h, &h->d_sp_count, (size_t)n)) || (rc = dev_alloc(h, &h->d_sp_cnt32, (size_t)n)) || (rc = dev_alloc(h, &h->d_sp_all, (size_t)n * n)))) return rc;
  const int64_t wgs = (h->S + kSparseSegsPerBlock - 1) / kSparseSegsPerBlock;
  if (wgs != h->sp_wgs || !h->d_sp_wg_count) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((rc = dev_alloc(h, &h->d_sp_wg_count, (size_t)wgs * n)) || (rc = dev_alloc(h, &h->d_sp_wg_off, (size_t)wgs * n))) return rc;
    h->sp_wgs = wgs;
  }
  if (wgs > 0) {
    SparseCountParams sp = sparse_params(h);
    sp.wg_count = h->d_sp_wg_count;
    hipLaunchKernelGGL(sparse_count_kernel<false>, dim3((unsigned)wgs), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, sp);
    hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)n), dim3(256), 0, h->stream, h->d_sp_wg_count, (int32_t)wgs, n, h->d_sp_wg_off, h->d_sp_count);
    HIP_TRY(h, hipGetLastError());
  } else {
    HIP_TRY(h, hipMemsetAsync(h->d_sp_count, 0, sizeof(int64_t) * (size_t)n, h->stream));
  }
  h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false;
  h->counted_sparse = true;
  return GGS_OK;
}

// n_wk = histogram of (word, z) over this handle's tokens (UPLDA:471-474 summed over the corpus).  With an exchange the
// histogram goes straight into the slice-major send buffer of the count reduce-scatter.
int launch_count_rebuild(ggs_handle *h) {
  if (use_sparse(h)) return launch_sparse_count(h);     // no dense buffer: the pairs are emitted inside the exchange step, once their number is known
  h->counted_sparse = false;
  const size_t cells = h->xg ? (size_t)h->xg->nranks * h->V * h->Ksm : (size_t)h->K * h->V;
  int32_t *dst = h->xg ? h->d_cnt_send : h->d_n_wk;
  if (!(h->xg && h->cnt_send_zeroed)) HIP_TRY(h, hipMemsetAsync(dst, 0, cells * sizeof(int32_t), h->stream));
  h->cnt_send_zeroed = false;
  if (h->S > 0) {
    CountParams cp{};
    cp.zw = h->d_zw; cp.seg_word = h->d_seg_word; cp.seg_begin = h->d_seg_begin; cp.n_wk = dst; cp.K = h->K; cp.num_segs = (int32_t)h->S;
    cp.koff = h->xg ? h->d_koff : nullptr; cp.row_stride = h->xg ? h->Ksm : h->K;
    cp.seg_end = nullptr; cp.segs_per_block = kCountSegsPerBlock;
    hipLaunchKernelGGL(count_sorted_kernel, dim3((unsigned)((h->S + kCountSegsPerBlock - 1) / kCountSegsPerBlock)), dim3(256), (size_t)h->K * sizeof(int32_t),
                       h->stream, cp);
  }
  HIP_TRY(h, hipGetLastError());
  h->n_k_valid = false;
  if (h->xg) { h->counts_global = false; h->cnt_own_valid = false; }
  return GGS_OK;
}
// The hot words' share of the send buffer, behind a z step whose kernels counted the cold tokens themselves.
int launch_count_hot(ggs_handle *h) {
  if (h->HS > 0) {
    CountParams cp{};
    cp.zw = h->d_zw; cp.seg_word = h->d_hseg_word; cp.seg_begin = h->d_hseg_begin; cp.seg_end = h->d_hseg_end; cp.n_wk = h->d_cnt_send; cp.K = h->K;
    cp.num_segs = (int32_t)h->HS; cp.koff = h->d_koff; cp.row_stride = h->Ksm; cp.segs_per_block = 1;
    hipLaunchKernelGGL(count_sorted_kernel, dim3((unsigned)h->HS), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, cp);
    HIP_TRY(h, hipGetLastError());
  }
  h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false;
  return GGS_OK;
}

// out[k] = sum over v, in index order, of src[v][k] (MAGNITUDE: of beta + src[v][k]) for the Ks columns of a topic
// slice -- the exact parallel formulation of ggs_exact_sum.hpp, or the element-by-element chain it replaces.
// `guided`: h->d_sum_pref already holds a guess of the running sums for these columns (the exact values of the last
// magnitude sum over the same buffer); otherwise two extra launches make one.  The walk leaves the exact running
// sums there (write_pref): the next sweep's guess, and this sweep's guess for the sum of the gammas.
template <typename T, bool MAGNITUDE>
void launch_column_sum(ggs_handle *h, const T *src, int32_t pitch, int32_t Ks, double *out, int32_t *n_k, bool guided, bool write_pref,
                       double *guess = nullptr, double *fn = nullptr) {   // work space other than the handle's d_sum_pref / d_sum_fn
  if (Ks <= 0) return;
  if (!h->exact_sum) {
    hipLaunchKernelGGL((column_chain_kernel<T, MAGNITUDE>), dim3((Ks + 7) / 8), dim3(256), 0, h->stream, src, pitch, Ks, h->V, h->beta, out);
    return;
  }
  SumParams sp{};
  sp.src = src; sp.guess = guess ? guess : h->d_sum_pref; sp.fn = fn ? fn : h->d_sum_fn; sp.out = out; sp.beta = h->beta; sp.n_k = n_k;
  sp.pitch = pitch; sp.K = Ks; sp.V = h->V; sp.nseg = h->sum_nseg; sp.write_pref = write_pref ? 1 : 0;
  const dim3 rows((unsigned)h->sum_nseg, (unsigned)((Ks + kSumBlock - 1) / kSumBlock));
  if (!guided) {
    hipLaunchKernelGGL((sum_seg_kernel<T, MAGNITUDE>), rows, dim3(kSumBlock), 0, h->stream, sp);
    hipLaunchKernelGGL(sum_prefix_kernel, dim3((unsigned)Ks), dim3(64), 0, h->stream, sp);
  }
  hipLaunchKernelGGL((sum_segfn_kernel<T, MAGNITUDE>), dim3((unsigned)h->sum_nseg, (unsigned)((Ks + kSegFnCols - 1) / kSegFnCols)), dim3(256), 0, h->stream, sp);
  hipLaunchKernelGGL((sum_walk_kernel<T, MAGNITUDE>), dim3((unsigned)Ks), dim3(64), 0, h->stream, sp);
}

// magnitude_k = sum_v (beta + n_kv) and tokensPerTopic for the Ks columns of `cnt`
int launch_magnitude_on(ggs_handle *h, const int32_t *cnt, int32_t pitch, int32_t Ks, double *mag, int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  if (h->exact_sum) {
    // the guess of the guided form is only a guess for the SAME columns of the SAME buffer
    const bool guided = h->sum_guided && h->guess_src == cnt && h->guess_cols == Ks;
    launch_column_sum<int32_t, true>(h, cnt, pitch, Ks, mag, n_k, guided, true);   // tokensPerTopic falls out of the segment pass
    h->guess_src = cnt; h->guess_cols = Ks;
  } else {
    HIP_TRY(h, hipMemsetAsync(n_k, 0, sizeof(int32_t) * (size_t)Ks, h->stream));
    launch_column_sum<int32_t, true>(h, cnt, pitch, Ks, mag, nullptr, false, false);
    hipLaunchKernelGGL(topic_totals_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 16)), dim3(256), (size_t)Ks * sizeof(int32_t), h->stream, cnt,
                       Ks, pitch, h->V, n_k);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// One collective of the attached exchange, on the handle's stream.
int xcall(ggs_handle *h, int rc, const char *what) {
  if (!rc) return GGS_OK;
  return set_err(h, GGS_ERR_HIP, std::string("exchange ") + what + " failed" + (h->xg->err.empty() ? "" : ": " + h->xg->err));
}
// Behind the reduce-scatter the send buffer is dead until the next z step fills it again (the z kernels add their cells
// into it, or count_sorted_kernel does): it is cleared right here, off the z step's critical path -- on the communication
// stream when the Phi phase is about to use it anyway (`defer_clear`: phi_step_b2 enqueues the fill behind the first
// all-gather, and the event the main stream waits for before the second one covers it), otherwise on the handle's stream.
int clear_send_buffer(ggs_handle *h, hipStream_t on) {
  HIP_TRY(h, hipMemsetAsync(h->d_cnt_send, 0, (size_t)h->xg->nranks * h->V * h->Ksm * sizeof(int32_t), on));
  h->cnt_send_zeroed = true;
  return GGS_OK;
}
// NOT cleared in here: inside ncclGroupStart/End a collective is only collected, and a fill enqueued beside it would land
// on the stream BEFORE it.  The callers clear once the collective is really enqueued (clear_send_buffer_if_dead); a
// buffer nobody cleared is cleared by the next z step itself.
// The sparse form of the count exchange: pair counts to the host, all-gathered; the pairs emitted at their offsets;
// all-to-all of the variable blocks; scatter-add into the zeroed slice.  Two host round trips (the sizes of what travels
// are only known on the device) -- this form is for exchanges whose dense buffer is hundreds of megabytes.
int sparse_exchange(ggs_handle *h) {
  const int n = h->xg->nranks, me = h->xg->rank;
  std::vector<int64_t> mine((size_t)n), soff((size_t)n), scnt((size_t)n), roff((size_t)n), rcnt((size_t)n);
  std::vector<int32_t> mine32((size_t)n), all((size_t)n * n);
  HIP_TRY(h, hipMemcpyAsync(mine.data(), h->d_sp_count, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  int64_t total = 0;
  for (int r = 0; r < n; ++r) {
    if (mine[(size_t)r] > INT32_MAX / 2) return set_err(h, GGS_ERR_UNSUPPORTED, "sparse count exchange: more than 2^30 pairs for one destination");
    mine32[(size_t)r] = (int32_t)mine[(size_t)r];
    soff[(size_t)r] = 2 * total; scnt[(size_t)r] = 2 * mine[(size_t)r];
    total += mine[(size_t)r];
  }
  h->sp_pairs_last = total;
  HIP_TRY(h, hipMemcpyAsync(h->d_sp_cnt32, mine32.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  int rc = xcall(h, h->xg->ops.all_gather_i32(h->xg->ops.ctx, h->d_sp_cnt32, h->d_sp_all, n, h->stream), "all_gather_i32 (pair counts)");
  if (rc) return rc;
  HIP_TRY(h, hipMemcpyAsync(all.data(), h->d_sp_all, sizeof(int32_t) * (size_t)n * n, hipMemcpyDeviceToHost, h->stream));
  // the pairs, at their destinations' offsets
  if ((size_t)(2 * total) > h->sp_send_cap) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if ((rc = dev_alloc(h, &h->d_sp_send, (size_t)(2 * total) + (size_t)(2 * total) / 8 + 64))) return rc;
    h->sp_send_cap = (size_t)(2 * total) + (size_t)(2 * total) / 8 + 64;
  }
  HIP_TRY(h, hipMemcpyAsync(h->d_sp_count, soff.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));   // the destinations' blocks
  if (h->sp_wgs > 0) {
    SparseCountParams sp = sparse_params(h);
    sp.wg_off = h->d_sp_wg_off; sp.dest_base = h->d_sp_count; sp.pairs = h->d_sp_send;
    hipLaunchKernelGGL(sparse_count_kernel<true>, dim3((unsigned)h->sp_wgs), dim3(256), (size_t)h->K * sizeof(int32_t), h->stream, sp);
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));        // `all` has arrived (and soff / mine32 may go out of scope)
  int64_t rtotal = 0;
  for (int s2 = 0; s2 < n; ++s2) {
    rcnt[(size_t)s2] = 2 * (int64_t)all[(size_t)s2 * n + me];
    roff[(size_t)s2] = rtotal;
    rtotal += rcnt[(size_t)s2];
  }
  if ((size_t)rtotal > h->sp_recv_cap) {
    if ((rc = dev_alloc(h, &h->d_sp_recv, (size_t)rtotal + (size_t)rtotal / 8 + 64))) return rc;
    h->sp_recv_cap = (size_t)rtotal + (size_t)rtotal / 8 + 64;
  }
  if ((rc = xcall(h, h->xg->ops.all_to_all_v_i32(h->xg->ops.ctx, h->d_sp_send, soff.data(), scnt.data(), h->d_sp_recv, roff.data(), rcnt.data(), h->stream), "all_to_all_v_i32")))
    return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_cnt_own, 0, sizeof(int32_t) * (size_t)h->V * h->Ksm, h->stream));
  if (rtotal > 0) {
    hipLaunchKernelGGL(scatter_add_pairs_kernel, dim3(grid_for(rtotal / 2, 256)), dim3(256), 0, h->stream, h->d_sp_recv, rtotal / 2, h->d_cnt_own);
    HIP_TRY(h, hipGetLastError());
  }
  HIP_TRY(h, hipStreamSynchronize(h->stream));        // the host arrays handed to the transport stay alive until it has used them
  h->cnt_own_valid = true;
  return GGS_OK;
}
int launch_count_rebuild(ggs_handle *h);
int exchange_reduce_scatter(ggs_handle *h) {
  if (h->cnt_own_valid) return GGS_OK;
  if (use_sparse(h) != h->counted_sparse) {            // the form was switched between the count and its exchange: count again in the form that travels
    int rc = launch_count_rebuild(h);
    if (rc) return rc;
  }
  if (use_sparse(h)) return sparse_exchange(h);
  int rc = xcall(h, h->xg->ops.reduce_scatter_i32(h->xg->ops.ctx, h->d_cnt_send, h->d_cnt_own, (int64_t)h->V * h->Ksm, h->stream), "reduce_scatter_i32");
  if (rc) return rc;
  h->cnt_own_valid = true;
  h->cnt_send_zeroed = false;
  return GGS_OK;
}
// the send buffer's contents have been through the reduce-scatter (cnt_own is their sum): dead, clear them on `on`
int clear_send_buffer_if_dead(ggs_handle *h, hipStream_t on) {
  if (!h->xg || h->cnt_send_zeroed || !h->cnt_own_valid || use_sparse(h)) return GGS_OK;
  return clear_send_buffer(h, on);
}

// Corpus-wide counts in d_n_wk: with an exchange, gathered from the ranks' slices on demand (a COLLECTIVE call).  In
// steps, so that a one-process group can issue each collective for all of its devices inside ncclGroupStart/End.
int gather_counts_step_gather(ggs_handle *h) {
  const size_t cells = (size_t)h->xg->nranks * h->V * h->Ksm;
  int rc;
  if (!h->d_cnt_all && (rc = dev_alloc(h, &h->d_cnt_all, cells))) return rc;
  return xcall(h, h->xg->ops.all_gather_i32(h->xg->ops.ctx, h->d_cnt_own, h->d_cnt_all, (int64_t)h->V * h->Ksm, h->stream), "all_gather_i32");
}
int gather_counts_step_unslice(ggs_handle *h) {
  hipLaunchKernelGGL(counts_unslice_kernel, dim3(grid_for((int64_t)h->K * h->V, 256)), dim3(256), 0, h->stream, h->d_cnt_all, h->d_koff, h->Ksm, h->d_n_wk,
                     h->K, h->V);
  HIP_TRY(h, hipGetLastError());
  h->counts_global = true; h->n_k_valid = false;
  return GGS_OK;
}
int ensure_global_counts(ggs_handle *h) {
  if (!h->xg || h->counts_global) return GGS_OK;
  int rc;
  if ((rc = exchange_reduce_scatter(h)) || (rc = clear_send_buffer_if_dead(h, h->stream)) || (rc = gather_counts_step_gather(h))) return rc;
  return gather_counts_step_unslice(h);
}

// tokensPerTopic (and the Dirichlet magnitudes) of the corpus-wide counts
int launch_magnitude(ggs_handle *h) {
  int rc = ensure_global_counts(h);
  if (rc) return rc;
  if (h->n_k_valid) return GGS_OK;
  if ((rc = launch_magnitude_on(h, h->d_n_wk, h->K, h->K, h->d_mag, h->d_n_k))) return rc;
  h->n_k_valid = true;
  return GGS_OK;
}

// Topic priors (ggs_set_topic_priors).  The sweep draw is then the CONDITIONAL one (conditional_phi): the masked gamma draw, and
// (g / sum_gamma) * sum_phi in place of the division and its clamp.  sum_phi[k], the index-order sum of the OLD phi row (masked
// cells are +0.0 and leave the running sum as it is), is an exact column sum of phiT over all K topics -- every rank of an exchange
// holds the whole old phiT and sums it for itself -- taken before anything overwrites phiT, unguided, in work space of its own.
// The initial draw runs to its end as ever and is then multiplied by the priors (phi_apply_priors).
bool conditional_phi(const ggs_handle *h, bool initial) { return h->have_priors && !initial; }
// scheme=nzvsspalias: the sweep draw is the variable-selection one (ggs_phi_vs.hpp); the initial draw is pcgs's
bool vs_phi(const ggs_handle *h, bool initial) { return h->scheme == Scheme::nzvsspalias && !initial; }
// ... and what a draw leaves the words' lists to be built from: nothing (the initial Phi), or its drawn cells
void vs_note_draw(ggs_handle *h, bool initial) {
  if (h->scheme == Scheme::nzvsspalias) { h->vs_lists = initial ? ggs_handle::VsLists::empty : ggs_handle::VsLists::drawn; if (initial) h->vs_drawn = false; }
}
// The indicator chain of the topics [k0, k0 + Ks) from their counts cnt [V][cnt_pitch] (tokensPerTopic in n_k) and the Phi now
// in d_phiT: the undrawn cells into d_vs_und (by topic) and d_vs_mask (by word).  Before anything overwrites phiT.
int launch_vs_chain(ggs_handle *h, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, const int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  VsBitsParams bp{};
  bp.cnt = cnt; bp.phiT = h->d_phiT; bp.cz = h->d_vs_cz; bp.pz = h->d_vs_pz;
  bp.cnt_pitch = cnt_pitch; bp.Kp = h->Kp; bp.k0 = k0; bp.Ks = Ks; bp.V = h->V; bp.W = h->vs_W;
  void *bargs[] = {&bp};
  HIP_TRY(h, launch(h, h->plan.vsbits, (int64_t)h->vs_W * ((Ks + 63) / 64), bargs, h->stream));
  VsChainParams cp{};
  cp.cz = h->d_vs_cz; cp.pz = h->d_vs_pz; cp.und = h->d_vs_und; cp.work = h->d_vs_work; cp.n_k = n_k; cp.u = nullptr;
  cp.s_end = h->d_vs_s_end; cp.rounds = h->d_vs_rounds; cp.status = h->d_status; cp.seed = h->seed; cp.iteration = (uint32_t)h->iteration;
  cp.Ks = Ks; cp.k0 = k0; cp.V = h->V; cp.W = h->vs_W; cp.beta = h->beta; cp.odds = h->vs_pi / (1 - h->vs_pi);
  void *cargs[] = {&cp};
  HIP_TRY(h, hipLaunchKernel(h->plan.vschain.fn, dim3((unsigned)Ks), dim3(kVsBlock), cargs, (size_t)h->plan.vschain.lds, h->stream));   // a workgroup per topic
  hipLaunchKernelGGL(vs_mask_kernel, dim3(grid_for((int64_t)h->V * h->vs_pitch, 256)), dim3(256), 0, h->stream, h->d_vs_und, h->vs_W, k0, Ks, h->V, h->vs_pitch,
                     h->d_vs_mask);
  HIP_TRY(h, hipGetLastError());
  h->vs_drawn = true;
  return GGS_OK;
}
int launch_sum_phi(ggs_handle *h) {
  launch_column_sum<double, false>(h, h->d_phiT, h->Kp, h->K, h->d_pr_sum_phi, nullptr, false, false, h->d_pr_pref, h->d_pr_fn);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_apply_priors(ggs_handle *h) {
  hipLaunchKernelGGL(phi_apply_priors_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_phiT, h->d_pr_mask, h->pr_pitch, h->K,
                     h->Kp, h->V, h->d_phiT32, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  h->alias_stale = true;
  return GGS_OK;
}

// Phi draw: initial (K8) or per sweep (K6) for the topics [k0, k0 + Ks) from their corpus-wide counts
// cnt [V][cnt_pitch]; rows into out [V][out_pitch].  In steps, so that the exchange can slot its collectives in:
//   phi_slice_magnitude   the Dirichlet magnitudes (and tokensPerTopic)
//   phi_slice_gamma       the gamma draws of the segments [seg0, seg1) + the segment functions of their column sums
//   phi_slice_total       the walk of those: tot[k] = sum_v gamma, in index order
//   phi_slice_normalise   one GPU: divide in place (with an exchange the division is done by the repack kernel)
int phi_slice_gamma(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                    const double *mag, int32_t seg0, int32_t seg1) {
  if (Ks <= 0 || seg1 <= seg0) return GGS_OK;
  PhiGammaParams gp{};
  gp.n_wk = cnt; gp.mag = mag; gp.phiT = out; gp.status = h->d_status;
  gp.seed = h->seed; gp.iteration = (uint32_t)h->iteration;
  gp.purpose = initial ? GGS_PURPOSE_INIT_PHI : GGS_PURPOSE_PHI;
  gp.K = Ks; gp.Kp = out_pitch; gp.V = h->V; gp.cnt_pitch = cnt_pitch; gp.k0 = k0; gp.beta = h->beta;
  // Dirichlet(int size, double beta): magnitude = V*beta, partition = 1.0/V
  gp.prior_pm = (1.0 / (double)h->V) * ((double)h->V * h->beta);
  gp.initial = initial ? 1 : 0;
  // tiles of one 64-row segment x kc <= kPhiCols topics, the column groups as equal as they come.  A single wave per
  // tile issues an instruction every ~8 cycles, so what makes the draw fast is waves per SIMD: a narrow slice (one rank
  // in eight draws 13 topics) is cut into narrower tiles until there are ~4 waves for each of the chip's SIMDs; the price
  // is a thinner leftover queue per tile (the general rejection loops then run with fewer lanes in use).
  const int64_t want_tiles = (int64_t)h->num_cus * 4 * 4;
  int kc_cap = (int)std::min<int64_t>(kPhiCols, std::max<int64_t>(2, (int64_t)Ks * (seg1 - seg0) / want_tiles));
  if (const char *e = debug_env("GGS_DEBUG_PHICOLS")) kc_cap = std::max(1, std::min(kPhiCols, std::atoi(e)));
  gp.ncg = (Ks + kc_cap - 1) / kc_cap;
  gp.kc = (Ks + gp.ncg - 1) / gp.ncg;
  gp.ncg = (Ks + gp.kc - 1) / gp.kc;
  gp.seg_begin = seg0; gp.seg_end = seg1;
  gp.queue_cap = std::min(kPhiQueue, h->gamma_queue_cap);
  gp.prio = h->xg ? 1 : 0;
  gp.guess = h->exact_sum ? h->d_sum_pref : nullptr; gp.fn = h->d_sum_fn;
  const int64_t tiles = (int64_t)(seg1 - seg0) * gp.ncg;
  // single-wave workgroups; a grid of at most 32 per CU, the rest by striding
  const dim3 grid((unsigned)std::min<int64_t>(tiles, (int64_t)h->num_cus * 32));
  if (conditional_phi(h, initial)) {                   // the masked draw; its sums' guess is still the magnitudes' (any guess will do)
    gp.zero_mask = h->d_pr_mask; gp.mask_pitch = h->pr_pitch;
    hipLaunchKernelGGL(phi_gamma_kernel<true>, grid, dim3(64), 0, h->stream, gp);
  } else if (vs_phi(h, initial)) {                     // the cells the indicator chain left undrawn are masked; shape = beta + n
    gp.zero_mask = h->d_vs_mask; gp.mask_pitch = h->vs_pitch;
    gp.undrawn_negative = h->xg ? 1 : 0;               // the drawn set travels in the gathered gammas' signs of zero (phi_step_c)
    hipLaunchKernelGGL(phi_gamma_vs_kernel, grid, dim3(64), 0, h->stream, gp);
  } else {
    hipLaunchKernelGGL(phi_gamma_kernel<false>, grid, dim3(64), 0, h->stream, gp);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_slice_total(ggs_handle *h, const double *out, int32_t out_pitch, int32_t Ks, double *tot) {
  if (Ks <= 0) return GGS_OK;
  if (h->exact_sum) {
    SumParams sp{};
    sp.src = out; sp.guess = h->d_sum_pref; sp.fn = h->d_sum_fn; sp.out = tot; sp.beta = h->beta; sp.n_k = nullptr;
    sp.pitch = out_pitch; sp.K = Ks; sp.V = h->V; sp.nseg = h->sum_nseg; sp.write_pref = 0;   // the guess stays the magnitudes' running sums
    hipLaunchKernelGGL((sum_walk_kernel<double, false>), dim3((unsigned)Ks), dim3(64), 0, h->stream, sp);
  } else {
    launch_column_sum<double, false>(h, out, out_pitch, Ks, tot, nullptr, false, false);
  }
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
// scheme=polyaurn: the Poisson draws of the rows [seg0, seg1) * 64 (ggs_phi_poisson.hpp) into out, their integer totals
// into d_pa_acc -- zeroed first by the draw's first launch (`first`), so the two halves of an exchange's draw add up
int phi_slice_poisson(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                      int32_t seg0, int32_t seg1, bool first) {
  if (Ks <= 0) return GGS_OK;
  if (first) HIP_TRY(h, hipMemsetAsync(h->d_pa_acc, 0, sizeof(unsigned long long) * kPoissonAccStride * (size_t)Ks, h->stream));
  if (seg1 <= seg0) return GGS_OK;
  PhiPoissonParams pp{};
  pp.cnt = cnt; pp.out = out; pp.table = h->d_pa_table; pp.acc = h->d_pa_acc; pp.status = h->d_status;
  pp.seed = h->seed; pp.iteration = (uint32_t)h->iteration; pp.purpose = initial ? GGS_PURPOSE_INIT_PHI : GGS_PURPOSE_PHI;
  pp.Ks = Ks; pp.out_pitch = out_pitch; pp.cnt_pitch = cnt_pitch; pp.k0 = k0; pp.V = h->V;
  pp.row_begin = seg0 * kSumSegRows; pp.row_end = std::min(h->V, seg1 * kSumSegRows);
  pp.L = h->pa_L; pp.beta = h->beta; pp.t00 = h->pa_t00;
  // tiles sized by the launch's work, as phi_slice_gamma sizes its own: about eight per CU, at least one cell per thread (a
  // narrow slice -- one rank in eight draws 13 topics -- gets many short tiles); two workgroups per CU take them by grid
  // stride, so the totals cost 2 * Ks atomics per workgroup whatever the tile count
  const int64_t rows = pp.row_end - pp.row_begin, cells = rows * Ks;
  const int64_t want = std::max<int64_t>(kPoissonThreads, cells / ((int64_t)h->num_cus * 8));
  pp.rows_per_tile = (int32_t)std::max<int64_t>(1, std::min<int64_t>(rows, (want + Ks - 1) / Ks));
  const int64_t tiles = (rows + pp.rows_per_tile - 1) / pp.rows_per_tile;
  hipLaunchKernelGGL(phi_poisson_kernel, dim3((unsigned)std::min<int64_t>(tiles, (int64_t)h->num_cus * 2)), dim3(kPoissonThreads), (size_t)Ks * 12, h->stream, pp);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int phi_slice_poisson_totals(ggs_handle *h, int32_t Ks, double *tot, int32_t *n_k) {
  if (Ks <= 0) return GGS_OK;
  hipLaunchKernelGGL(phi_poisson_totals_kernel, dim3((unsigned)((Ks + 255) / 256)), dim3(256), 0, h->stream, h->d_pa_acc, Ks, tot, n_k);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}
int launch_phi_slice(ggs_handle *h, bool initial, const int32_t *cnt, int32_t cnt_pitch, int32_t Ks, int32_t k0, double *out, int32_t out_pitch,
                     double *mag, double *tot, int32_t *n_k, double *phi_mean) {
  if (Ks <= 0) return GGS_OK;
  int rc;
  if (poisson_phi(h->scheme)) {   // no magnitudes, no gammas, no exact-sum walk: the totals are integers
    if ((rc = phi_slice_poisson(h, initial, cnt, cnt_pitch, Ks, k0, out, out_pitch, 0, h->sum_nseg, true)) || (rc = phi_slice_poisson_totals(h, Ks, tot, n_k)))
      return rc;
    hipLaunchKernelGGL(phi_normalise_polyaurn_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V,
                       phi_mean, out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
    HIP_TRY(h, hipGetLastError());
    return GGS_OK;
  }
  // (nzvsspalias: the magnitudes are not the draw's, but their pass leaves tokensPerTopic for the chain and a guess for the sums)
  if ((rc = launch_magnitude_on(h, cnt, cnt_pitch, Ks, mag, n_k)) || (vs_phi(h, initial) && (rc = launch_vs_chain(h, cnt, cnt_pitch, Ks, k0, n_k))) ||
      (rc = phi_slice_gamma(h, initial, cnt, cnt_pitch, Ks, k0, out, out_pitch, mag, 0, h->sum_nseg)) || (rc = phi_slice_total(h, out, out_pitch, Ks, tot)))
    return rc;
  if (vs_phi(h, initial))                              // x / sum, a row of sum 0 all +0.0; the reference's loopOverTopics override never adds to the phi mean
    hipLaunchKernelGGL(phi_normalise_polyaurn_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V,
                       static_cast<double *>(nullptr), out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  else if (conditional_phi(h, initial))                     // one GPU: the slice is the whole matrix, sum_phi's columns are its columns
    hipLaunchKernelGGL(phi_normalise_conditional_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, h->d_pr_sum_phi, Ks,
                       out_pitch, h->V, phi_mean, out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  else
    hipLaunchKernelGGL(phi_normalise_kernel, dim3(grid_for((int64_t)Ks * h->V, 256, 2)), dim3(256), 0, h->stream, out, tot, Ks, out_pitch, h->V, phi_mean,
                       out == h->d_phiT ? h->d_phiT32 : nullptr, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// The steps of the Phi phase with an exchange attached (ggs_group_sweep issues each for all handles of a one-process
// group, the collective ones inside ncclGroupStart/End; one handle per process runs them back to back):
//   A     reduce-scatter of the counts by topic slice
//   B1    this rank's slice: magnitudes, the gammas of the first half of the vocabulary
//   G0    all-gather of that half on the communication stream -- it runs UNDER step B2
//   B2    the gammas of the second half, then the walk of the column sums (it needs every gamma of the slice)
//   G1    all-gather of the second half with the Ksm column sums behind it, on the main stream, issued behind G0
//   C     repack [nranks][..] -> phiT [V][Kp], dividing by the owner's column sum on the way (the same IEEE division
//         the one-GPU normalise kernel does: bit-identical) (+ the running phi mean)
// What travels is therefore the UNNORMALISED gammas: the division does not have to wait for the slice to be complete
// before the first bytes go out.  Events are recorded by the callers AFTER a grouped step (inside
// ncclGroupStart/End the collectives are only collected, not enqueued).
size_t half0_elems(const ggs_handle *h) { return (size_t)h->v_split * h->Ksm; }
size_t half1_elems(const ggs_handle *h) { return (size_t)(h->V - h->v_split) * h->Ksm + (size_t)h->Ksm; }
int phi_step_a(ggs_handle *h) { return exchange_reduce_scatter(h); }
// behind step A, outside any ncclGroupStart/End: a short vocabulary has no communication-stream step to hide the fill under
int phi_step_a_clear(ggs_handle *h) { return h->seg_split > 0 ? GGS_OK : clear_send_buffer_if_dead(h, h->stream); }
int phi_step_b1(ggs_handle *h, bool initial) {
  int rc;
  if (conditional_phi(h, initial) && (rc = launch_sum_phi(h))) return rc;   // phiT is the old Phi until step C
  if (poisson_phi(h->scheme)) {   // the Poisson draws of the first half (and the totals' zero fill)
    if ((rc = phi_slice_poisson(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, 0, h->seg_split, true))) return rc;
  } else if ((rc = launch_magnitude_on(h, h->d_cnt_own, h->Ksm, h->Ks, h->d_mag_own, h->d_n_k_own))) {
    return rc;
  }
  // nzvsspalias: the indicator chain of the rank's own topics, from their corpus-wide counts and the old Phi (phiT until step C);
  // d_vs_mask then holds the slice's undrawn cells for the two halves' draws
  if (vs_phi(h, initial) && (rc = launch_vs_chain(h, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_n_k_own))) return rc;
  if (h->seg_split > 0) {
    if (!poisson_phi(h->scheme) && (rc = phi_slice_gamma(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->d_mag_own, 0, h->seg_split))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_half_drawn, h->stream));
    HIP_TRY(h, hipStreamWaitEvent(h->comm_stream, h->ev_half_drawn, 0));
  }
  return GGS_OK;
}
int phi_step_g0(ggs_handle *h) {
  if (h->seg_split <= 0) return GGS_OK;
  return xcall(h, h->xg->ops.all_gather_f64(h->xg->ops.ctx, h->d_phi_own, h->d_phi_all0, (int64_t)half0_elems(h), h->comm_stream), "all_gather_f64");
}
int phi_step_b2(ggs_handle *h, bool initial) {
  int rc;
  if (h->seg_split > 0) {
    // behind the first all-gather on the communication stream (which waited for the slice's first half, hence for the
    // reduce-scatter before it): the send buffer's zero fill, deferred by phi_step_a
    if ((rc = clear_send_buffer_if_dead(h, h->comm_stream))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_half_gathered, h->comm_stream));
  }
  if (poisson_phi(h->scheme)) {   // the second half, then the integer totals into the slot behind the slice
    if ((rc = phi_slice_poisson(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->seg_split, h->sum_nseg, false))) return rc;
    return phi_slice_poisson_totals(h, h->Ks, h->d_phi_own + (size_t)h->V * h->Ksm, h->d_n_k_own);
  }
  if ((rc = phi_slice_gamma(h, initial, h->d_cnt_own, h->Ksm, h->Ks, h->k0, h->d_phi_own, h->Ksm, h->d_mag_own, h->seg_split, h->sum_nseg))) return rc;
  return phi_slice_total(h, h->d_phi_own, h->Ksm, h->Ks, h->d_phi_own + (size_t)h->V * h->Ksm);
}
int phi_step_g1(ggs_handle *h) {
  return xcall(h, h->xg->ops.all_gather_f64(h->xg->ops.ctx, h->d_phi_own + half0_elems(h), h->d_phi_all1, (int64_t)half1_elems(h), h->stream), "all_gather_f64");
}
int phi_join_halves(ggs_handle *h) {                   // the main stream goes on only when the first half has arrived too
  if (h->seg_split > 0) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_half_gathered, 0));
  return GGS_OK;
}
int phi_step_c(ggs_handle *h, bool initial, bool accumulate_mean) {
  PhiRepackParams rp{};
  rp.all0 = h->d_phi_all0; rp.all1 = h->d_phi_all1; rp.krank = h->d_krank; rp.kcol = h->d_kcol; rp.phiT = h->d_phiT;
  rp.phi_mean = accumulate_mean ? h->d_phi_mean : nullptr;
  rp.c0 = (int64_t)half0_elems(h); rp.c1 = (int64_t)half1_elems(h); rp.K = h->K; rp.Kp = h->Kp; rp.V = h->V; rp.Ksm = h->Ksm; rp.v_split = h->v_split;
  rp.phiT32 = h->d_phiT32; rp.Kp32 = h->plan.Kp32; rp.sum_phi = h->d_pr_sum_phi;
  if (vs_phi(h, initial)) {                            // every topic's undrawn cells from the signs of zero, then the repack that clears them
    rp.phi_mean = nullptr;                             // the reference's loopOverTopics override never adds to the phi mean
    hipLaunchKernelGGL(vs_mask_gathered_kernel, dim3(grid_for((int64_t)h->V * h->vs_pitch, 256)), dim3(256), 0, h->stream, rp, h->d_vs_mask, h->vs_pitch);
    hipLaunchKernelGGL(phi_repack_vs_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  } else if (poisson_phi(h->scheme)) hipLaunchKernelGGL(phi_repack_polyaurn_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  else if (conditional_phi(h, initial)) hipLaunchKernelGGL(phi_repack_conditional_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  else hipLaunchKernelGGL(phi_repack_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, rp);
  HIP_TRY(h, hipGetLastError());
  h->have_phi = true;
  h->alias_stale = true;
  vs_note_draw(h, initial);
  if (h->have_priors && initial) return phi_apply_priors(h);
  return GGS_OK;
}

// scheme=spalias: the alias tables of the Phi now in d_phiT (ggs_alias.hpp), on the handle's stream.  Called wherever Phi
// changes (the draws below, ggs_set_phi), inside the span ggs_get_timings counts as phi_ms.  With an exchange every rank
// holds the whole Phi after the all-gather and builds all V words for itself: what a rank's shard contains changes
// with the corpus, the tables' layout does not.
int launch_alias_build(ggs_handle *h) {
  if (!has_alias(h->scheme)) return GGS_OK;
  AliasParams ap{};
  ap.phiT = h->d_phiT; ap.alpha = h->d_alpha; ap.ps = h->d_alias_ps; ap.a = h->d_alias_a; ap.type_norm = h->d_alias_tn;
  ap.V = h->V; ap.K = h->K; ap.Kp = h->Kp; ap.wpb = h->plan.alias_wpb;
  void *args[] = {&ap};
  HIP_TRY(h, launch(h, h->plan.alias, ((int64_t)h->V + ap.wpb - 1) / ap.wpb, args, h->stream));
  if (h->scheme == Scheme::nzvsspalias && h->vs_lists == ggs_handle::VsLists::empty) {   // the reference fills no list before its first samplePhi
    HIP_TRY(h, hipMemsetAsync(h->d_nw, 0, (size_t)h->V * sizeof(int32_t), h->stream));
  } else if (doubly_sparse(h->scheme)) {               // the words' lists of non-zero topics, of the same Phi (nzvsspalias after a sweep: of its drawn cells)
    const bool from_mask = h->vs_lists == ggs_handle::VsLists::drawn;   // nzvsspalias alone has them (vs_note_draw)
    WordListParams wp{};
    wp.phiT = h->d_phiT; wp.nzw = h->d_nzw; wp.nw = h->d_nw; wp.V = h->V; wp.K = h->K; wp.Kp = h->Kp;
    wp.zero_mask = h->d_vs_mask; wp.mask_pitch = h->vs_pitch;
    void *wargs[] = {&wp};
    HIP_TRY(h, launch(h, from_mask ? h->plan.wordmask : h->plan.wordlist, h->V, wargs, h->stream));
  }
  h->alias_stale = false;
  return GGS_OK;
}

// The head of a count-form scheme's z step (launch_sweep_head), on the handle's stream: what the step conditions on, of the
// corpus-wide counts now in d_n_wk / d_n_k; also run for the getters.  With an exchange every rank holds the gathered counts and
// builds all for itself.  scheme=lightcollapsed: the words' lists and tables (count_alias_build_kernel)
int launch_count_alias_build(ggs_handle *h) {
  CountAliasParams cp{};
  cp.n_wk = h->d_n_wk; cp.n_k = h->d_n_k; cp.ps = h->d_alias_ps; cp.a = h->d_alias_a; cp.type_norm = h->d_alias_tn;
  cp.nzw = h->d_nzw; cp.nw = h->d_nw; cp.tpt = h->d_tpt; cp.beta_sum = h->beta * (double)h->V;
  cp.V = h->V; cp.K = h->K; cp.wpb = h->plan.alias_wpb;
  void *args[] = {&cp};
  HIP_TRY(h, launch(h, h->plan.countalias, ((int64_t)h->V + cp.wpb - 1) / cp.wpb, args, h->stream));
  return GGS_OK;
}

// scheme=adlda: den0, S0 and the words' lists
int launch_adlda_head(ggs_handle *h) {
  AdldaHeadParams hp{};
  hp.n_k = h->d_n_k; hp.alpha = h->d_alpha; hp.den0 = h->d_ad_den0; hp.s0 = h->d_ad_s0; hp.beta = h->beta; hp.beta_sum = h->beta * (double)h->V; hp.K = h->K;
  void *hargs[] = {&hp};
  HIP_TRY(h, launch(h, h->plan.adhead, 1, hargs, h->stream));
  WordListParams wp{};
  wp.counts = h->d_n_wk; wp.nzw = h->d_nzw; wp.nw = h->d_nw; wp.V = h->V; wp.K = h->K; wp.Kp = h->Kp;
  void *wargs[] = {&wp};
  HIP_TRY(h, launch(h, h->plan.adlists, h->V, wargs, h->stream));
  return GGS_OK;
}

int launch_sweep_head(ggs_handle *h) {
  const int rc = launch_magnitude(h);                  // the counts gathered, tokensPerTopic in step with them
  if (rc) return rc;
  if (count_tables(h->scheme)) return launch_count_alias_build(h);   // lightpcldaw2 too: Phi is not touched
  if (h->scheme == Scheme::adlda) return launch_adlda_head(h);
  // collapsed: the ratios (beta + n_wk)/(betaSum + n_k) into phiT, for the pcgs loop over them
  hipLaunchKernelGGL(psi_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_n_wk, h->d_n_k, h->beta, h->beta * (double)h->V, h->d_phiT,
                     h->K, h->Kp, h->V);
  HIP_TRY(h, hipGetLastError());
  return GGS_OK;
}

// Phi draw: initial (K8) or per sweep (K6).  One GPU: the whole matrix in place (and tokensPerTopic refreshed);
// with an exchange: steps A, B, C above.
int launch_phi(ggs_handle *h, bool initial, bool accumulate_mean, Events *E = nullptr) {
  int rc;
  if (h->xg) {
    if ((rc = phi_step_a(h)) || (rc = phi_step_a_clear(h))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[0], h->stream));
    if ((rc = phi_step_b1(h, initial)) || (rc = phi_step_g0(h)) || (rc = phi_step_b2(h, initial))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[1], h->stream));
    // the second all-gather is issued only behind the first: no two collectives of one communicator are ever in flight
    // on different streams at once (they could not share the links anyway), whatever the transport does about that itself
    if ((rc = phi_join_halves(h)) || (rc = phi_step_g1(h))) return rc;
    if (E) HIP_TRY(h, hipEventRecord(E->x[2], h->stream));
    if ((rc = phi_step_c(h, initial, accumulate_mean))) return rc;
    return launch_alias_build(h);
  }
  if (conditional_phi(h, initial) && (rc = launch_sum_phi(h))) return rc;   // before the draw overwrites phiT
  if ((rc = launch_phi_slice(h, initial, h->d_n_wk, h->K, h->K, 0, h->d_phiT, h->Kp, h->d_mag, h->d_tot, h->d_n_k, accumulate_mean ? h->d_phi_mean : nullptr)))
    return rc;
  h->n_k_valid = true;
  h->have_phi = true;
  vs_note_draw(h, initial);
  if (h->have_priors && initial && (rc = phi_apply_priors(h))) return rc;
  return launch_alias_build(h);
}

// `lds`, `docs_per_block`: 0 = those of the corpus' configuration (plan.cfg_plain / cfg_parts)
int launch_theta(ggs_handle *h, hipStream_t stream, double *dst, int32_t iteration, int64_t d0 = 0, int64_t d1 = -1, int32_t lds = 0, int32_t docs_per_block = 0) {
  if (d1 < 0) d1 = h->D;
  if (d1 <= d0) return GGS_OK;
  if (docs_per_block <= 0) docs_per_block = h->cfg->theta_docs;
  ThetaParams tp{};
  tp.doc_ptr = h->d_doc_ptr + d0; tp.z = h->d_z; tp.alpha = h->d_alpha; tp.theta = dst + (size_t)d0 * h->K; tp.status = h->d_status;
  tp.num_docs = d1 - d0; tp.doc_base = h->doc_base + d0; tp.seed = h->seed; tp.iteration = (uint32_t)iteration;
  tp.K = h->K; tp.docs_per_block = docs_per_block; tp.queue_cap = std::min(kGammaQueue, h->gamma_queue_cap);
  tp.sym_alpha = h->alpha_symmetric ? 1 : 0;
  const int64_t grid = (d1 - d0 + docs_per_block - 1) / docs_per_block;
  void *args[] = {&tp};
  HIP_TRY(h, hipLaunchKernel(h->plan.theta.fn, dim3((unsigned)grid), dim3(kThetaBlock), args, (size_t)(lds ? lds : h->cfg->theta_lds), stream));
  return GGS_OK;
}

// z_sliced_kernel<KMAX> / z_hot_kernel<KMAX> for KMAX = K rounded up to a multiple of 8
#define GGS_KMAX_SWITCH(KERNEL)                                                                                                     \
  switch ((K + 7) / 8) {                                                                                                            \
    case 1: return reinterpret_cast<const void *>(KERNEL<8>);      case 2: return reinterpret_cast<const void *>(KERNEL<16>);       \
    case 3: return reinterpret_cast<const void *>(KERNEL<24>);     case 4: return reinterpret_cast<const void *>(KERNEL<32>);       \
    case 5: return reinterpret_cast<const void *>(KERNEL<40>);     case 6: return reinterpret_cast<const void *>(KERNEL<48>);       \
    case 7: return reinterpret_cast<const void *>(KERNEL<56>);     case 8: return reinterpret_cast<const void *>(KERNEL<64>);       \
    case 9: return reinterpret_cast<const void *>(KERNEL<72>);     case 10: return reinterpret_cast<const void *>(KERNEL<80>);      \
    case 11: return reinterpret_cast<const void *>(KERNEL<88>);    case 12: return reinterpret_cast<const void *>(KERNEL<96>);      \
    case 13: return reinterpret_cast<const void *>(KERNEL<104>);   case 14: return reinterpret_cast<const void *>(KERNEL<112>);     \
    case 15: return reinterpret_cast<const void *>(KERNEL<120>);   case 16: return reinterpret_cast<const void *>(KERNEL<128>);     \
    case 17: return reinterpret_cast<const void *>(KERNEL<136>);   case 18: return reinterpret_cast<const void *>(KERNEL<144>);     \
    case 19: return reinterpret_cast<const void *>(KERNEL<152>);   case 20: return reinterpret_cast<const void *>(KERNEL<160>);     \
    case 21: return reinterpret_cast<const void *>(KERNEL<168>);   case 22: return reinterpret_cast<const void *>(KERNEL<176>);     \
    case 23: return reinterpret_cast<const void *>(KERNEL<184>);   default: return reinterpret_cast<const void *>(KERNEL<192>);     \
  }
const void *sliced_kernel_for(int K) { GGS_KMAX_SWITCH(z_sliced_kernel) }
const void *sliced32_kernel_for(int K) { GGS_KMAX_SWITCH(z_sliced32_kernel) }

const void *hot_kernel_for(int K) { GGS_KMAX_SWITCH(z_hot_kernel) }
const void *warm_kernel_for(int K) { GGS_KMAX_SWITCH(z_warm_kernel) }
const void *pcgs_kernel_for(int K) { GGS_KMAX_SWITCH(pcgs_sliced_kernel) }
const void *polyaurn_kernel_for(int K) { GGS_KMAX_SWITCH(polyaurn_sliced_kernel) }
const void *collapsed_kernel_for(int K) {
  switch ((K + 7) / 8) {
#define GGS_CK(N) case N: return reinterpret_cast<const void *>(pcgs_sliced_kernel<8 * N, true>);
    GGS_CK(1) GGS_CK(2) GGS_CK(3) GGS_CK(4) GGS_CK(5) GGS_CK(6) GGS_CK(7) GGS_CK(8) GGS_CK(9) GGS_CK(10) GGS_CK(11) GGS_CK(12)
    GGS_CK(13) GGS_CK(14) GGS_CK(15) GGS_CK(16) GGS_CK(17) GGS_CK(18) GGS_CK(19) GGS_CK(20) GGS_CK(21) GGS_CK(22) GGS_CK(23)
#undef GGS_CK
    default: return reinterpret_cast<const void *>(pcgs_sliced_kernel<192, true>);
  }
}

// pcgs_wave_kernel<NB, COLLAPSED> (scheme polyaurn: polyaurn_wave_kernel<NB>) for NB = blocks of 128 topics, rounded up to a
// power of two
const void *pcgs_wave_kernel_for(int nb, bool collapsed, bool polyaurn) {
#define GGS_WK(N) if (nb <= N) return polyaurn ? reinterpret_cast<const void *>(polyaurn_wave_kernel<N>) : collapsed ? reinterpret_cast<const void *>(pcgs_wave_kernel<N, true>) : reinterpret_cast<const void *>(pcgs_wave_kernel<N, false>);
  GGS_WK(1) GGS_WK(2) GGS_WK(4) GGS_WK(8) GGS_WK(16)
#undef GGS_WK
  return polyaurn ? reinterpret_cast<const void *>(polyaurn_wave_kernel<32>) : collapsed ? reinterpret_cast<const void *>(pcgs_wave_kernel<32, true>) : reinterpret_cast<const void *>(pcgs_wave_kernel<32, false>);
}
constexpr int kPcgsWaveMaxTopics = 32 * 128;          // 4096: two rows of K/64 doubles per lane in registers
// Where the wave-per-document kernel takes over from the lane-per-document score-register kernels (which exist up to 192
// topics; their 176..192 variants spill 12-164 bytes per lane to scratch).  Measured on the benchmark corpus, z step in ms,
// lane-per-document / wave-per-document (round 4, after the wave kernel's rework; the wave kernel's time steps with the
// number of 128-topic blocks: flat up to 128 topics, flat from 129 to 256):
//   pcgs       K = 100: 2.51 / 3.33, 128: 3.69 / 3.3, 144: 4.02 / 4.9, 160: 4.28 / 4.9, 176: 4.69 / 4.9, 192: 6.04 / 5.0
//   collapsed  K = 100: 3.60 / 3.74, 128: 6.31 / 3.71, 144: 6.96 / 5.6, 160: 7.63 / 5.6, 176: 8.62 / 5.6, 192: 11.4 / 5.6
constexpr int kPcgsWaveFromTopics = 176, kCollapsedWaveFromTopics = 96;
// scheme polyaurn: the lane-per-document kernels up to 168 topics -- polyaurn_sliced_kernel<176> spills to scratch where
// pcgs_sliced_kernel<176> spills less, and the two kernels' times are within 10 % of each other there (pcgs above)
constexpr int kPolyaurnWaveFromTopics = 168;

const void *tile_kernel_for(int K) {
  const int nt = (K + 63) / 64;
  return nt <= 1 ? reinterpret_cast<const void *>(z_kernel<1>) : nt <= 2 ? reinterpret_cast<const void *>(z_kernel<2>)
       : nt <= 4 ? reinterpret_cast<const void *>(z_kernel<4>) : nt <= 8 ? reinterpret_cast<const void *>(z_kernel<8>)
       : nt <= 16 ? reinterpret_cast<const void *>(z_kernel<16>) : reinterpret_cast<const void *>(z_kernel<20>);
}
const void *stream_kernel_for(bool two_pass, bool regck, int group) {
  if (two_pass) return reinterpret_cast<const void *>(z_stream_kernel);
  if (!regck) return reinterpret_cast<const void *>(z_stream1_kernel<false, 4>);
  return group == 1 ? reinterpret_cast<const void *>(z_stream1_kernel<true, 1>) : group == 2 ? reinterpret_cast<const void *>(z_stream1_kernel<true, 2>)
                                                                                             : reinterpret_cast<const void *>(z_stream1_kernel<true, 4>);
}
// the lane-per-document kernel of a scheme: scores in registers (K <= 192), or streamed
const void *pcgs_lane_kernel_for(int K, bool sliced, bool collapsed, bool polyaurn) {
  if (sliced) return collapsed ? collapsed_kernel_for(K) : polyaurn ? polyaurn_kernel_for(K) : pcgs_kernel_for(K);
  return collapsed ? reinterpret_cast<const void *>(pcgs_z_kernel<true>) : polyaurn ? reinterpret_cast<const void *>(polyaurn_z_kernel) : reinterpret_cast<const void *>(pcgs_z_kernel<false>);
}

// The resident single-wave workgroups per CU of a persistent grid (exactly what is resident: a workgroup that is not would walk
// its share only after the others have finished theirs): what the kernel's registers allow (asked of the runtime, whose answer
// ignores the LDS allocation granule) and what LDS allows, at most the CU's 32.
int resident_waves_per_cu(const void *fn, int lds) {
  int by_regs = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&by_regs, fn, 64, (size_t)lds) != hipSuccess || by_regs < 1) by_regs = 1;
  return lds_workgroups_per_cu(lds, std::min(by_regs, 32));
}

// Every launch a handle of (K, V, scheme) can make on the device: which kernel, how much LDS (the layout functions beside
// the kernels), how many workgroups per CU.  No environment, no handle; the only HIP calls are the occupancy queries of the
// two wave-per-document kernels.
int plan_launches(const int K, const int V, const Scheme scheme, const Knobs &kn, LaunchPlan &pl) {
  const int Kp = (K + 1) & ~1, pitch16 = (Kp / 2) | 1;
  if (scheme == Scheme::ggs) {                        // ---- the ggs z step
    // score-register kernels up to K = 160: measured on the benchmark corpus (sweep, ms; round 3) K=136: 2.13 sliced / 2.40
    // streaming, 152: 2.33 / 2.56, 160: 2.40 / 2.50, 164: 3.06 / 2.83, 168: 3.06 / 2.75, 184: 3.24 / 2.94 (round 2: 184: 3.55 /
    // 3.64, 192: 4.22 / 3.59) -- from KMAX = 168 on the cold kernel fills the whole register file (256 + 256) and the one-pass
    // streaming kernel with the next theta drawn beside it wins (the sliced kernels can take K up to kSlicedMaxTopics = 192:
    // GGS_DEBUG_ZKERNEL=1).  The sliced kernel tags chunk tokens (word ids) in bit 30.
    const bool sliced_ok = K <= kSlicedMaxTopics && V < (1 << kSlotShift);
    bool sliced = sliced_ok && K <= kSlicedDefaultTopics, stream = !sliced && K > 2 * kSliceTopics, two_pass = false;
    if (kn.zkernel.set) {          // 0: whole-row tile kernel, 1: sliced where possible, 2: streaming kernel where it applies, 3: its two-pass form
      const int mode = kn.zkernel.v;
      sliced = sliced_ok && mode == 1;
      stream = (mode == 2 || mode == 3) ? K > 2 * kSliceTopics : (stream && mode != 0);
      two_pass = mode == 3;
      if (sliced) stream = false;
    }
    pl.kernel = sliced ? 1 : stream ? (two_pass ? 3 : 2) : 0;
    // The z waves are persistent and stride the chunk table statically, so a grid is what is truly co-resident
    // (lds_workgroups_per_cu); the passes are latency chains, so waves in flight matter more than lanes in use.
    if (stream) {
      // 64-token chunks, a 2-slot slice ring + the theta row zero-padded to whole slices (one-pass kernel: to whole
      // checkpoint groups, plus a checkpoint per group and lane); no score registers, so 8 waves per CU fit the
      // register file and LDS bounds the residency
      const int ns = stream_slices(K);
      // checkpoint group: the smallest that keeps the checkpoints in registers (K <= 256: one slice, <= 512: two, <= 1024: four); beyond, four slices and LDS
      int group = ns <= kRegCheckpoints ? 1 : ns <= 2 * kRegCheckpoints ? 2 : 4;
      if (kn.group.set && (kn.group.v == 1 || kn.group.v == 2 || kn.group.v == 4)) group = kn.group.v;
      bool regck = !two_pass && z_stream1_groups(K, group) <= kRegCheckpoints;          // checkpoints in registers or in LDS
      if (kn.regck.set) regck = regck && kn.regck.v != 0;
      if (!regck) group = 4;                               // the LDS-checkpoint kernel is instantiated for groups of four
      // Chunks of 64 consecutive tokens across ONE document boundary (two theta rows per wave) instead of near-equal
      // cuts of single documents: 98 % of the lanes busy instead of 78 % at 200-token documents.  Where the second row
      // would cost resident waves (K > 512: 8 KiB at K = 1024) the single-document chunks stay.
      pl.two_rows = !two_pass && (kn.tworows.set ? kn.tworows.v != 0 : K <= 512);
      pl.z.fn = stream_kernel_for(two_pass, regck, group);
      pl.z.lds = two_pass ? z_stream_lds_bytes(K) : z_stream1_lds_bytes(K, group, pl.two_rows, regck);
      if (pl.z.lds > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;   // K > ~16000: the theta row itself would need slicing
    } else if (sliced) {
      // 64-token chunks; one 4-wave workgroup per CU (a wave per SIMD: the score registers take most of the 512-entry file),
      // per wave the two theta rows and the slice ring, per workgroup the hot-word table.  The cold chunks from phiT32 (a
      // 32-topic slice per 128 bytes); its wave LDS is the fp64 form's: the ring, then two float32 theta rows and the
      // replay's KMAX products where the two fp64 theta rows were
      pl.f32 = !kn.phi64.is(1);
      pl.Kp32 = round_up(K, kSlice32Topics);
      pl.ring_base = sliced_ring_base(K); pl.wave_lds = sliced_wave_lds(K); pl.hot_pitch = table_row_pitch(K);
      pl.hot_wave_lds = hot_wave_lds(K); pl.warm_wave_lds = warm_wave_lds(K);
      if (kn.split.set) { pl.split = kn.split.v != 0; pl.split_forced = kn.split.v == 2; }
      // split: the two workgroups must fit one CU together
      pl.hot_cap = pl.split ? table_rows_beside_cold(K, pl.hot_wave_lds) : table_rows_fused(K);
      if (kn.hot.set) pl.hot_cap = std::max(0, std::min(pl.hot_cap, kn.hot.v));
      pl.cold = {pl.f32 ? sliced32_kernel_for(K) : sliced_kernel_for(K), kSlicedWaves * 64, sliced_cold_lds(K), 1};
      pl.hot = {hot_kernel_for(K), kSlicedWaves * 64, table_lds(K, pl.hot_wave_lds, 0), 1};
      // the warm tiers: the same LDS beside the cold kernel's workgroup, more of it for theta rows (warm_docs per wave), the rest a table
      pl.warm = {warm_kernel_for(K), kSlicedWaves * 64, table_lds(K, pl.warm_wave_lds, 0), 1};
      pl.warm_docs = warm_docs_for(sliced_kmax(K));
      pl.warm_cap = table_rows_beside_cold(K, pl.warm_wave_lds);
      if (pl.warm_cap < 16) pl.warm_cap = 0;               // the table loads and barriers of a tier want tokens to pay them
      if (kn.warm.set) pl.warm_tiers_max = std::max(0, std::min(kWarmMaxTiers, kn.warm.v));
      if (kn.warm_rows.set) pl.warm_cap = std::max(0, std::min(pl.warm_cap, kn.warm_rows.v));
      if (kn.warm_fill.set) pl.warm_min_fill_pct = std::max(1, std::min(100, kn.warm_fill.v));
      if (kn.warm_cpw.set) pl.warm_min_chunks_per_wave = std::max(0, kn.warm_cpw.v);
    } else {
      // a tile of T token rows + one theta row per wave: the largest tile that still lets 6 single-wave workgroups share a
      // CU, but at least 8 rows
      int T = z_tile_rows_in(kMaxLdsBytes / 6 / kLdsGranule * kLdsGranule, Kp, pitch16);
      if (kn.tile.set) T = kn.tile.v;
      pl.tile_tokens = std::max(8, std::min(64, T));
      pl.z.fn = tile_kernel_for(K);
      pl.z.lds = z_tile_lds_bytes(Kp, pitch16, pl.tile_tokens);
      if (pl.z.lds > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;   // K > ~2400 needs a K-sliced kernel
    }
    if (!sliced) {
      pl.z.per_cu = lds_workgroups_per_cu(pl.z.lds, 8);
      if (kn.wpc.set) pl.z.per_cu = std::max(1, kn.wpc.v);
    }
  }
  // ---- the theta draw: of every sweep for scheme ggs, of the log posterior's diagnostic theta for the pcgs family
  // The documents per workgroup: by the cells alone (theta_cells_lds_bytes: the 32 KiB were measured before the cell list
  // and the class-A table came beside the cells); 32 or more are halved where the whole workgroup would pass the quarter
  // of the CU's LDS below (K = 96 - 115: 16 instead of 32, at K = 100 35.4 KiB; K = 46 - 57: 32 instead of 64).  Not below 16: with 8
  // documents the two serial K-chains of a workgroup take over (K = 200, 18 846 documents: the draw 0.48 ms instead of 0.25).
  const int theta_quarter = (kMaxLdsBytes - 24 * 1024) / 4;
  int B = 64;
  while (B > 1 && (theta_cells_lds_bytes(K, B) > 32 * 1024 || (B > 16 && theta_lds_bytes(K, B) > theta_quarter))) B >>= 1;
  if (theta_lds_bytes(K, B) > kMaxLdsBytes) return GGS_ERR_UNSUPPORTED;
  pl.theta.fn = reinterpret_cast<const void *>(theta_kernel<kThetaBlock>); pl.theta.block = kThetaBlock;
  // The request is padded to a quarter of the CU's LDS: at most 4 workgroups (16 waves) of the theta draw per CU.
  // It runs on the side stream beside the Phi phase, which is the critical path; stream priority orders dispatch,
  // not running waves, and measured with 5-6 resident workgroups theta finishes early (0.53 ms instead of 0.75)
  // while the Phi phase it starves gets longer (0.67 -> 0.72 ms).
  // ... and 24 KiB of every CU stay free for the main stream's own LDS users (the walk of the exact column sums,
  // 20.5 KiB of static LDS per workgroup, 22 KiB allocated: with the CU's LDS handed out to theta workgroups to the last
  // granule it waited for the theta draw to END -- 5 ms at K = 1024).  Workgroups of 16 documents at K = 193 - 227 pass
  // the quarter with their list (K = 200: 35.3 KiB, 36 allocated): four of them leave 16 KiB, and the walk takes the 36 KiB
  // that one of them frees when it ends.  That configuration draws theta only where the z step is in one part (D <= V: few
  // rounds of theta workgroups; measured there, 1.005 -> 0.989 ms per sweep against the build without the list).
  pl.cfg_plain = {1, pl.z.per_cu, B, std::max(theta_lds_bytes(K, B), theta_quarter), 0};
  // ... unless the theta draw is the critical leg itself (theta_main): then five workgroups per CU, of 16 documents
  // each.  Measured at K = 100 on one box, ms per sweep (documents per workgroup x workgroups per CU): 32x4 1.60-1.61,
  // 32x5 1.598-1.62, 24x5 1.593, 16x4 1.614, 16x5 1.568-1.587, 16x6 1.58, 16x8 1.598, 12x5 1.609, 8x8 1.635 -- the smaller
  // workgroups leave the Phi chain beside them its pace (0.39 ms against 0.44), so that it ends before the theta draw does.
  pl.theta_docs_main = kn.theta_b.set ? std::max(1, std::min(B, kn.theta_b.v)) : std::min(B, 16);
  pl.theta_lds_main = std::max(theta_lds_bytes(K, pl.theta_docs_main), (kMaxLdsBytes - 24 * 1024) / (kn.theta_wgs.set ? std::max(1, kn.theta_wgs.v) : 5));
  // K > 192 (one-pass streaming z kernel): theta workgroups small enough to sit BESIDE the z waves -- on the LDS the z
  // waves give up -- so that the next theta of a part of the documents is drawn while the following parts are sampled
  // (z_phase).  The padded request caps them at kBeside per CU while z runs.
  pl.cfg_parts = pl.cfg_plain;
  if (scheme == Scheme::ggs) {                        // the parts of the one-pass streaming kernel's z step (pl.kernel == 2)
    pl.parts_forced = kn.zparts.set;
    int parts = kn.zparts.set ? std::max(1, std::min(8, kn.zparts.v)) : pl.kernel == 2 ? 8 : 1;   // measured at K = 1024: 1 part 18.4 ms per sweep, 2: 18.1, 4: 16.5, 8: 15.9
    if (parts > 1 && pl.kernel == 2) {
      const int kBeside = kn.beside.set ? std::max(1, kn.beside.v) : 4;   // measured at K = 1024 (sweep): 2 -> 16.9 ms, 3 -> 16.1, 4 -> 15.0, 5 -> 15.0
      // The z waves and the documents per workgroup are the ones the cells alone allow (as measured, before the cell
      // list came beside the cells).  Where the list takes the request over a granule that the z waves' remainder does not
      // have four times (K = 161-164, 234-256, 513-572, 769-828, 1153-1280), three theta workgroups sit beside the z waves
      // instead of kBeside.  Measured against the other two ways at K = 161 / 256 / 520, ms per sweep (without the list
      // 2.881 / 3.600 / 8.993): this 2.884 / 3.581 / 8.704, a z wave less 2.969 / 3.674 / 8.931, half the documents 4.12 at 256.
      const int z_alloc = lds_alloc_of(pl.z.lds);
      auto z_waves_beside = [&](int theta_lds) { return std::min(pl.z.per_cu, (kMaxLdsBytes - kLdsGranule - kBeside * lds_alloc_of(theta_lds)) / z_alloc); };
      int Bt = 64;
      while (Bt > 1 && theta_cells_lds_bytes(K, Bt) > 10 * 1024) Bt >>= 1;
      const int zw = z_waves_beside(theta_cells_lds_bytes(K, Bt));
      const int t_lds = theta_lds_bytes(K, Bt);
      if (theta_cells_lds_bytes(K, Bt) <= 12 * 1024 && zw >= 2)
        pl.cfg_parts = {parts, zw, Bt, std::max(t_lds, theta_quarter), std::max(t_lds, (kMaxLdsBytes - kLdsGranule - zw * z_alloc) / kBeside / kLdsGranule * kLdsGranule)};
      else
        parts = 1;
    }
    pl.cfg_parts.parts = parts;
    return GGS_OK;
  }

  // ---- the pcgs family: a lane or a wave per document; the alias schemes' table build and their own z kernel
  const bool collapsed = scheme == Scheme::collapsed, polyaurn = scheme == Scheme::polyaurn;
  // the wave-per-document kernel: any K up to 4096, any document length.  Waves per CU (the grid is persistent: exactly what
  // is resident): what the kernel's registers allow (asked of the runtime) and what LDS allows (the runtime's answer
  // ignores the allocation granule)
  if (K <= kPcgsWaveMaxTopics) {
    const int nb = pcgs_wave_blocks(Kp);
    pl.wave.fn = pcgs_wave_kernel_for(nb, collapsed, polyaurn);
    pl.wave.lds = pcgs_wave_lds_bytes(nb);
    pl.wave.per_cu = resident_waves_per_cu(pl.wave.fn, pl.wave.lds);
  }
  pl.wave_forced = kn.pcgs_wave.set ? kn.pcgs_wave.v != 0 : K > (collapsed ? kCollapsedWaveFromTopics : polyaurn ? kPolyaurnWaveFromTopics : kPcgsWaveFromTopics);
  if (pl.wave_forced && !pl.wave.fn) return GGS_ERR_UNSUPPORTED;   // more than 4096 topics
  // the lane-per-document kernel: its waves per CU also size the padded document order, whichever kernel runs
  const bool lane_sliced = K <= kSlicedMaxTopics && !(kn.pcgs_stream.set && kn.pcgs_stream.v != 0);
  pl.lane.lds = lane_sliced ? pcgs_sliced_lds_bytes(K) : pcgs_z_lds_bytes(K);
  if (pl.lane.lds > kMaxLdsBytes && !pl.wave_forced) return GGS_ERR_UNSUPPORTED;
  pl.lane.per_cu = lds_workgroups_per_cu(pl.lane.lds, 8);
  if (!pl.wave_forced) pl.lane.fn = pcgs_lane_kernel_for(K, lane_sliced, collapsed, polyaurn);
  if (collapsed) pl.serial.fn = reinterpret_cast<const void *>(collapsed_serial_kernel);
  if (has_alias(scheme)) {
    pl.alias_wpb = alias_words_per_block(K);
    pl.alias = {reinterpret_cast<const void *>(alias_build_kernel), 64, (int)alias_lds_bytes(K, pl.alias_wpb), 0};
    pl.alias.per_cu = lds_workgroups_per_cu(pl.alias.lds, 16);
  }
  if (doubly_sparse(scheme)) pl.wordlist = {reinterpret_cast<const void *>(word_list_build_kernel), kWordListBlock, 0, 8};   // a wave per word, four to a workgroup
  // the z kernels of the sparse walks and of adlda: their LDS comes with the corpus
  if (scheme == Scheme::spalias) pl.spalias.fn = reinterpret_cast<const void *>(spalias_wave_kernel);
  if (scheme == Scheme::polyaurn_sparse) pl.pusparse.fn = reinterpret_cast<const void *>(polyaurn_sparse_wave_kernel);
  if (scheme == Scheme::nzvsspalias) {                 // the list build from the drawn cells, the chain's kernels (LDS by V, a workgroup per topic) and the z step
    pl.wordmask = {reinterpret_cast<const void *>(word_list_mask_kernel), kWordListBlock, 0, 8};
    pl.vsbits = {reinterpret_cast<const void *>(vs_bits_kernel), 64, 0, 32};
    const bool global = V > kVsLdsMaxV || (kn.vs_global.set && kn.vs_global.v != 0);
    pl.vschain = {global ? reinterpret_cast<const void *>(vs_chain_kernel<true>) : reinterpret_cast<const void *>(vs_chain_kernel<false>), kVsBlock,
                  global ? 0 : (int)vs_chain_lds_bytes((V + 31) / 32), 1};
    pl.nzvs.fn = reinterpret_cast<const void *>(nzvs_wave_kernel);
  }
  if (scheme == Scheme::lightpclda) {
    // as many resident waves as fit: a lone wave issues at a fraction of a SIMD's rate, and the step is a chain of dependent operations
    pl.lightpc = {reinterpret_cast<const void *>(lightpc_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightpc.per_cu = resident_waves_per_cu(pl.lightpc.fn, pl.lightpc.lds);
  }
  if (count_tables(scheme)) {
    // the tables over the counts: alias_build_kernel's words per workgroup and residency; the z step: lightpc's rule
    pl.alias_wpb = alias_words_per_block(K);
    pl.countalias = {reinterpret_cast<const void *>(count_alias_build_kernel), 64, (int)count_alias_lds_bytes(K, pl.alias_wpb), 0};
    pl.countalias.per_cu = lds_workgroups_per_cu(pl.countalias.lds, 16);
  }
  if (scheme == Scheme::lightpcldaw2) {
    pl.lightpcw2 = {reinterpret_cast<const void *>(lightpcw2_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightpcw2.per_cu = resident_waves_per_cu(pl.lightpcw2.fn, pl.lightpcw2.lds);
  }
  if (scheme == Scheme::lightcollapsed) {
    pl.lightcol = {reinterpret_cast<const void *>(lightcollapsed_wave_kernel), 64, (int)light_lds_bytes(K), 0};
    pl.lightcol.per_cu = resident_waves_per_cu(pl.lightcol.fn, pl.lightcol.lds);
  }
  if (scheme == Scheme::adlda) {                       // one wave for the head, a wave per word for the lists; the z kernel's LDS comes with the corpus
    pl.adhead = {reinterpret_cast<const void *>(adlda_head_kernel), 64, 0, 1};
    pl.adlists = {reinterpret_cast<const void *>(word_list_counts_kernel), kWordListBlock, 0, 8};
    pl.adlda.fn = reinterpret_cast<const void *>(adlda_wave_kernel);
  }
  return GGS_OK;
}

const KernelLaunch &pcgs_entry(const LaunchPlan &pl, Scheme s, bool wave) {
  return row_of(s).entry ? pl.*row_of(s).entry : wave ? pl.wave : pl.lane;
}
int launch_pcgs_z(ggs_handle *h) {
  if (h->N == 0) return GGS_OK;
  PcgsParams pp{};
  pp.tok = h->d_tok; pp.inv_perm = h->d_inv_perm; pp.z = h->d_z; pp.zw = h->d_zw; pp.doc_ptr = h->d_doc_ptr; pp.order = h->d_order;
  pp.alpha = h->d_alpha; pp.phiT = h->d_phiT; pp.status = h->d_status;
  pp.num_docs = h->pcgs_order_len; pp.tok_base = h->tok_base; pp.seed = h->seed; pp.iteration = (uint32_t)h->iteration;   // the length of the (padded) order list
  pp.K = h->K; pp.Kp = h->Kp;
  int rc;
  if (h->alias_stale && (rc = launch_alias_build(h))) return rc;   // the schemes with tables over Phi
  if (count_form(h->scheme)) {
    if ((rc = launch_sweep_head(h))) return rc;
    pp.n_wk = h->d_n_wk; pp.n_k = h->d_n_k; pp.beta = h->beta; pp.beta_sum = h->beta * (double)h->V;   // betaSum = beta * numTypes, MSLDA:136
  } else if (count_tables(h->scheme)) {                // lightpcldaw2: Phi as it stands, the lists and tables of the corpus-wide sweep-start counts
    if ((rc = launch_sweep_head(h))) return rc;
    pp.n_wk = h->d_n_wk; pp.n_k = h->d_n_k; pp.beta = h->beta; pp.beta_sum = h->beta * (double)h->V;
  }
  PolyaurnSparseParams sp{};                           // spalias's kernel takes its base, SpaliasParams
  LightCountParams lp{};                               // lightpclda's kernel takes its base, LightpcParams
  AdldaParams ad{};
  void *args[] = {&pp, &h->margin_scale};              // the wave-per-document kernel takes both, the lane-per-document kernels the first
  if (sparse_walk(h->scheme)) {
    // one wave per document over its non-zero topics (ggs_z_spalias.hpp), or over the word's where they are fewer
    // (ggs_z_polyaurn_sparse.hpp: the lists and the counters, null in a spalias handle)
    sp.b = pp; sp.ps = h->d_alias_ps; sp.a = h->d_alias_a; sp.type_norm = h->d_alias_tn; sp.cap = h->sp_cap; sp.margin_scale = h->margin_scale;
    sp.nzw = h->d_nzw; sp.nw = h->d_nw; sp.stats = h->d_ps_stats;
    args[0] = static_cast<SpaliasParams *>(&sp);
  } else if (has_mh(h->scheme)) {
    // one wave per document, two proposals per token (ggs_z_light.hpp): over spalias's tables (lightpclda), or over the lists and
    // tables of the sweep-start counts (lightcollapsed, lightpcldaw2; null in a lightpclda handle)
    lp.b = pp; lp.ps = h->d_alias_ps; lp.a = h->d_alias_a; lp.mh = h->d_mh; lp.alpha_sum = h->alpha_sum;
    lp.nzw = h->d_nzw; lp.nw = h->d_nw; lp.tpt = h->d_tpt;
    args[0] = static_cast<LightpcParams *>(&lp);
  } else if (h->scheme == Scheme::adlda) {             // one wave per document over den0, S0 and the lists of the sweep-start counts
    ad.b = pp; ad.den0 = h->d_ad_den0; ad.s0 = h->d_ad_s0; ad.nzw = h->d_nzw; ad.nw = h->d_nw; ad.stats = h->d_ps_stats; ad.cap = h->sp_cap; ad.margin_scale = h->margin_scale;
    args[0] = &ad;
  }
  HIP_TRY(h, launch(h, h->pcgs_z, h->pcgs_items, args, h->stream));
  return GGS_OK;
}

// `count`: with an exchange the sliced kernels add every token's new (word, topic) cell into the (zeroed) send buffer of the
// count reduce-scatter themselves; the timed comparison of the two z forms launches without it
// ... where few tokens share a cell: the atomics of different XCDs on one line serialise at the memory side.  Measured on the
// benchmark corpus split N ways (z step with / without them, and the count kernel they replace): N = 8 (50 tokens per word
// on the rank) 0.139 / 0.132 ms against 0.040 of count kernel; N = 4 (100) 0.290 / 0.26 against 0.05; N = 2 (200) 0.627 / 0.52
// against 0.07 -- they pay up to about 64 tokens per word (GGS_DEBUG_ZCOUNTS=2 forces them).
bool z_counts_itself(const ggs_handle *h) {
  return h->xg && h->z_counts && h->plan.sliced() && (h->z_counts_forced || h->N <= (int64_t)64 * h->V) && !use_sparse(h);
}
// `defer_join` (with `count`, split form): the hot words' count launch follows the hot kernel on ITS stream and the
// handle's stream is not made to wait for that stream here -- the caller does (join_hot_stream), behind the z step's end
// event, so that the hot chunks' count sits beside the tail of the cold kernel instead of behind it.
int launch_count_hot(ggs_handle *h);
int launch_z(ggs_handle *h, bool force_fused = false, int64_t c0 = 0, int64_t c1 = -1, bool count = false, bool defer_join = false) {
  h->hot_join_pending = false;
  if (h->N == 0) return GGS_OK;
  const LaunchPlan &pl = h->plan;
  ZParams zp{};
  zp.tok = h->d_tok; zp.inv_perm = h->d_inv_perm; zp.z = h->d_z; zp.zw = h->d_zw; zp.chunk_start = h->d_chunk_start; zp.chunk_doc = h->d_chunk_doc; zp.chunk_len = h->d_chunk_len;
  zp.theta = h->d_theta; zp.phiT = h->d_phiT; zp.status = h->d_status;
  zp.tok_base = h->tok_base; zp.seed = h->seed; zp.iteration = (uint32_t)h->iteration;
  zp.K = h->K; zp.Kp = h->Kp; zp.pitch16 = h->pitch16; zp.tile_tokens = pl.tile_tokens;
  zp.margin_scale = h->margin_scale;
  zp.chunk_doc1 = h->d_chunk_doc1; zp.two_rows = (pl.two_rows && h->d_chunk_doc1) ? 1 : 0;
  zp.ct_tok = h->d_ct_tok; zp.ct_idx = h->d_ct_idx; zp.ct_ip = h->d_ct_ip; zp.c_docs = h->d_c_docs; zp.num_cold = h->Cc;
  zp.hot_words = h->d_hot_words; zp.num_hot = h->num_hot; zp.hot_pitch = pl.hot_pitch;
  zp.wave_lds = pl.wave_lds; zp.hot_off = kSlicedWaves * pl.wave_lds; zp.ring_base = pl.ring_base;
  zp.cnt_send = (count && z_counts_itself(h)) ? h->d_cnt_send : nullptr;
  zp.smap = h->smap;
  zp.ht_pack = reinterpret_cast<const int4 *>(h->d_ht_pack); zp.h_docs = h->d_h_docs;
  zp.wt_pack = reinterpret_cast<const int4 *>(h->d_wt_pack); zp.w_docs = h->d_w_docs; zp.warm_words = h->d_warm_words;
  zp.warm_meta = h->d_warm_meta; zp.warm_tiers = h->warm_tiers; zp.warm_rows = pl.warm_cap;
  zp.phiT32 = h->d_phiT32; zp.Kp32 = pl.Kp32; zp.replays = h->d_replays; zp.margin_scale32 = h->margin_scale32;
  void *args[] = {&zp};
  if (!pl.sliced()) {
    // a range of the chunk table (the one-document chunks are in document order); persistent single-wave workgroups stride it
    if (c1 < 0) c1 = h->C;
    if (c1 <= c0) return GGS_OK;
    zp.chunk_start += c0; zp.chunk_doc += c0; zp.chunk_len += c0; zp.num_chunks = c1 - c0;
    if (zp.chunk_doc1) zp.chunk_doc1 += c0;
    KernelLaunch z = pl.z;
    z.per_cu = h->cfg->z_per_cu;
    HIP_TRY(h, launch(h, z, zp.num_chunks, args, h->stream));
    return GGS_OK;
  }
  // one 4-wave workgroup per CU (a wave per SIMD), persistent; the hot-word table fills the LDS the rings leave
  zp.num_chunks = h->Cs;
  const int hot_rows_lds = h->num_hot * pl.hot_pitch;
  // the warm tiers (z_warm_kernel): behind the hot chunks on their stream, or behind the one kernel of the fused form
  ZParams wp = zp;
  wp.wave_lds = pl.warm_wave_lds; wp.hot_off = kSlicedWaves * pl.warm_wave_lds;
  void *wargs[] = {&wp};
  auto launch_warm = [&](hipStream_t st) { return h->Cw == 0 ? hipSuccess : launch(h, pl.warm, h->warm_chunks_max, wargs, st, h->warm_rows_max * pl.hot_pitch); };
  if (h->z_split && !force_fused && h->Cs > h->Cc && h->Cc > 0) {
    // cold chunks on the main stream, hot chunks beside them (z_hot_kernel): two waves per SIMD
    ZParams hp = zp;
    hp.wave_lds = pl.hot_wave_lds; hp.hot_off = kSlicedWaves * pl.hot_wave_lds;
    void *hargs[] = {&hp};
    if (h->hot_fork_from) {
      HIP_TRY(h, hipStreamWaitEvent(h->side_hot, h->hot_fork_from, 0));
    } else {
      HIP_TRY(h, hipEventRecord(h->ev_hot_fork, h->stream));
      HIP_TRY(h, hipStreamWaitEvent(h->side_hot, h->ev_hot_fork, 0));
    }
    zp.num_chunks = h->Cc; zp.num_hot = 0;
    HIP_TRY(h, launch(h, pl.cold, h->Cc, args, h->stream));
    HIP_TRY(h, launch(h, pl.hot, h->Cs - h->Cc, hargs, h->side_hot, hot_rows_lds));
    HIP_TRY(h, launch_warm(h->side_hot));
    if (defer_join && zp.cnt_send) {
      hipStream_t main_stream = h->stream;
      h->stream = h->side_hot;
      const int rc = launch_count_hot(h);
      h->stream = main_stream;
      if (rc) return rc;
      h->hot_counted = true;
    }
    HIP_TRY(h, hipEventRecord(h->ev_hot_join, h->side_hot));
    if (defer_join) h->hot_join_pending = true;
    else HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_hot_join, 0));
  } else {
    HIP_TRY(h, launch(h, pl.cold, std::max(h->Cc, h->Cs - h->Cc), args, h->stream, hot_rows_lds));
    HIP_TRY(h, launch_warm(h->stream));
  }
  if (pl.f32) ++h->z_f32_launches;
  return GGS_OK;
}

bool sample_phi_this_iteration(const ggs_handle *h) {  // UPLDA:1350-1352
  return h->phi_burn_in > 0 && h->iteration > h->phi_burn_in && (h->iteration % h->phi_thin) == 0;
}

// java.util.Random(seed).nextInt(bound), n times (JDK 8 javadoc algorithm: 48-bit LCG,
// next(31), power-of-two shortcut, modulo rejection loop otherwise).
uint64_t java_lcg_next_ints(int32_t seed, int32_t bound, int64_t n, int32_t *out) {   // returns the generator's state after the n draws
  constexpr uint64_t kMult = 0x5DEECE66DULL, kMask = (1ULL << 48) - 1;
  uint64_t s = ((uint64_t)(int64_t)seed ^ kMult) & kMask;
  auto next31 = [&]() { s = (s * kMult + 0xBULL) & kMask; return (int32_t)(s >> 17); };
  const int32_t m = bound - 1;
  for (int64_t i = 0; i < n; ++i) {
    int32_t r = next31();
    if ((bound & m) == 0) r = (int32_t)(((int64_t)bound * (int64_t)r) >> 31);
    else
      for (int32_t u = r;; u = next31()) {
        r = u % bound;
        if ((int32_t)((uint32_t)u - (uint32_t)r + (uint32_t)m) >= 0) break;
      }
    out[i] = r;
  }
  return s;
}

int require_ready(ggs_handle *h, bool need_phi) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!h->have_corpus) return set_err(h, GGS_ERR_STATE, "no corpus: call ggs_set_corpus first");
  if (need_phi && !h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  return bind_device(h);
}

// The side-stream theta must not outlive the z it was drawn from.
int drop_theta_ahead(ggs_handle *h) {
  if (h->side) HIP_TRY(h, hipStreamSynchronize(h->side));
  h->theta_ahead_iter = INT64_MIN;
  return GGS_OK;
}

// waits for every enqueued sweep and adds its phase times to the timings
int settle_sweeps(ggs_handle *h) {
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int j = h->ev_pending - 1; j >= 0; --j) {
    const Events &E = h->evs[((h->ev_head - j) % kEvRing + kEvRing) % kEvRing];
    float ms = 0;
    // a consumed ahead-draw: the stream waited on th1 before the z kernel, so both side-stream events are complete;
    // their span is the duration of a kernel that ran beside the previous sweep's Phi phase
    // (every event or barrier packet on the critical stream costs ~6 us of device time: a theta drawn on it starts at the
    // previous sweep's e[2])
    if (E.used_ahead && E.theta_on_main) { HIP_TRY(h, hipEventElapsedTime(&ms, h->evs[((h->ev_head - j - 1) % kEvRing + kEvRing) % kEvRing].e[2], E.th1)); }
    else if (E.used_ahead) { HIP_TRY(h, hipEventElapsedTime(&ms, E.th0, E.th1)); }
    else { HIP_TRY(h, hipEventElapsedTime(&ms, E.e[0], E.e[1])); }
    h->tm.theta_ms += ms;
    HIP_TRY(h, hipEventElapsedTime(&ms, E.e[1], E.e[2])); h->tm.z_ms += ms;
    if (E.light) {                                       // the ends only: the phases in the last fully timed sweep's proportions
      HIP_TRY(h, hipEventElapsedTime(&ms, E.e[2], E.e[5]));
      h->tm.merge_ms += ms * h->frac[0];
      h->tm.exchange_rs_ms += ms * h->frac[1]; h->tm.exchange_ag_ms += ms * h->frac[3]; h->tm.exchange_ms += ms * (h->frac[1] + h->frac[3]);
      h->tm.phi_ms += ms * (h->frac[2] + h->frac[4]);
      h->tm.sweeps += 1;
      h->tm.tokens_sampled += h->N;
      continue;
    }
    HIP_TRY(h, hipEventElapsedTime(&ms, E.e[2], E.e[3])); h->tm.merge_ms += ms;
    if (E.exchanged) {
      float span = 0, part[5] = {ms, 0, 0, 0, 0};
      (void)hipEventElapsedTime(&span, E.e[2], E.e[5]);
      (void)hipEventElapsedTime(&part[1], E.e[E.e4_is_e3 ? 3 : 4], E.x[0]); (void)hipEventElapsedTime(&part[2], E.x[0], E.x[1]);
      (void)hipEventElapsedTime(&part[3], E.x[1], E.x[2]); (void)hipEventElapsedTime(&part[4], E.x[2], E.e[5]);
      if (span > 0) {
        // what lies between e[3] and e[4] in a split sweep (the caller's own work) is nobody's phase: renormalise
        const float sum = part[0] + part[1] + part[2] + part[3] + part[4];
        for (int q = 0; q < 5; ++q) h->frac[q] = sum > 0 ? part[q] / sum : 0.0;
        h->have_frac = true;
      }   // reduce-scatter | slice draw (the first half's all-gather beneath it) | what is left of the all-gathers | repack
      HIP_TRY(h, hipEventElapsedTime(&ms, E.e[E.e4_is_e3 ? 3 : 4], E.x[0])); h->tm.exchange_ms += ms; h->tm.exchange_rs_ms += ms;
      HIP_TRY(h, hipEventElapsedTime(&ms, E.x[0], E.x[1])); h->tm.phi_ms += ms;
      HIP_TRY(h, hipEventElapsedTime(&ms, E.x[1], E.x[2])); h->tm.exchange_ms += ms; h->tm.exchange_ag_ms += ms;
      HIP_TRY(h, hipEventElapsedTime(&ms, E.x[2], E.e[5])); h->tm.phi_ms += ms;
    } else {
      HIP_TRY(h, hipEventElapsedTime(&ms, E.e[E.e4_is_e3 ? 3 : 4], E.e[5])); h->tm.phi_ms += ms;
    }
    h->tm.sweeps += 1;
    h->tm.tokens_sampled += h->N;
  }
  h->ev_pending = 0;
  return GGS_OK;
}

// the handle's launches go to another stream for a scope (the count rebuild and the Phi chain of a whole sweep)
struct StreamSwap {
  ggs_handle *h;
  hipStream_t user;
  StreamSwap(ggs_handle *h_, hipStream_t s) : h(h_), user(h_->stream) { h->stream = s; }
  ~StreamSwap() { h->stream = user; }
};

int z_phase(ggs_handle *h) {
  int rc;
  if (h->ev_pending >= kEvRing - 2 && (rc = settle_sweeps(h))) return rc;   // keep this slot and the next one free
  h->ev_head = (h->ev_head + 1) % kEvRing;
  Events &E = h->evs[h->ev_head];
  E.light = h->xg && h->have_frac && h->detail_every > 1 && !h->force_detail && (h->sweeps_enqueued % h->detail_every) != 0 && !count_form(h->scheme);
  h->sweeps_enqueued += 1;
  if (pcgs_family(h->scheme)) {                         // no theta: it is integrated out (UPLDA:1509-1513)
    E.used_ahead = false;
    HIP_TRY(h, hipEventRecord(E.e[0], h->stream));
    HIP_TRY(h, hipEventRecord(E.e[1], h->stream));
    if ((rc = launch_pcgs_z(h))) return rc;
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));
    if ((rc = launch_count_rebuild(h))) return rc;
    if (!E.light) HIP_TRY(h, hipEventRecord(E.e[3], h->stream));
    return GGS_OK;
  }
  E.used_ahead = h->theta_ahead_iter == (int64_t)h->iteration;
  h->hot_fork_from = nullptr;
  if (E.used_ahead) {
    if (E.theta_on_main) h->hot_fork_from = E.th1;          // drawn on this very stream: nothing to wait for, and the hot kernel's stream (which ran the Phi chain) forks from th1
    else HIP_TRY(h, hipStreamWaitEvent(h->stream, E.th1, 0));   // drawn during the previous iteration's Phi phase
    std::swap(h->d_theta, h->d_theta_next);
  } else {
    E.theta_on_main = false;
    if (h->side) HIP_TRY(h, hipStreamSynchronize(h->side));
    HIP_TRY(h, hipEventRecord(E.e[0], h->stream));
    if ((rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  HIP_TRY(h, hipEventRecord(E.e[1], h->stream));
  if (h->plan.sliced() && h->z_split && !h->z_split_tried && h->Cs > h->Cc && h->Cc > 0) {
    // Whether the guest kernel really runs beside the cold one depends on how the runtime maps streams to hardware
    // queues (measured: beside each other in a plain process, one after the other under torchrun + RCCL).  Both forms
    // write the same z, so the first z step of a corpus simply runs twice, timed, and the slower form is dropped.
    h->z_split_tried = true;
    float t_split = 0, t_fused = 0;
    hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
    if (hipEventCreate(&t0) != hipSuccess || hipEventCreate(&t1) != hipSuccess || hipEventCreate(&t2) != hipSuccess) return set_err(h, GGS_ERR_HIP, "hipEventCreate");
    if ((rc = launch_z(h, false)) || (rc = launch_z(h, true))) return rc;   // untimed: code upload, cold caches
    HIP_TRY(h, hipEventRecord(t0, h->stream));
    if ((rc = launch_z(h, false))) return rc;
    HIP_TRY(h, hipEventRecord(t1, h->stream));
    if ((rc = launch_z(h, true))) return rc;
    HIP_TRY(h, hipEventRecord(t2, h->stream));
    HIP_TRY(h, hipEventSynchronize(t2));
    HIP_TRY(h, hipEventElapsedTime(&t_split, t0, t1));
    HIP_TRY(h, hipEventElapsedTime(&t_fused, t1, t2));
    (void)hipEventDestroy(t0); (void)hipEventDestroy(t1); (void)hipEventDestroy(t2);
    if (t_fused < t_split) h->z_split = false;
    HIP_TRY(h, hipEventRecord(E.e[1], h->stream));          // this sweep's z time: one launch of the form kept
  }
  if (!h->hot_fork_from) h->hot_fork_from = E.e[1];        // the event just recorded serves as the hot chunks' fork: one packet less
  h->theta_ahead_iter = INT64_MIN;
  const bool ahead = h->overlap_theta && h->side && h->D > 0 && h->iteration < INT32_MAX;   // there is no iteration behind the last
  const int32_t P = (int32_t)h->part_doc.size() - 1;   // 1 for a small corpus
  if (ahead && P > 1 && h->plan.stream()) {
    // part by part: z of part p on the main stream, then -- beside z of part p + 1 -- theta of iteration t+1 for the
    // documents of part p on the side stream; the last part's theta runs beside the counts and the Phi draw
    Events &N = h->evs[(h->ev_head + 1) % kEvRing];
    for (int32_t p = 0; p < P; ++p) {
      if ((rc = launch_z(h, false, h->part_chunk[(size_t)p], h->part_chunk[(size_t)p + 1]))) return rc;
      HIP_TRY(h, hipEventRecord(h->ev_part[p], h->stream));
      HIP_TRY(h, hipStreamWaitEvent(h->side, h->ev_part[p], 0));
      if (p == 0) { N.theta_on_main = false; HIP_TRY(h, hipEventRecord(N.th0, h->side)); }
      if ((rc = launch_theta(h, h->side, h->d_theta_next, h->iteration + 1, h->part_doc[(size_t)p], h->part_doc[(size_t)p + 1],
                             p + 1 < P ? h->cfg->theta_lds_beside_z : 0)))
        return rc;
    }
    HIP_TRY(h, hipEventRecord(N.th1, h->side));
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));
    h->theta_ahead_iter = (int64_t)h->iteration + 1;
  } else {
    const bool counting = z_counts_itself(h) && h->Cs > 0;
    if (counting && !h->cnt_send_zeroed && (rc = clear_send_buffer(h, h->stream))) return rc;   // nobody cleared it behind the last reduce-scatter (or none came): counts no z step asked for are overwritten, as a count rebuild overwrites them
    h->hot_counted = false;
    if ((rc = launch_z(h, false, 0, -1, counting, /*defer_join=*/counting))) return rc;
    if (counting) { h->z_counted = true; h->cnt_send_zeroed = false; h->counted_sparse = false; }
    HIP_TRY(h, hipEventRecord(E.e[2], h->stream));      // the cold kernel's end; the hot chunks' stream is joined below, and by the theta draw's stream
    h->chain_on_side = h->chain_on_side && ahead;
    if (ahead) {
      // theta of iteration t+1 from the z just drawn, concurrent with the counts and the Phi draw
      Events &N = h->evs[(h->ev_head + 1) % kEvRing];
      hipStream_t ts = h->chain_on_side ? h->stream : h->side;
      HIP_TRY(h, hipStreamWaitEvent(h->chain_on_side ? h->side_hot : h->side, E.e[2], 0));
      if (h->hot_join_pending) HIP_TRY(h, hipStreamWaitEvent(ts, h->ev_hot_join, 0));   // the theta draw reads the hot chunks' z as well
      N.theta_on_main = h->chain_on_side;
      if (!h->chain_on_side) HIP_TRY(h, hipEventRecord(N.th0, ts));
      if ((rc = launch_theta(h, ts, h->d_theta_next, h->iteration + 1, 0, -1, h->chain_on_side ? h->plan.theta_lds_main : 0, h->chain_on_side ? h->plan.theta_docs_main : 0))) return rc;
      HIP_TRY(h, hipEventRecord(N.th1, ts));
      h->theta_ahead_iter = (int64_t)h->iteration + 1;
    }
  }
  {
    StreamSwap on_chain(h, h->chain_on_side ? h->side_hot : h->stream);
    if (h->hot_join_pending) { HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_hot_join, 0)); h->hot_join_pending = false; }
    if (h->z_counted) {                              // the z kernels added the cold tokens' cells: the hot words' segments are left
      h->z_counted = false;
      if (h->hot_counted) { h->n_k_valid = false; h->counts_global = false; h->cnt_own_valid = false; }   // ... and were counted on the hot chunks' stream
      else if ((rc = launch_count_hot(h))) return rc;
    } else if ((rc = launch_count_rebuild(h))) return rc;   // this shard's counts; summed across shards by the caller
    if (!E.light) HIP_TRY(h, hipEventRecord(E.e[3], h->stream));
    if (h->chain_on_side && !h->whole_sweep) HIP_TRY(h, hipEventRecord(h->ev_chain_done, h->stream));
  }
  // ggs_sweep_begin on its own: what the caller does on the handle's stream before ggs_sweep_end (a getter) sees the counts
  if (h->chain_on_side && !h->whole_sweep) HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_chain_done, 0));
  return GGS_OK;
}

// `settle` = wait for the device, raise what the sweeps flagged and add their phase times to the timings.  A batch
// (ggs_sweep with n_sweeps > 1) settles once, after its last sweep: the device flags are sticky, and the ~40 us host
// round trip per sweep is 2 % of a 1.9 ms sweep.
int finish_sweep_enqueue_on(ggs_handle *h, bool with_phi);
int finish_sweep_enqueue(ggs_handle *h, bool with_phi) {
  if (!h->chain_on_side) return finish_sweep_enqueue_on(h, with_phi);
  int rc;
  {
    StreamSwap on_chain(h, h->side_hot);
    if ((rc = finish_sweep_enqueue_on(h, with_phi))) return rc;
    HIP_TRY(h, hipEventRecord(h->ev_chain_done, h->stream));
  }
  HIP_TRY(h, hipStreamWaitEvent(h->stream, h->ev_chain_done, 0));   // behind the theta draw: the next z step, a getter, a synchronise see both legs
  return GGS_OK;
}
int finish_sweep_enqueue_on(ggs_handle *h, bool with_phi) {
  int rc;
  Events &E = h->evs[h->ev_head];
  E.e4_is_e3 = h->whole_sweep;                         // one event packet less on the stream (~6 us each)
  if (!E.e4_is_e3 && !E.light) HIP_TRY(h, hipEventRecord(E.e[4], h->stream));
  bool acc = false;
  E.exchanged = false;
  if (with_phi) {
    acc = (h->flags & GGS_FLAG_SAVE_PHI_MEAN) && sample_phi_this_iteration(h);
    if (count_form(h->scheme)) {   // no Phi in the count form: the merge (with an exchange: the gather of the count slices) and tokensPerTopic
      acc = false;
      if ((rc = launch_magnitude(h))) return rc;
    } else {
      E.exchanged = h->xg != nullptr;
      if ((rc = launch_phi(h, false, acc, E.light ? nullptr : &E))) return rc;
    }
  }
  HIP_TRY(h, hipEventRecord(E.e[5], h->stream));
  if (acc) h->n_sampled_phi++;             // GGS:168-170
  h->ev_pending += 1;
  return GGS_OK;
}
int finish_sweep_settle(ggs_handle *h) {
  int rc;
  if ((rc = check_status(h))) return rc;   // synchronises the stream
  if ((rc = settle_sweeps(h))) return rc;
  if (h->flags & GGS_FLAG_PARANOID) return ggs_check_invariants(h);
  return GGS_OK;
}
int finish_sweep(ggs_handle *h, bool with_phi, bool settle = true) {
  int rc = finish_sweep_enqueue(h, with_phi);
  if (rc) return rc;
  if (!settle && !(h->flags & GGS_FLAG_PARANOID)) return GGS_OK;
  return finish_sweep_settle(h);
}

// An Exchange that never got attached: its communicator goes with it when the library created it.
void exchange_free(Exchange *x) {
  if (!x) return;
  if (x->own_comm && x->comm && x->api) (void)x->api->CommDestroy(x->comm);
  delete x;
}
// what every attach call checks BEFORE it creates anything (ncclCommInitRank is a blocking collective)
int exchange_precheck(ggs_handle *h, int32_t rank, int32_t nranks) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (h->xg) return set_err(h, GGS_ERR_STATE, "an exchange is already attached");
  if (h->have_corpus) return set_err(h, GGS_ERR_STATE, "attach the exchange before ggs_set_corpus");
  if (nranks < 1 || rank < 0 || rank >= nranks) return set_err(h, GGS_ERR_BAD_ARG, "rank outside [0, nranks)");
  return bind_device(h);
}

// Buffers and the column map of an attached exchange; the handle moves to a stream of its own.  Takes ownership of x.
int setup_exchange(ggs_handle *h, Exchange *x) {
  int rc = exchange_precheck(h, x->rank, x->nranks);
  if (rc) { exchange_free(x); return rc; }
  const std::vector<int32_t> sl = topic_slices(h->K, x->nranks);
  h->xg = x;
  h->k0 = sl[(size_t)x->rank]; h->Ks = sl[(size_t)x->rank + 1] - h->k0; h->Ksm = (h->K + x->nranks - 1) / x->nranks;
  {
    auto magic = [](uint32_t d) { return d > 1 ? (uint32_t)((0x100000000ull + d - 1) / d) : 0u; };   // udiv_magic (ggs_kernels.hpp)
    h->smap.size = h->K / x->nranks; h->smap.rem = h->K % x->nranks; h->smap.ksm = h->Ksm;
    h->smap.m_size = magic((uint32_t)std::max(h->smap.size, 1)); h->smap.m_size1 = magic((uint32_t)h->smap.size + 1);
    h->smap.rank_stride = (int64_t)h->V * h->Ksm;
    if (const char *e = debug_env("GGS_DEBUG_ZCOUNTS")) { h->z_counts = std::atoi(e) != 0; h->z_counts_forced = std::atoi(e) == 2; }
    if (const char *e = debug_env("GGS_DEBUG_TIMING_EVERY")) h->detail_every = std::max(1, std::atoi(e));
    if (const char *e = debug_env("GGS_DEBUG_COUNT_EXCHANGE")) h->count_mode = std::max(0, std::min(2, std::atoi(e)));
  }
  std::vector<int64_t> koff((size_t)h->K);
  for (int32_t r = 0; r < x->nranks; ++r)
    for (int32_t k = sl[(size_t)r]; k < sl[(size_t)r + 1]; ++k) koff[(size_t)k] = (int64_t)r * h->V * h->Ksm + (k - sl[(size_t)r]);
  std::vector<int32_t> krank((size_t)h->K), kcol((size_t)h->K);
  for (int32_t r = 0; r < x->nranks; ++r)
    for (int32_t k = sl[(size_t)r]; k < sl[(size_t)r + 1]; ++k) { krank[(size_t)k] = r; kcol[(size_t)k] = k - sl[(size_t)r]; }
  // the all-gather of the gammas in two halves of the vocabulary (whole 64-row segments: the draw's tiles); a short
  // vocabulary goes in one
  h->seg_split = h->sum_nseg >= 16 ? h->sum_nseg / 2 : 0;
  if (const char *e = debug_env("GGS_DEBUG_AGSPLIT")) h->seg_split = std::max(0, std::min(h->sum_nseg - 1, std::atoi(e)));
  h->v_split = h->seg_split * kSumSegRows;
  const size_t slice = (size_t)h->V * h->Ksm, all = slice * (size_t)x->nranks;
  auto fail = [&](int code) {                        // a half-built exchange must not stay attached
    void *bufs[] = {h->d_koff, h->d_krank, h->d_kcol, h->d_cnt_send, h->d_cnt_own, h->d_phi_own, h->d_phi_all0, h->d_phi_all1, h->d_mag_own, h->d_n_k_own};
    for (void *b : bufs) if (b) (void)hipFree(b);
    h->d_koff = nullptr; h->d_krank = h->d_kcol = nullptr; h->d_cnt_send = h->d_cnt_own = nullptr; h->d_phi_own = h->d_phi_all0 = h->d_phi_all1 = nullptr;
    h->d_mag_own = nullptr; h->d_n_k_own = nullptr;
    h->xg = nullptr; h->Ks = h->Ksm = h->K; h->k0 = 0;
    exchange_free(x);
    return code;
  };
  if ((rc = dev_alloc(h, &h->d_koff, (size_t)h->K)) || (rc = dev_alloc(h, &h->d_krank, (size_t)h->K)) || (rc = dev_alloc(h, &h->d_kcol, (size_t)h->K)) ||
      (rc = dev_alloc(h, &h->d_cnt_send, all)) || (rc = dev_alloc(h, &h->d_cnt_own, slice)) || (rc = dev_alloc(h, &h->d_phi_own, slice + (size_t)h->Ksm)) ||
      (rc = dev_alloc(h, &h->d_phi_all0, half0_elems(h) * (size_t)x->nranks)) || (rc = dev_alloc(h, &h->d_phi_all1, half1_elems(h) * (size_t)x->nranks)) ||
      (rc = dev_alloc(h, &h->d_mag_own, (size_t)h->Ksm)) || (rc = dev_alloc(h, &h->d_n_k_own, (size_t)h->Ksm)))
    return fail(rc);
  if (hipMemcpy(h->d_koff, koff.data(), sizeof(int64_t) * koff.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_krank, krank.data(), sizeof(int32_t) * krank.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(h->d_kcol, kcol.data(), sizeof(int32_t) * kcol.size(), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(h->d_cnt_send, 0, all * sizeof(int32_t)) != hipSuccess || hipMemset(h->d_cnt_own, 0, slice * sizeof(int32_t)) != hipSuccess ||
      hipMemset(h->d_phi_own, 0, (slice + (size_t)h->Ksm) * sizeof(double)) != hipSuccess ||
      hipMemset(h->d_phi_all0, 0, std::max<size_t>(half0_elems(h) * (size_t)x->nranks, 1) * sizeof(double)) != hipSuccess ||
      hipMemset(h->d_phi_all1, 0, half1_elems(h) * (size_t)x->nranks * sizeof(double)) != hipSuccess)
    return fail(set_err(h, GGS_ERR_HIP, "exchange buffers: copy / memset failed"));
  {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(&h->comm_stream, hipStreamNonBlocking, hi) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_half_drawn, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_half_gathered, hipEventDisableTiming) != hipSuccess)
      return fail(set_err(h, GGS_ERR_HIP, "exchange: communication stream / events"));
  }
  if (!h->stream) {
    // Collectives are ordered by THIS stream alone: not the legacy default stream, whose implicit synchronisation with
    // other libraries' blocking streams is exactly the convention not to rely on.  HIGH priority: measured with RCCL
    // and a torch process group in the process, a normal-priority stream shares its hardware queue with theirs and the
    // sweep's phases stretch (one rank: 2.59 ms per sweep against 1.93 on a high-priority stream or the null stream).
    if (!(debug_env("GGS_DEBUG_OWN_STREAM") && std::atoi(debug_env("GGS_DEBUG_OWN_STREAM")) == 0)) {   // 0: experiments
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
      HIP_TRY(h, hipStreamCreateWithPriority(&h->own_stream, hipStreamNonBlocking, hi));
      h->stream = h->own_stream;
    }
  }
  HIP_TRY(h, hipDeviceSynchronize());
  h->counts_global = false; h->cnt_own_valid = false; h->n_k_valid = false;
  h->cnt_send_zeroed = true;                           // the memset above
  return GGS_OK;
}

Exchange *new_rccl_exchange(ggs_handle *h, int32_t rank, int32_t nranks, int *rc) {
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) { *rc = set_err(h, GGS_ERR_UNSUPPORTED, err); return nullptr; }
  auto *x = new (std::nothrow) Exchange();
  if (!x) { *rc = GGS_ERR_HIP; return nullptr; }
  x->rank = rank; x->nranks = nranks; x->api = api;
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops); x->ops.ctx = x;
  x->ops.reduce_scatter_i32 = xops::rccl_reduce_scatter_i32;
  x->ops.all_gather_f64 = xops::rccl_all_gather_f64;
  x->ops.all_gather_i32 = xops::rccl_all_gather_i32;
  x->ops.all_to_all_v_i32 = (api->Send && api->Recv) ? xops::rccl_all_to_all_v_i32 : nullptr;
  *rc = GGS_OK;
  return x;
}

// a collective step for every handle of the group: inside ncclGroupStart/End for RCCL; an adopted group (the caller's
// transport) simply gets the calls one after the other, rank 0 first
template <typename Step>
int group_collective(ggs_handle **hs, int32_t n, Step step) {
  RcclApi *api = hs[0]->xg->api;
  int r = GGS_OK;
  if (api) api->GroupStart();
  for (int32_t i = 0; i < n && !r; ++i)
    if (!(r = bind_device(hs[i]))) r = step(hs[i]);
  if (api && api->GroupEnd() != ncclSuccess && !r) r = set_err(hs[0], GGS_ERR_HIP, "ncclGroupEnd failed");
  return r;
}

// The scheme a configuration asks for (`poisson_L`: polyaurn's alias_poisson_threshold), or what is wrong with the request:
// answered before any device is asked for.
int scheme_of(const ggs_config *cfg, Scheme &scheme, int32_t &poisson_L) {
  const int32_t f = cfg->flags;
  scheme = Scheme::ggs;
  for (int i = 0; i < kNumSchemes; ++i) {              // the rows stand in the order of their bits: the highest bit set names the scheme
    if (!(f & kSchemes[i].flag)) continue;
    if (f & kSchemes[i].refused) return GGS_ERR_BAD_ARG;
    scheme = (Scheme)i;
  }
  poisson_L = cfg->alias_poisson_threshold == 0 ? 100 : cfg->alias_poisson_threshold;   // LDAConfiguration.java:44
  if (poisson_phi(scheme) && ((f & GGS_FLAG_COLLAPSED) || poisson_L < 1 || poisson_L > kPoissonMaxThreshold)) return GGS_ERR_BAD_ARG;
  if (wave_only(scheme) && cfg->num_topics > kPcgsWaveMaxTopics) return GGS_ERR_UNSUPPORTED;
  return GGS_OK;
}

}  // namespace

extern "C" {

int ggs_abi_version(void) { return GGS_ABI_VERSION; }

const char *ggs_last_error(const ggs_handle *h) { return h ? h->err.c_str() : "null handle"; }

int ggs_create(const ggs_config *cfg, ggs_handle **out) {
  if (!cfg || !out) return GGS_ERR_BAD_ARG;
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(ggs_config)) return GGS_ERR_BAD_ARG;
  if (cfg->num_topics <= 0 || cfg->num_types <= 0 || !(cfg->beta > 0)) return GGS_ERR_BAD_ARG;
  Scheme scheme = Scheme::ggs; int32_t poisson_L = 0;
  if (const int rc = scheme_of(cfg, scheme, poisson_L)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device_id < 0 || cfg->device_id >= ndev) return GGS_ERR_HIP;
  ggs_handle *h = new (std::nothrow) ggs_handle();
  if (!h) return GGS_ERR_HIP;
  const Knobs kn;                                      // every GGS_DEBUG_* variable this call reads
  // 1. the model
  h->K = cfg->num_topics; h->V = cfg->num_types; h->device = cfg->device_id;
  h->Ks = h->Ksm = h->K; h->k0 = 0;
  h->Kp = (h->K + 1) & ~1;
  h->pitch16 = (h->Kp / 2) | 1;             // odd number of 16-byte units per LDS row
  h->beta = cfg->beta; h->seed = cfg->seed; h->flags = cfg->flags;
  h->scheme = scheme; h->pa_L = poisson_L;
  h->phi_burn_in = cfg->phi_burn_in; h->phi_thin = cfg->phi_mean_thin > 0 ? cfg->phi_mean_thin : 1;
  h->alpha.assign(h->K, cfg->alpha_scalar);
  if (cfg->alpha) std::copy(cfg->alpha, cfg->alpha + h->K, h->alpha.begin());
  for (double a : h->alpha)
    if (!(a > 0)) { delete h; return GGS_ERR_BAD_ARG; }
  for (double a : h->alpha) h->alpha_sum = h->alpha_sum + a;
  h->alpha_symmetric = std::all_of(h->alpha.begin(), h->alpha.end(), [&](double a) { return std::memcmp(&a, &h->alpha[0], sizeof a) == 0; });
  // 2. the handle's own switches
  // GGS_DEBUG_MARGIN: above 1 the margins force the exact replays in tests.  Below 1 voids the proof, so only the float32 cold
  // kernel takes it (its decided draw is a count of partial sums, always a topic < K); the checkpoint-and-refine walks of the
  // fp64 margin kernels keep >= 1, where a wrong slice could walk them out of it
  if (kn.margin.set) { h->margin_scale = std::max(1.0, kn.margin.f); h->margin_scale32 = std::max(0.0, kn.margin.f); }
  if (kn.chain.set) h->exact_sum = kn.chain.v == 0;
  if (kn.guided.set) h->sum_guided = kn.guided.v != 0;
  if (kn.no_overlap.set) h->overlap_theta = kn.no_overlap.v == 0;
  if (kn.theta_main.set) { h->theta_main = kn.theta_main.v != 0; h->theta_main_always = kn.theta_main.v == 2; }
  if (kn.gamma_queue.set) h->gamma_queue_cap = std::max(0, kn.gamma_queue.v);
  h->sum_nseg = (h->V + kSumSegRows - 1) / kSumSegRows;

  int rc = GGS_OK;
  auto bail = [&](int code) { ggs_destroy(h); return code; };
  // 3. the device and the launches this handle can make on it
  if (hipSetDevice(h->device) != hipSuccess) return bail(GGS_ERR_HIP);
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) != hipSuccess) return bail(GGS_ERR_HIP);
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // GGS_DEBUG_NUM_CUS: a smaller count for every persistent grid and list sized by it (it can only lower the count, and a
    // smaller grid is always resident; no kernel waits on another workgroup).  Results do not depend on it: the tests give
    // one CU many items per workgroup, which the real chip gets only from a large corpus
    if (kn.num_cus.set) h->num_cus = std::max(1, std::min(h->num_cus, kn.num_cus.v));
  }
  if ((rc = plan_launches(h->K, h->V, h->scheme, kn, h->plan))) return bail(rc);
  h->cfg = &h->plan.cfg_parts;
  h->z_split = h->plan.split;
  if (pcgs_family(h->scheme)) h->pcgs_z = pcgs_entry(h->plan, h->scheme, h->plan.wave_forced);
  // The attribute is process-global per kernel, not per handle: always the hardware maximum, so that a later handle
  // with a smaller K never lowers the cap under a live one.
  for (const KernelLaunch *l : h->plan.all())
    if (l->fn && hipFuncSetAttribute(l->fn, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return bail(GGS_ERR_HIP);
  // the document kernels of the two diagnostics: four K-long histograms per block pass 64 KiB from K = 4095
  for (const void *f : {reinterpret_cast<const void *>(ll_docs_kernel), reinterpret_cast<const void *>(lp_docs_kernel)})
    if (hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return bail(GGS_ERR_HIP);
  // 4. the model's buffers
  // (a lightcollapsed or adlda handle has no Phi: ggs_get_phi allocates the buffer of its point estimate when it is first asked for one)
  const bool with_phi = !counts_only(h->scheme);
  const size_t kv = (size_t)h->K * h->V, phi_elems = (size_t)h->V * h->Kp + kPhiTailPadBytes / 8;
  if ((rc = upload(h, &h->d_alpha, h->alpha)) || (with_phi && (rc = dev_alloc_zeroed(h, &h->d_phiT, phi_elems))) ||
      (rc = dev_alloc(h, &h->d_mag, h->K)) || (rc = dev_alloc(h, &h->d_tot, h->K)) || (rc = dev_alloc_zeroed(h, &h->d_n_wk, kv)) ||
      (rc = dev_alloc_zeroed(h, &h->d_n_k, h->K)) || (rc = dev_alloc_zeroed(h, &h->d_status, 4)))
    return bail(rc);
  if ((h->flags & GGS_FLAG_SAVE_PHI_MEAN) && (rc = dev_alloc_zeroed(h, &h->d_phi_mean, kv))) return bail(rc);
  if (h->plan.sliced() && h->plan.f32) {
    if ((rc = dev_alloc_zeroed(h, &h->d_phiT32, (size_t)h->V * h->plan.Kp32 + kPhiTailPadBytes / 4))) return bail(rc);
    if (kn.replays.is(1) && (rc = dev_alloc_zeroed(h, &h->d_replays, 1))) return bail(rc);
  }
  if (h->exact_sum && ((rc = dev_alloc(h, &h->d_sum_pref, ((size_t)h->sum_nseg + 1) * h->K)) ||
                       (rc = dev_alloc(h, &h->d_sum_fn, (size_t)h->sum_nseg * h->K * 4))))
    return bail(rc);
  // tables, lists and counters start zeroed: no entry is ever read that the build (adlda: the head) did not write
  if (has_tables(h->scheme) && ((rc = dev_alloc_zeroed(h, &h->d_alias_ps, kv)) || (rc = dev_alloc_zeroed(h, &h->d_alias_a, kv)) || (rc = dev_alloc_zeroed(h, &h->d_alias_tn, (size_t)h->V)))) return bail(rc);
  if (has_mh(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_mh, 3))) return bail(rc);
  if (has_word_lists(h->scheme) && ((rc = dev_alloc_zeroed(h, &h->d_nzw, kv)) || (rc = dev_alloc_zeroed(h, &h->d_nw, (size_t)h->V)))) return bail(rc);
  if (has_sparse_stats(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_ps_stats, 4))) return bail(rc);
  if (h->scheme == Scheme::nzvsspalias) {              // the chain's rows, the mask, its outputs
    h->vs_W = (h->V + 31) / 32; h->vs_pitch = (h->K + 31) / 32;
    h->vs_global = h->plan.vschain.lds == 0;
    const size_t kw = (size_t)h->K * h->vs_W, vm = (size_t)h->V * h->vs_pitch;
    if ((rc = dev_alloc(h, &h->d_vs_cz, kw)) || (rc = dev_alloc(h, &h->d_vs_pz, kw)) || (rc = dev_alloc_zeroed(h, &h->d_vs_und, kw)) ||
        (rc = dev_alloc_zeroed(h, &h->d_vs_mask, vm)) || (rc = dev_alloc(h, &h->d_vs_s_end, (size_t)h->K)) || (rc = dev_alloc_zeroed(h, &h->d_vs_rounds, (size_t)h->K)) ||
        (rc = dev_alloc(h, &h->d_vs_zero, 1)) || (h->vs_global && (rc = dev_alloc(h, &h->d_vs_work, 2 * kw))))
      return bail(rc);
  }
  if (poisson_phi(h->scheme)) {
    std::vector<double> T;
    build_poisson_table(h->beta, h->pa_L, T);
    h->pa_t00 = T[0];
    if ((rc = upload(h, &h->d_pa_table, T)) || (rc = dev_alloc(h, &h->d_pa_acc, (size_t)h->K * kPoissonAccStride))) return bail(rc);
  }
  if (count_tables(h->scheme) && (rc = dev_alloc_zeroed(h, &h->d_tpt, (size_t)h->V))) return bail(rc);
  if (h->scheme == Scheme::adlda && ((rc = dev_alloc_zeroed(h, &h->d_ad_den0, (size_t)h->K)) || (rc = dev_alloc_zeroed(h, &h->d_ad_s0, 1)))) return bail(rc);
  if (h->scheme == Scheme::collapsed && (rc = dev_alloc(h, &h->d_lcg, 2))) return bail(rc);
  // 5. events and streams
  for (auto &e : h->ev_part)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return bail(GGS_ERR_HIP);
  for (auto &E : h->evs) {
    for (auto &e : E.e)
      if (hipEventCreate(&e) != hipSuccess) return bail(GGS_ERR_HIP);
    for (auto &e : E.x)
      if (hipEventCreate(&e) != hipSuccess) return bail(GGS_ERR_HIP);
    if (hipEventCreate(&E.th0) != hipSuccess || hipEventCreate(&E.th1) != hipSuccess) return bail(GGS_ERR_HIP);
  }
  {
    // lowest priority: the theta draw fills whatever the Phi phase (on the caller's stream) leaves idle
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    // (a CU-masked side stream was tried: hipExtStreamCreateWithCUMask gives a blocking stream that
    // serialises with the legacy default stream, so the overlap is lost -- priority alone it is)
    if (hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo) != hipSuccess) return bail(GGS_ERR_HIP);
    if (hipStreamCreateWithPriority(&h->side_hot, hipStreamNonBlocking, hi) != hipSuccess || hipEventCreate(&h->ev_hot_fork) != hipSuccess ||
        hipEventCreate(&h->ev_hot_join) != hipSuccess || hipEventCreateWithFlags(&h->ev_chain_done, hipEventDisableTiming) != hipSuccess)
      return bail(GGS_ERR_HIP);
  }
  if (hipDeviceSynchronize() != hipSuccess) return bail(GGS_ERR_HIP);   // the memsets above ran on the null stream
  *out = h;
  return GGS_OK;
}

void ggs_destroy(ggs_handle *h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  (void)hipDeviceSynchronize();
  if (h->d_replays) {                                  // GGS_DEBUG_REPLAYS: the undecided tokens of the float32 cold path, measured
    unsigned long long n = 0;
    if (hipMemcpy(&n, h->d_replays, sizeof(n), hipMemcpyDeviceToHost) == hipSuccess)
      fprintf(stderr, "[ggs] z replays: %llu tokens in %lld launches of z_sliced32_kernel (%.2f per launch)\n", n, (long long)h->z_f32_launches,
              h->z_f32_launches ? (double)n / (double)h->z_f32_launches : 0.0);
  }
  for (void **slot : h->owned)
    if (*slot) (void)hipFree(*slot);
  if (h->d_scratch) (void)hipFree(h->d_scratch);
  if (h->d_heldout_spill) (void)hipFree(h->d_heldout_spill);
  exchange_free(h->xg);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  if (h->comm_stream) (void)hipStreamDestroy(h->comm_stream);
  if (h->ev_half_drawn) (void)hipEventDestroy(h->ev_half_drawn);
  if (h->ev_half_gathered) (void)hipEventDestroy(h->ev_half_gathered);
  for (auto &e : h->ev_part)
    if (e) (void)hipEventDestroy(e);
  for (auto &E : h->evs) {
    for (auto &e : E.e)
      if (e) (void)hipEventDestroy(e);
    for (auto &e : E.x)
      if (e) (void)hipEventDestroy(e);
    if (E.th0) (void)hipEventDestroy(E.th0);
    if (E.th1) (void)hipEventDestroy(E.th1);
  }
  if (h->side) (void)hipStreamDestroy(h->side);
  if (h->side_hot) (void)hipStreamDestroy(h->side_hot);
  if (h->ev_hot_fork) (void)hipEventDestroy(h->ev_hot_fork);
  if (h->ev_hot_join) (void)hipEventDestroy(h->ev_hot_join);
  if (h->ev_chain_done) (void)hipEventDestroy(h->ev_chain_done);
  delete h;
}

int ggs_set_stream(ggs_handle *h, void *hip_stream) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = drop_theta_ahead(h))) return rc;
  if (h->xg && !hip_stream) return set_err(h, GGS_ERR_BAD_ARG, "with an exchange attached the handle does not run on the legacy default stream");
  h->stream = reinterpret_cast<hipStream_t>(hip_stream);
  return GGS_OK;
}

int ggs_set_corpus(ggs_handle *h, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, int64_t doc_base, int64_t tok_base) {
  // 1. validate, before the handle is touched
  if (!h || D < 0 || !doc_ptr || doc_base < 0 || tok_base < 0) return set_err(h, GGS_ERR_BAD_ARG, "bad corpus arguments");
  if (doc_ptr[0] != 0) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr[0] must be 0");
  for (int64_t d = 0; d < D; ++d)
    if (doc_ptr[d + 1] < doc_ptr[d]) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr must be non-decreasing");
  const int64_t N = doc_ptr[D];
  if (N > 0 && !tokens) return set_err(h, GGS_ERR_BAD_ARG, "tokens is null");
  if (N >= (int64_t)1 << 31 || D >= (int64_t)1 << 31) return set_err(h, GGS_ERR_UNSUPPORTED, "more than 2^31-1 tokens or documents per device");
  for (int64_t i = 0; i < N; ++i)
    if (tokens[i] < 0 || tokens[i] >= h->V) return set_err(h, GGS_ERR_BAD_ARG, "token id outside [0, num_types)");
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = drop_theta_ahead(h))) return rc;

  // 2. what this corpus chooses between the plan's entries.  The parts of the z step pay where the theta draw (D x K
  // gammas) is longer than the Phi chain it otherwise hides beside (V x K gammas): the excess is what is drawn beside
  // the z parts.  Measured: D = 100 000, V = 50 000, K = 1 024: 1 part 18.4 ms per sweep, 2: 18.1, 4: 16.5, 8: 15.9;
  // D = 18 846, V = 60 000, K = 200: 8 parts 1.112, 4: 1.071, 2: 1.019, 1: 1.006 (every part costs an event packet, a launch
  // and the drain of the persistent z waves).
  const LaunchPlan &pl = h->plan;
  int32_t parts = pl.cfg_parts.parts;
  if (!pl.parts_forced && parts > 1) parts = D <= (int64_t)h->V ? 1 : D < 2 * (int64_t)h->V ? std::min(parts, 4) : parts;
  h->cfg = parts > 1 ? &pl.cfg_parts : &pl.cfg_plain;

  // 3. the lists, on the host (ggs_corpus_lists.hpp): the count rebuild's, and those of the z step the plan launches
  const bool pcgs = pcgs_family(h->scheme);
  CorpusShape shape;
  shape.V = h->V; shape.tile_tokens = pl.tile_tokens; shape.z_parts = parts;
  shape.pcgs = pcgs; shape.sliced = pl.sliced(); shape.two_rows = pl.two_rows;
  shape.hot_cap = pl.hot_cap; shape.warm_cap = pl.warm_cap; shape.warm_docs = pl.warm_docs;
  shape.warm_tiers_max = pl.warm_tiers_max; shape.warm_min_fill_pct = pl.warm_min_fill_pct; shape.warm_min_chunks_per_wave = pl.warm_min_chunks_per_wave;
  shape.sliced_waves = (int64_t)h->num_cus * kSlicedWaves; shape.pcgs_waves = (int64_t)h->num_cus * pl.lane.per_cu;
  const CorpusLists L = build_corpus_lists(shape, D, doc_ptr, tokens);
  if (pcgs) {
    // the lane-per-document kernels keep the counts as int16: a longer document sends the corpus to the wave-per-document kernel
    h->pcgs_wave = pl.wave_forced || L.longest > kPcgsMaxDocLen;
    if (h->pcgs_wave && !pl.wave.fn) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=pcgs: a document of 32768 tokens or more with more than 4096 topics");
    h->pcgs_z = pcgs_entry(pl, h->scheme, h->pcgs_wave);
    h->pcgs_items = (wave_only(h->scheme) || h->pcgs_wave) ? (int64_t)L.order.size() : ((int64_t)L.order.size() + 63) / 64;   // a wave or a lane per entry
    if (const auto corpus_lds = row_of(h->scheme).corpus_lds) {
      // the list of a document's non-zero topics holds at most min(K, its length) entries (adlda: beside den0, alpha and a block of
      // terms); the resident waves by LDS and, but for spalias, by the kernel's registers.  (The doubly sparse walks took
      // min(lds_workgroups_per_cu(lds, 32), by_regs): with Q = what LDS allows and by_regs >= 1, min(max(1, min(32, Q)), by_regs) =
      // max(1, min(by_regs, 32, Q)) whether min(32, Q) is 0 or not, which is resident_waves_per_cu.)
      h->sp_cap = (int32_t)std::max<int64_t>(1, std::min<int64_t>(h->K, L.longest));
      h->pcgs_z.lds = (int)corpus_lds(h->K, h->sp_cap);
      h->pcgs_z.per_cu = h->scheme == Scheme::spalias ? lds_workgroups_per_cu(h->pcgs_z.lds, 32) : resident_waves_per_cu(h->pcgs_z.fn, h->pcgs_z.lds);
      if (const char *e = debug_env("GGS_DEBUG_SPALIAS_WPC")) h->pcgs_z.per_cu = std::max(1, std::min(h->pcgs_z.per_cu, std::atoi(e)));
    }
  }
  h->D = D; h->N = N; h->C = (int64_t)L.cstart.size(); h->S = (int64_t)L.seg_word.size(); h->doc_base = doc_base; h->tok_base = tok_base;
  h->part_doc = L.part_doc; h->part_chunk = L.part_chunk;
  h->pcgs_order_len = (int64_t)L.order.size();
  h->num_hot = (int32_t)L.hot_words.size(); h->HS = (int64_t)L.hseg_word.size();
  h->Cc = L.Cc; h->Cs = L.Cs;
  h->warm_tiers = L.warm_tiers; h->num_warm = L.num_warm; h->Cw = L.Cw; h->warm_chunks_max = L.warm_chunks_max; h->warm_rows_max = L.warm_rows_max;

  // 4. upload (on the null stream), the state of the corpus zeroed
  const size_t theta_elems = (size_t)D * h->K + 2;
  if ((rc = upload(h, &h->d_doc_ptr, doc_ptr, (size_t)D + 1)) || (rc = upload(h, &h->d_tok, tokens, (size_t)N)) ||
      (rc = upload(h, &h->d_perm, L.perm)) || (rc = upload(h, &h->d_inv_perm, L.inv)) ||
      (rc = upload(h, &h->d_seg_word, L.seg_word)) || (rc = upload(h, &h->d_seg_begin, L.seg_begin)))
    return rc;
  if (pcgs && (rc = upload(h, &h->d_order, L.order))) return rc;
  if (pl.sliced() && ((rc = upload(h, &h->d_ct_tok, L.ct_tok)) || (rc = upload(h, &h->d_ct_idx, L.ct_idx)) || (rc = upload(h, &h->d_ct_ip, L.ct_ip)) ||
                      (rc = upload(h, &h->d_c_docs, L.c_docs)) || (rc = upload(h, &h->d_hot_words, L.hot_words)) ||
                      (rc = upload(h, &h->d_ht_pack, L.ht_pack)) || (rc = upload(h, &h->d_h_docs, L.h_docs)) ||
                      (rc = upload(h, &h->d_hseg_word, L.hseg_word)) || (rc = upload(h, &h->d_hseg_begin, L.hseg_begin)) || (rc = upload(h, &h->d_hseg_end, L.hseg_end))))
    return rc;
  if (h->C && ((rc = upload(h, &h->d_chunk_start, L.cstart)) || (rc = upload(h, &h->d_chunk_doc, L.cdoc)) || (rc = upload(h, &h->d_chunk_len, L.clen)) ||
               (pl.two_rows && (rc = upload(h, &h->d_chunk_doc1, L.cdoc1)))))
    return rc;
  if (L.warm_tiers > 0 && ((rc = upload(h, &h->d_wt_pack, L.wt_pack)) || (rc = upload(h, &h->d_w_docs, L.w_docs)) ||
                           (rc = upload(h, &h->d_warm_words, L.warm_words)) || (rc = upload(h, &h->d_warm_meta, L.warm_meta))))
    return rc;
  const bool with_theta = !counts_only(h->scheme) && !no_theta(h->scheme);   // no theta in its chain and none for a diagnostic (ggs_log_posterior is unsupported); lightpcldaw2: ensure_diag_theta
  if (!with_theta && h->d_theta) { (void)hipFree(h->d_theta); h->d_theta = nullptr; }   // an earlier corpus' diagnostic theta
  if ((rc = dev_alloc(h, &h->d_z, (size_t)N)) || (rc = dev_alloc(h, &h->d_zw, (size_t)N)) ||
      (with_theta && (rc = dev_alloc(h, &h->d_theta, theta_elems))) || (!pcgs && (rc = dev_alloc(h, &h->d_theta_next, theta_elems))))   // theta_next: what the ggs z phase swaps in
    return rc;
  HIP_TRY(h, hipMemset(h->d_z, 0, sizeof(int32_t) * std::max<size_t>((size_t)N, 1)));
  HIP_TRY(h, hipMemset(h->d_zw, 0, sizeof(int32_t) * std::max<size_t>((size_t)N, 1)));
  if (with_theta) HIP_TRY(h, hipMemset(h->d_theta, 0, sizeof(double) * std::max<size_t>((size_t)D * h->K, 1)));
  if (!pcgs) HIP_TRY(h, hipMemset(h->d_theta_next, 0, sizeof(double) * std::max<size_t>((size_t)D * h->K, 1)));
  if (h->d_mh) HIP_TRY(h, hipMemset(h->d_mh, 0, 3 * sizeof(unsigned long long)));
  if (h->d_ps_stats) HIP_TRY(h, hipMemset(h->d_ps_stats, 0, 4 * sizeof(unsigned long long)));
  // the phi mean is the mean over ONE corpus' chain, like the counters above: a sum that ran on into the next corpus' Phi would be neither's
  if (h->d_phi_mean) HIP_TRY(h, hipMemset(h->d_phi_mean, 0, sizeof(double) * (size_t)h->K * h->V));
  h->n_sampled_phi = 0;
  HIP_TRY(h, hipDeviceSynchronize());   // the uploads and memsets above ran on the null stream; the handle's stream may not synchronise with it

  // 5. a new corpus: no Phi, no sweep in progress, the z form to be timed again
  h->have_corpus = true; h->have_phi = false; h->in_sweep = false; h->global_tokens = -1; h->lcg_ready = false;
  h->z_split = pl.split; h->z_split_tried = pl.split_forced;
  h->counts_global = h->xg == nullptr; h->cnt_own_valid = false; h->n_k_valid = false;
  return GGS_OK;
}

int ggs_init_z_java_lcg(ggs_handle *h, int32_t seed) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->tok_base != 0) return set_err(h, GGS_ERR_STATE, "java-LCG init is one sequential stream: only valid with tok_base == 0");
  if ((rc = drop_theta_ahead(h))) return rc;
  // One sequential stream, so it runs on the host exactly once at start-up.
  std::vector<int32_t> z((size_t)h->N);
  const uint64_t lcg_state = java_lcg_next_ints(seed, h->K, h->N, z.data());
  if (h->scheme == Scheme::collapsed) {
    // SerialCollapsedLDA owns ONE Randoms(seed) (SerialCollapsedLDA.java:60-65): addInstances draws the initial topics
    // from it (:789) and the sampling loop goes on with the same object (MSLDA:206): the serial sweep continues this stream
    HIP_TRY(h, hipMemcpyAsync(h->d_lcg, &lcg_state, sizeof lcg_state, hipMemcpyHostToDevice, h->stream));
    h->lcg_ready = true;
  }
  if (h->N) HIP_TRY(h, hipMemcpyAsync(h->d_z, z.data(), sizeof(int32_t) * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  if ((rc = launch_permute_z(h))) return rc;
  if ((rc = launch_count_rebuild(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GGS_OK;
}

int ggs_set_z(ggs_handle *h, const int32_t *z, int32_t redraw_phi) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->N > 0 && !z) return set_err(h, GGS_ERR_BAD_ARG, "z is null");
  for (int64_t i = 0; i < h->N; ++i)
    if (z[i] < 0 || z[i] >= h->K) return set_err(h, GGS_ERR_BAD_ARG, "topic indicator outside [0, num_topics)");
  if ((rc = drop_theta_ahead(h))) return rc;
  h->lcg_ready = false;                                // a restored z is not the state any java.util.Random stream left: the serial chain starts a new Random(java_seed)
  if (h->N) HIP_TRY(h, hipMemcpyAsync(h->d_z, z, sizeof(int32_t) * (size_t)h->N, hipMemcpyHostToDevice, h->stream));
  if ((rc = launch_permute_z(h))) return rc;
  if ((rc = launch_count_rebuild(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (redraw_phi) return ggs_init_phi(h);
  return GGS_OK;
}

int ggs_init_phi(ggs_handle *h) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme)) {   // nothing to draw: corpus-wide counts and tokensPerTopic are the whole model
    if ((rc = launch_magnitude(h))) return rc;
    h->have_phi = true;
    return check_status(h);
  }
  if ((rc = launch_phi(h, true, false))) return rc;   // with an exchange: the start-up count reduce-scatter, the slice, the all-gather
  return check_status(h);
}

int ggs_set_iteration(ggs_handle *h, int32_t it) {     // a theta drawn ahead for another iteration is simply not used
  if (!h) return GGS_ERR_BAD_ARG;
  if (it < 0) return set_err(h, GGS_ERR_BAD_ARG, "the iteration number is 0 ... INT32_MAX");
  h->iteration = it;
  return GGS_OK;
}
// iterations are 0 ... INT32_MAX: a call whose steps would count past the end is refused as a whole, before anything is launched
static int iteration_room(ggs_handle *h, int32_t steps) {
  if (steps > 0 && (int64_t)h->iteration + (int64_t)steps > (int64_t)INT32_MAX)
    return set_err(h, GGS_ERR_STATE, "the iteration number would pass INT32_MAX");
  return GGS_OK;
}
int ggs_get_iteration(const ggs_handle *h, int32_t *it) { if (!h || !it) return GGS_ERR_BAD_ARG; *it = h->iteration; return GGS_OK; }

// see theta_main: only where the z step is one launch pair (no parts), theta is drawn at all, no collective is in the chain, and
// the theta draw (D x K gammas) is the longer leg (the Phi chain draws V x K)
bool chain_on_side_ok(const ggs_handle *h) {
  return h->theta_main && h->plan.sliced() && h->side_hot && h->ev_chain_done && !h->xg &&
         (h->D >= (int64_t)h->V || h->theta_main_always);
}

int ggs_sweep_begin(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_begin called twice without ggs_sweep_end");
  if ((rc = iteration_room(h, 1))) return rc;
  h->iteration += 1;                                   // currentIteration = iteration, UPLDA:646
  h->chain_on_side = chain_on_side_ok(h);              // kept until the sweep's end
  if ((rc = z_phase(h))) { h->chain_on_side = false; return rc; }
  h->in_sweep = true;
  return GGS_OK;
}

int ggs_sweep_end(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_end without ggs_sweep_begin");
  h->in_sweep = false;
  rc = finish_sweep(h, true);
  h->chain_on_side = false;
  return rc;
}

int ggs_sweep_end_async(ggs_handle *h) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!h->in_sweep) return set_err(h, GGS_ERR_STATE, "ggs_sweep_end_async without ggs_sweep_begin");
  h->in_sweep = false;
  rc = finish_sweep(h, true, false);
  h->chain_on_side = false;
  return rc;
}

int ggs_sweep(ggs_handle *h, int32_t n_sweeps) {
  if (h && n_sweeps > 0) {                             // all n_sweeps or none
    int rc = require_ready(h, true);
    if (rc || (rc = iteration_room(h, n_sweeps))) return rc;
  }
  for (int32_t i = 0; i < n_sweeps; ++i) {
    if (h) h->whole_sweep = true;
    int rc = ggs_sweep_begin(h);
    if (!rc) {
      h->in_sweep = false;
      rc = finish_sweep(h, true, i == n_sweeps - 1);
    }
    if (h) h->chain_on_side = h->whole_sweep = false;
    if (rc) return rc;
  }
  return GGS_OK;
}

int ggs_collapsed_serial_sweep(ggs_handle *h, int32_t java_seed, int32_t n_sweeps) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->scheme != Scheme::collapsed) return set_err(h, GGS_ERR_STATE, "ggs_collapsed_serial_sweep needs GGS_FLAG_COLLAPSED");
  if (h->xg || h->tok_base != 0) return set_err(h, GGS_ERR_STATE, "the serial chain runs over ONE unsharded corpus");
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  if ((size_t)h->K * 16 > (size_t)kMaxLdsBytes) return set_err(h, GGS_ERR_UNSUPPORTED, "num_topics too large for the serial kernel's LDS");
  if ((rc = iteration_room(h, n_sweeps))) return rc;
  if ((rc = launch_magnitude(h))) return rc;           // tokensPerTopic in step with the counts
  if (!h->lcg_ready) {                                 // new java.util.Random(seed): the scrambled initial state
    const uint64_t st = ((uint64_t)(int64_t)java_seed ^ 0x5DEECE66DULL) & ((1ULL << 48) - 1);
    HIP_TRY(h, hipMemcpyAsync(h->d_lcg, &st, sizeof st, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->lcg_ready = true;
  }
  CollapsedSerialParams cp{};
  cp.doc_ptr = h->d_doc_ptr; cp.tok = h->d_tok; cp.inv_perm = h->d_inv_perm; cp.z = h->d_z; cp.zw = h->d_zw; cp.n_wk = h->d_n_wk; cp.n_k = h->d_n_k;
  cp.alpha = h->d_alpha; cp.lcg = h->d_lcg; cp.status = h->d_status; cp.num_docs = h->D; cp.beta = h->beta; cp.beta_sum = h->beta * (double)h->V; cp.K = h->K;
  for (int32_t i = 0; i < n_sweeps; ++i) {
    h->iteration += 1;
    hipLaunchKernelGGL(collapsed_serial_kernel, dim3(1), dim3(64), (size_t)h->K * 16, h->stream, cp);
  }
  HIP_TRY(h, hipGetLastError());
  h->have_phi = true;
  return check_status(h);
}

int ggs_sample_z_given_phi(ggs_handle *h, int32_t n_sweeps) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  if (count_form(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, scheme=lightcollapsed and scheme=adlda have no Phi to condition on");
  if ((rc = iteration_room(h, n_sweeps))) return rc;
  for (int32_t i = 0; i < n_sweeps; ++i) {
    h->iteration += 1;                                 // UPLDA:980
    h->force_detail = true;
    rc = z_phase(h);
    h->force_detail = false;
    if (rc) return rc;
    if ((rc = finish_sweep(h, false))) return rc;
  }
  // tokensPerTopic follows the rebuilt counts (with an exchange: the counts are merged here, UPLDA:993)
  if ((rc = launch_magnitude(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GGS_OK;
}

int ggs_counts_device_ptr(ggs_handle *h, void **dev_ptr, int64_t *num_elems) {
  if (!h || !dev_ptr || !num_elems) return GGS_ERR_BAD_ARG;
  if (h->xg) return set_err(h, GGS_ERR_STATE, "an exchange is attached: the library merges the counts itself");
  *dev_ptr = h->d_n_wk; *num_elems = (int64_t)h->K * h->V;
  h->n_k_valid = false;          // the caller may sum other shards' counts into the buffer
  return GGS_OK;
}

int ggs_set_global_token_count(ggs_handle *h, int64_t n_tokens) {
  if (!h || n_tokens < 0) return GGS_ERR_BAD_ARG;
  h->global_tokens = n_tokens;
  return GGS_OK;
}

// ---- multi-GPU: the exchange (include/ggs_hip.h) ------------------------------------------------------------------
int ggs_attach_exchange(ggs_handle *h, int32_t rank, int32_t nranks, const ggs_exchange_ops *ops) {
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  if (!ops || (ops->struct_size != (int32_t)sizeof(ggs_exchange_ops) && ops->struct_size != GGS_EXCHANGE_OPS_V3_SIZE) || !ops->reduce_scatter_i32 ||
      !ops->all_gather_f64 || !ops->all_gather_i32)
    return set_err(h, GGS_ERR_BAD_ARG, "ggs_exchange_ops: wrong struct_size or a null callback");
  auto *x = new (std::nothrow) Exchange();
  if (!x) return GGS_ERR_HIP;
  x->rank = rank; x->nranks = nranks;
  std::memcpy(&x->ops, ops, (size_t)ops->struct_size);   // a version-3 table has no all_to_all_v_i32: it stays null, the count exchange dense
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops);
  return setup_exchange(h, x);
}

int ggs_attach_null_exchange(ggs_handle *h, int32_t rank, int32_t nranks) {
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  auto *x = new (std::nothrow) Exchange();
  if (!x) return GGS_ERR_HIP;
  x->rank = rank; x->nranks = nranks; x->is_null = true;
  x->ops.struct_size = (int32_t)sizeof(ggs_exchange_ops); x->ops.ctx = x;
  x->ops.reduce_scatter_i32 = xops::null_reduce_scatter_i32;
  x->ops.all_gather_f64 = xops::null_all_gather<double>;
  x->ops.all_gather_i32 = xops::null_all_gather<int32_t>;
  x->ops.all_to_all_v_i32 = xops::null_all_to_all_v_i32;
  return setup_exchange(h, x);
}

int ggs_rccl_unique_id(void *out_id) {
  if (!out_id) return GGS_ERR_BAD_ARG;
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) return GGS_ERR_UNSUPPORTED;
  static_assert(sizeof(ncclUniqueId) == GGS_RCCL_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return GGS_ERR_HIP;
  std::memcpy(out_id, &id, sizeof id);
  return GGS_OK;
}

int ggs_attach_rccl(ggs_handle *h, int32_t rank, int32_t nranks, const void *unique_id) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!unique_id) return set_err(h, GGS_ERR_BAD_ARG, "null unique id");
  int rc = exchange_precheck(h, rank, nranks);       // before the blocking collective below: a rejected call must not have joined it
  if (rc) return rc;
  Exchange *x = new_rccl_exchange(h, rank, nranks, &rc);
  if (!x) return rc;
  ncclUniqueId id;
  std::memcpy(&id, unique_id, sizeof id);
  const ncclResult_t r = x->api->CommInitRank(&x->comm, nranks, id, rank);      // collective: every rank of the job is in here
  if (r != ncclSuccess) {
    const std::string msg = std::string("ncclCommInitRank: ") + x->api->GetErrorString(r);
    delete x;
    return set_err(h, GGS_ERR_HIP, msg);
  }
  x->own_comm = true;
  return setup_exchange(h, x);
}

int ggs_attach_rccl_comm(ggs_handle *h, int32_t rank, int32_t nranks, void *nccl_comm) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (!nccl_comm) return set_err(h, GGS_ERR_BAD_ARG, "null communicator");
  int rc = exchange_precheck(h, rank, nranks);
  if (rc) return rc;
  Exchange *x = new_rccl_exchange(h, rank, nranks, &rc);
  if (!x) return rc;
  x->comm = static_cast<ncclComm_t>(nccl_comm);
  return setup_exchange(h, x);
}

int ggs_get_exchange_info(const ggs_handle *h, int32_t *rank, int32_t *nranks, int32_t *k_begin, int32_t *k_end) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (rank) *rank = h->xg ? h->xg->rank : 0;
  if (nranks) *nranks = h->xg ? h->xg->nranks : 1;
  if (k_begin) *k_begin = h->k0;
  if (k_end) *k_end = h->k0 + h->Ks;
  return GGS_OK;
}

int ggs_set_count_exchange(ggs_handle *h, int32_t mode) {
  if (!h || mode < 0 || mode > 2) return GGS_ERR_BAD_ARG;
  if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
  h->count_mode = mode;
  return GGS_OK;
}
int ggs_get_count_exchange(const ggs_handle *h, int32_t *sparse, int64_t *pairs_last, int64_t *cells) {
  if (!h || !sparse) return GGS_ERR_BAD_ARG;
  *sparse = use_sparse(h) ? 1 : 0;
  if (pairs_last) *pairs_last = h->sp_pairs_last;
  if (cells) *cells = h->xg ? (int64_t)h->V * h->Ksm * h->xg->nranks : (int64_t)h->V * h->K;
  return GGS_OK;
}

int ggs_get_exchange_provider(const ggs_handle *h, int32_t *provider, int32_t *comm_nranks, int32_t *comm_rank) {
  if (!h) return GGS_ERR_BAD_ARG;
  const Exchange *x = h->xg;
  if (provider) *provider = !x ? 0 : x->api ? 1 : x->is_null ? 3 : 2;
  int n = x ? x->nranks : 1, r = x ? x->rank : 0;
  if (x && x->api && x->comm) {                         // what the communicator itself reports, not what the caller passed in
    if (x->api->CommCount && x->api->CommCount(x->comm, &n) != ncclSuccess) n = -1;
    if (x->api->CommUserRank && x->api->CommUserRank(x->comm, &r) != ncclSuccess) r = -1;
  }
  if (comm_nranks) *comm_nranks = n;
  if (comm_rank) *comm_rank = r;
  return GGS_OK;
}

// ---- one process, n GPUs ----
namespace {
bool is_group(ggs_handle **hs, int32_t n) {
  if (!hs || n < 1 || !hs[0] || (int32_t)hs[0]->group.size() != n) return false;
  for (int32_t i = 0; i < n; ++i)
    if (hs[i] != hs[0]->group[(size_t)i] || !hs[i]->xg || hs[i]->xg->api != hs[0]->xg->api) return false;   // all RCCL, or all the caller's transport
  return true;
}

// the Phi phase for every handle of the group: each collective step for all devices inside ncclGroupStart/End
int group_phi(ggs_handle **hs, int32_t n, bool initial, bool in_sweep) {
  std::vector<char> acc((size_t)n, 0);
  int rc = GGS_OK;
  for (int32_t i = 0; i < n && !rc; ++i) {
    ggs_handle *h = hs[i];
    if ((rc = bind_device(h))) break;
    if (in_sweep) {
      Events &E = h->evs[h->ev_head];
      if (!E.light && hipEventRecord(E.e[4], h->stream) != hipSuccess) { rc = set_err(h, GGS_ERR_HIP, "hipEventRecord"); break; }
      E.exchanged = true; E.e4_is_e3 = false;
      acc[(size_t)i] = (h->flags & GGS_FLAG_SAVE_PHI_MEAN) && sample_phi_this_iteration(h);
    }
  }
  if (rc) return rc;
  auto timed = [&](ggs_handle *h) -> Events * { return (in_sweep && !h->evs[h->ev_head].light) ? &h->evs[h->ev_head] : nullptr; };   // a light sweep records no phase events
  auto grouped = [&](auto step) { return group_collective(hs, n, [&](ggs_handle *h) { return step(h, timed(h)); }); };
  // a step for every handle; events are recorded AFTER a grouped step: inside ncclGroupStart/End the collectives are
  // only collected, and an event recorded there would land on the stream before them
  auto each = [&](auto step) {
    int r = GGS_OK;
    for (int32_t i = 0; i < n && !r; ++i)
      if (!(r = bind_device(hs[i]))) r = step(hs[i], timed(hs[i]));
    return r;
  };
  auto record = [](ggs_handle *h, hipEvent_t ev) { return hipEventRecord(ev, h->stream) == hipSuccess ? GGS_OK : set_err(h, GGS_ERR_HIP, "hipEventRecord"); };
  if ((rc = grouped([](ggs_handle *h, Events *) { return phi_step_a(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { int r = phi_step_a_clear(h); if (!r && E) r = record(h, E->x[0]); return r ? r : phi_step_b1(h, initial); })) ||
      (rc = grouped([](ggs_handle *h, Events *) { return phi_step_g0(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { int r = phi_step_b2(h, initial); if (!r && E) r = record(h, E->x[1]); return r ? r : phi_join_halves(h); })) ||
      (rc = grouped([](ggs_handle *h, Events *) { return phi_step_g1(h); })) ||
      (rc = each([&](ggs_handle *h, Events *E) { return E ? record(h, E->x[2]) : GGS_OK; })))
    return rc;
  for (int32_t i = 0; i < n; ++i) {
    ggs_handle *h = hs[i];
    if ((rc = bind_device(h)) || (rc = phi_step_c(h, initial, acc[(size_t)i] != 0)) || (rc = launch_alias_build(h))) return rc;
    if (in_sweep) {
      HIP_TRY(h, hipEventRecord(h->evs[h->ev_head].e[5], h->stream));
      if (acc[(size_t)i]) h->n_sampled_phi++;
      h->ev_pending += 1;
    }
  }
  return GGS_OK;
}
}  // namespace

namespace {
// corpus-wide counts on every handle of the group: the two collectives of ensure_global_counts, each grouped
int group_gather_counts(ggs_handle **hs, int32_t n) {
  int rc;
  if ((rc = group_collective(hs, n, [](ggs_handle *h) { return h->counts_global ? GGS_OK : exchange_reduce_scatter(h); }))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = bind_device(hs[i])) || (rc = clear_send_buffer_if_dead(hs[i], hs[i]->stream))) return rc;
  if ((rc = group_collective(hs, n, [](ggs_handle *h) { return h->counts_global ? GGS_OK : gather_counts_step_gather(h); }))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if (!hs[i]->counts_global && ((rc = bind_device(hs[i])) || (rc = gather_counts_step_unslice(hs[i])))) return rc;
  return GGS_OK;
}
}  // namespace

int ggs_group_gather_counts(ggs_handle **hs, int32_t n) {
  if (!is_group(hs, n)) return GGS_ERR_BAD_ARG;
  return group_gather_counts(hs, n);
}

int ggs_group_create(const ggs_config *cfg, int32_t n, const int32_t *device_ids, ggs_handle **out) {
  if (!cfg || n < 1 || !device_ids || !out) return GGS_ERR_BAD_ARG;
  for (int32_t i = 0; i < n; ++i) out[i] = nullptr;
  std::string err;
  RcclApi *api = RcclApi::get(err);
  if (!api) return GGS_ERR_UNSUPPORTED;
  int rc = GGS_OK;
  for (int32_t i = 0; i < n && !rc; ++i) {
    ggs_config c = *cfg;
    c.device_id = device_ids[i];
    rc = ggs_create(&c, &out[i]);
  }
  std::vector<ncclComm_t> comms((size_t)n, nullptr);
  if (!rc && api->CommInitAll(comms.data(), n, device_ids) != ncclSuccess) rc = GGS_ERR_HIP;
  for (int32_t i = 0; i < n && !rc; ++i) {
    Exchange *x = new_rccl_exchange(out[i], i, n, &rc);
    if (!x) break;
    x->comm = comms[(size_t)i]; x->own_comm = true; comms[(size_t)i] = nullptr;
    rc = setup_exchange(out[i], x);
  }
  if (rc) {
    for (ncclComm_t c : comms) if (c) (void)api->CommDestroy(c);
    for (int32_t i = 0; i < n; ++i) { ggs_destroy(out[i]); out[i] = nullptr; }
    return rc;
  }
  out[0]->group.assign(out, out + n);
  for (int32_t i = 0; i < n; ++i) out[i]->in_group = true;
  return GGS_OK;
}

int ggs_group_adopt(ggs_handle **hs, int32_t n) {
  if (!hs || n < 1) return GGS_ERR_BAD_ARG;
  for (int32_t i = 0; i < n; ++i) {
    if (!hs[i]) return GGS_ERR_BAD_ARG;
    if (!hs[i]->xg || hs[i]->xg->api) return set_err(hs[i], GGS_ERR_STATE, "ggs_group_adopt takes handles with a caller-supplied exchange (ggs_attach_exchange)");
    if (hs[i]->xg->rank != i || hs[i]->xg->nranks != n) return set_err(hs[i], GGS_ERR_BAD_ARG, "ggs_group_adopt: handle i must be rank i of n");
  }
  hs[0]->group.assign(hs, hs + n);
  for (int32_t i = 0; i < n; ++i) hs[i]->in_group = true;
  return GGS_OK;
}

void ggs_group_destroy(ggs_handle **handles, int32_t n) {
  if (!handles) return;
  for (int32_t i = 0; i < n; ++i) { ggs_destroy(handles[i]); handles[i] = nullptr; }
}

int ggs_group_set_z(ggs_handle **hs, int32_t n, const int32_t *const *z, int32_t redraw_phi) {
  if (!is_group(hs, n) || !z) return GGS_ERR_BAD_ARG;
  int rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = ggs_set_z(hs[i], z[i], 0))) return rc;          // this shard's counts
  if (!redraw_phi) return GGS_OK;
  if (count_form(hs[0]->scheme)) {                                                 // no Phi: the merged counts and tokensPerTopic are the model
    if ((rc = group_gather_counts(hs, n))) return rc;
    for (int32_t i = 0; i < n; ++i) {
      if ((rc = bind_device(hs[i])) || (rc = launch_magnitude(hs[i]))) return rc;
      hs[i]->have_phi = true;
    }
  } else if ((rc = group_phi(hs, n, true, false))) return rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = bind_device(hs[i])) || (rc = check_status(hs[i]))) return rc;
  return GGS_OK;
}

int ggs_group_sweep(ggs_handle **hs, int32_t n, int32_t n_sweeps) {
  if (!is_group(hs, n)) return GGS_ERR_BAD_ARG;
  int rc;
  for (int32_t i = 0; i < n; ++i)
    if ((rc = iteration_room(hs[i], n_sweeps))) return rc;
  for (int32_t s = 0; s < n_sweeps; ++s) {
    if ((count_form(hs[0]->scheme) || count_tables(hs[0]->scheme)) && (rc = group_gather_counts(hs, n))) return rc;   // the z step conditions on the corpus-wide sweep-start counts
    for (int32_t i = 0; i < n; ++i) {
      ggs_handle *h = hs[i];
      if ((rc = require_ready(h, true))) return rc;
      if (h->in_sweep) return set_err(h, GGS_ERR_STATE, "inside a split sweep");
      h->iteration += 1;
      if ((rc = z_phase(h))) return rc;
    }
    if (count_form(hs[0]->scheme)) {                                               // the AD-LDA merge: gathered counts, then tokensPerTopic; no Phi
      if ((rc = group_gather_counts(hs, n))) return rc;
      for (int32_t i = 0; i < n; ++i) {
        ggs_handle *h = hs[i];
        if ((rc = bind_device(h))) return rc;
        Events &E = h->evs[h->ev_head];
        E.exchanged = false; E.e4_is_e3 = false;
        HIP_TRY(h, hipEventRecord(E.e[4], h->stream));
        if ((rc = launch_magnitude(h))) return rc;
        HIP_TRY(h, hipEventRecord(E.e[5], h->stream));
        h->ev_pending += 1;
      }
    } else if ((rc = group_phi(hs, n, false, true))) return rc;
    if (s == n_sweeps - 1 || (hs[0]->flags & GGS_FLAG_PARANOID))
      for (int32_t i = 0; i < n; ++i)
        if ((rc = bind_device(hs[i])) || (rc = check_status(hs[i])) || (rc = settle_sweeps(hs[i]))) return rc;
  }
  return GGS_OK;
}

static int copy_out(ggs_handle *h, void *dst, const void *src, size_t bytes) {
  if (!bytes) return GGS_OK;
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  return GGS_OK;
}

int ggs_synchronize(ggs_handle *h) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  return check_status(h);
}

int ggs_get_z(ggs_handle *h, int32_t *z) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (h->N > 0 && !z) return GGS_ERR_BAD_ARG;
  return copy_out(h, z, h->d_z, sizeof(int32_t) * (size_t)h->N);
}
int ggs_get_type_topic_counts(ggs_handle *h, int32_t *n_wk) {
  if (!h || !n_wk) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  return copy_out(h, n_wk, h->d_n_wk, sizeof(int32_t) * (size_t)h->K * h->V);
}
int ggs_get_topic_totals(ggs_handle *h, int32_t *n_k) {
  if (!h || !n_k) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  // valid whatever came last: a sweep, ggs_set_z(redraw=0), an external all-reduce on ggs_counts_device_ptr
  h->n_k_valid = h->n_k_valid && h->xg != nullptr;
  if ((rc = launch_magnitude(h))) return rc;
  return copy_out(h, n_k, h->d_n_k, sizeof(int32_t) * (size_t)h->K);
}

static int phi_out(ggs_handle *h, const double *src_T, int32_t pitch, double *dst, double scale) {
  const size_t kv = (size_t)h->K * h->V;
  int rc = ensure_scratch(h, kv * sizeof(double));
  if (rc) return rc;
  hipLaunchKernelGGL(phiT_to_phi_kernel, dim3(grid_for((int64_t)kv, 256)), dim3(256), 0, h->stream, src_T, static_cast<double *>(h->d_scratch),
                     h->K, pitch, h->V, scale);
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, dst, h->d_scratch, kv * sizeof(double));
}
int ggs_get_phi(ggs_handle *h, double *phi) {
  if (!h || !phi) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (count_form(h->scheme)) {   // the point estimate from the current counts
    if (!h->d_phiT && (rc = dev_alloc(h, &h->d_phiT, (size_t)h->V * h->Kp + kPhiTailPadBytes / 8))) return rc;   // lightcollapsed: only now
    if ((rc = launch_magnitude(h))) return rc;
    hipLaunchKernelGGL(psi_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 2)), dim3(256), 0, h->stream, h->d_n_wk, h->d_n_k, h->beta, h->beta * (double)h->V,
                       h->d_phiT, h->K, h->Kp, h->V);
    HIP_TRY(h, hipGetLastError());
  }
  return phi_out(h, h->d_phiT, h->Kp, phi, 1.0);
}
int ggs_set_phi(ggs_handle *h, const double *phi) {
  if (!h || !phi) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (counts_only(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightcollapsed and scheme=adlda have no Phi to set");
  const size_t kv = (size_t)h->K * h->V;
  if (h->have_priors) {   // the z step leaves the prior factor out because Phi is exactly zero wherever the prior is (ggs_hip.h)
    for (int32_t v = 0; v < h->V; ++v)
      for (int32_t j = 0; j < h->pr_pitch; ++j)
        for (uint32_t bits = h->pr_mask[(size_t)v * h->pr_pitch + j]; bits; bits &= bits - 1)
          if (phi[(size_t)(j * 32 + __builtin_ctz(bits)) * h->V + v] != 0.0)
            return set_err(h, GGS_ERR_BAD_ARG, "ggs_set_phi: phi is not zero in a cell the topic priors zero");
  }
  if ((rc = ensure_scratch(h, kv * sizeof(double)))) return rc;
  HIP_TRY(h, hipMemcpyAsync(h->d_scratch, phi, kv * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(phi_to_phiT_kernel, dim3(grid_for((int64_t)kv, 256)), dim3(256), 0, h->stream, static_cast<const double *>(h->d_scratch),
                     h->d_phiT, h->K, h->Kp, h->V, h->d_phiT32, h->plan.Kp32);
  HIP_TRY(h, hipGetLastError());
  // UPLDA:1897-1902: `if (savePhiMeans()) phiMean = new double[numTopics][numTypes]` -- the running sum restarts, noSampledPhi keeps counting
  if (h->d_phi_mean) HIP_TRY(h, hipMemsetAsync(h->d_phi_mean, 0, kv * sizeof(double), h->stream));
  h->alias_stale = true;
  h->vs_lists = ggs_handle::VsLists::nonzero;          // nzvsspalias: the lists of a Phi that was set are its non-zero cells (ours)
  h->vs_drawn = false;                                 // ... and no draw stands behind it: ggs_get_vs_stats reports none
  if ((rc = launch_alias_build(h))) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  h->have_phi = true;
  return GGS_OK;
}

int ggs_set_topic_priors(ggs_handle *h, int64_t n_zero, const int32_t *topic, const int32_t *word) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::spalias) return set_err(h, GGS_ERR_STATE, "ggs_set_topic_priors needs GGS_FLAG_SPALIAS");
  if (h->have_phi) return set_err(h, GGS_ERR_STATE, "ggs_set_topic_priors: the handle already has a Phi");
  if (n_zero < 0 || (n_zero > 0 && (!topic || !word))) return set_err(h, GGS_ERR_BAD_ARG, "bad topic prior arguments");
  // 1. validate into a mask of its own: a refused call leaves the handle as it was
  const int32_t pitch = (h->K + 31) / 32;
  std::vector<uint32_t> mask((size_t)h->V * pitch, 0u);
  std::vector<int32_t> per_topic((size_t)h->K, 0), per_word((size_t)h->V, 0);
  for (int64_t i = 0; i < n_zero; ++i) {
    const int32_t k = topic[i], v = word[i];
    if (k < 0 || k >= h->K || v < 0 || v >= h->V) return set_err(h, GGS_ERR_BAD_ARG, "topic prior cell outside [0, num_topics) x [0, num_types)");
    uint32_t &m = mask[(size_t)v * pitch + (k >> 5)];
    if (m & (1u << (k & 31))) continue;                // duplicates are allowed
    m |= 1u << (k & 31);
    per_topic[(size_t)k] += 1; per_word[(size_t)v] += 1;
  }
  // ensureConsistentPriors, SpaliasUncollapsedParallelWithPriors.java:102-121
  for (int32_t k = 0; k < h->K; ++k)
    if (per_topic[(size_t)k] == h->V) return set_err(h, GGS_ERR_BAD_ARG, "Inconsistent prior spec, one topic has all Zero priors!");
  for (int32_t v = 0; v < h->V; ++v)
    if (per_word[(size_t)v] == h->K) return set_err(h, GGS_ERR_BAD_ARG, "Inconsistent prior spec, word " + std::to_string(v) + " has all Zero priors!");
  // 2. what the conditional Phi phase needs
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = upload(h, &h->d_pr_mask, mask)) || (rc = dev_alloc(h, &h->d_pr_sum_phi, (size_t)h->K))) return rc;
  if (h->exact_sum && ((rc = dev_alloc(h, &h->d_pr_pref, ((size_t)h->sum_nseg + 1) * h->K)) || (rc = dev_alloc(h, &h->d_pr_fn, (size_t)h->sum_nseg * h->K * 4))))
    return rc;
  h->pr_mask.swap(mask);
  h->pr_pitch = pitch;
  h->have_priors = true;
  return GGS_OK;
}

int ggs_get_topic_priors(ggs_handle *h, double *priors) {
  if (!h || !priors) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::spalias) return set_err(h, GGS_ERR_STATE, "ggs_get_topic_priors needs GGS_FLAG_SPALIAS");
  std::fill(priors, priors + (size_t)h->K * h->V, 1.0);
  if (!h->have_priors) return GGS_OK;
  std::vector<uint32_t> mask((size_t)h->V * h->pr_pitch);       // the mask the kernels read
  if ((rc = copy_out(h, mask.data(), h->d_pr_mask, mask.size() * sizeof(uint32_t)))) return rc;
  for (int32_t v = 0; v < h->V; ++v)
    for (int32_t j = 0; j < h->pr_pitch; ++j)
      for (uint32_t bits = mask[(size_t)v * h->pr_pitch + j]; bits; bits &= bits - 1)
        priors[(size_t)(j * 32 + __builtin_ctz(bits)) * h->V + v] = 0.0;
  return GGS_OK;
}

// What ggs_get_alias_tables and ggs_get_word_topic_lists read, brought up to date: of the current counts (a count-form scheme: what
// the next sweep builds at its head), or of the current Phi
static int refresh_tables(ggs_handle *h) {
  int rc;
  if (count_form(h->scheme) || count_tables(h->scheme)) return (rc = require_ready(h, false)) ? rc : launch_sweep_head(h);
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi yet: call ggs_init_phi or ggs_set_phi first");
  return h->alias_stale ? launch_alias_build(h) : GGS_OK;
}
int ggs_get_alias_tables(ggs_handle *h, double *ps, int32_t *a, double *type_norm) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_tables(h->scheme))                          // adlda: lightcollapsed's sibling has them; promised GGS_ERR_UNSUPPORTED in ggs_hip.h
    return counts_only(h->scheme) ? set_err(h, GGS_ERR_UNSUPPORTED, "scheme=adlda builds no alias tables") : set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_alias_tables", kHasTables));
  if ((rc = refresh_tables(h))) return rc;
  const size_t kv = (size_t)h->K * h->V;
  std::vector<int32_t> n(count_tables(h->scheme) ? (size_t)h->V : 0);   // lightcollapsed, lightpcldaw2: the kernel writes a row's first nw[w] entries
  if (!n.empty()) HIP_TRY(h, hipMemcpyAsync(n.data(), h->d_nw, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (ps) HIP_TRY(h, hipMemcpyAsync(ps, h->d_alias_ps, kv * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (a) HIP_TRY(h, hipMemcpyAsync(a, h->d_alias_a, kv * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (type_norm) HIP_TRY(h, hipMemcpyAsync(type_norm, h->d_alias_tn, (size_t)h->V * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (size_t w = 0; w < n.size(); ++w)                // ... behind them ps = 1.0, a = the index
    for (int32_t i = n[w]; i < h->K; ++i) {
      if (ps) ps[w * h->K + i] = 1.0;
      if (a) a[w * h->K + i] = i;
    }
  return GGS_OK;
}
int ggs_get_mh_stats(ggs_handle *h, int64_t out[3]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_mh(h->scheme))                              // adlda: as in ggs_get_alias_tables
    return counts_only(h->scheme) ? set_err(h, GGS_ERR_UNSUPPORTED, "scheme=adlda has no Metropolis-Hastings step") : set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_mh_stats", kHasMh));
  unsigned long long v[3];
  HIP_TRY(h, hipMemcpyAsync(v, h->d_mh, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 3; ++i) out[i] = (int64_t)v[i];
  return GGS_OK;
}
int ggs_get_word_topic_lists(ggs_handle *h, int32_t *nw, int32_t *topics) {
  if (!h) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_word_lists(h->scheme)) return set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_word_topic_lists", kHasWordLists));
  if ((rc = refresh_tables(h))) return rc;
  const size_t kv = (size_t)h->K * h->V;
  std::vector<int32_t> n((size_t)h->V);
  std::vector<uint16_t> l(topics ? kv : 0);
  HIP_TRY(h, hipMemcpyAsync(n.data(), h->d_nw, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  if (topics) HIP_TRY(h, hipMemcpyAsync(l.data(), h->d_nzw, kv * sizeof(uint16_t), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if (nw) std::copy(n.begin(), n.end(), nw);
  if (topics)
    for (int32_t w = 0; w < h->V; ++w)
      for (int32_t i = 0; i < h->K; ++i) topics[(size_t)w * h->K + i] = i < n[(size_t)w] ? (int32_t)l[(size_t)w * h->K + i] : -1;
  return GGS_OK;
}
int ggs_get_sparse_stats(ggs_handle *h, int64_t out[4]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (!has_sparse_stats(h->scheme)) return set_err(h, GGS_ERR_STATE, needs_flag("ggs_get_sparse_stats", kSparseStats));
  unsigned long long v[4];
  HIP_TRY(h, hipMemcpyAsync(v, h->d_ps_stats, sizeof(v), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < 4; ++i) out[i] = (int64_t)v[i];
  return GGS_OK;
}
int ggs_set_variable_selection_prior(ggs_handle *h, double pi) {
  if (!h) return GGS_ERR_BAD_ARG;
  if (h->scheme != Scheme::nzvsspalias) return set_err(h, GGS_ERR_STATE, "ggs_set_variable_selection_prior needs GGS_FLAG_NZVSSPALIAS");
  if (h->have_phi) return set_err(h, GGS_ERR_STATE, "ggs_set_variable_selection_prior: the handle already has a Phi");
  if (!(pi > 0.0 && pi < 1.0)) return set_err(h, GGS_ERR_BAD_ARG, "the variable-selection prior must lie in (0, 1)");
  h->vs_pi = pi;
  return GGS_OK;
}
int ggs_get_vs_stats(ggs_handle *h, int64_t out[3]) {
  if (!h || !out) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  if (h->scheme != Scheme::nzvsspalias) return set_err(h, GGS_ERR_STATE, "ggs_get_vs_stats needs GGS_FLAG_NZVSSPALIAS");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi yet: call ggs_init_phi or ggs_set_phi first");
  out[0] = out[1] = out[2] = 0;
  HIP_TRY(h, hipMemsetAsync(h->d_vs_zero, 0, sizeof(unsigned long long), h->stream));
  hipLaunchKernelGGL(vs_zero_cells_kernel, dim3(grid_for((int64_t)h->K * h->V, 256, 4)), dim3(256), 0, h->stream, h->d_phiT, h->K, h->Kp, h->V, h->d_vs_zero);
  HIP_TRY(h, hipGetLastError());
  unsigned long long zero = 0;
  if ((rc = copy_out(h, &zero, h->d_vs_zero, sizeof zero))) return rc;
  out[1] = (int64_t)zero;
  if (!h->vs_drawn) return GGS_OK;                     // no variable-selection draw yet: nothing undrawn, no rounds
  std::vector<uint32_t> und((size_t)h->V * h->vs_pitch);    // the by-word mask: every topic's cells, with an exchange too
  std::vector<int32_t> rounds((size_t)h->Ks);               // the chains this handle ran: its own topics
  if ((rc = copy_out(h, und.data(), h->d_vs_mask, und.size() * sizeof(uint32_t))) || (rc = copy_out(h, rounds.data(), h->d_vs_rounds, rounds.size() * sizeof(int32_t))))
    return rc;
  for (uint32_t w : und) out[0] += __builtin_popcount(w);
  for (int32_t r : rounds) out[2] = std::max<int64_t>(out[2], r);
  return GGS_OK;
}
int ggs_get_phi_mean(ggs_handle *h, double *phi_mean, int32_t *n_sampled) {
  if (!h || !n_sampled) return GGS_ERR_BAD_ARG;
  *n_sampled = h->n_sampled_phi;
  if (h->n_sampled_phi == 0 || !h->d_phi_mean) return GGS_OK;   // Java returns null (UPLDA:1955-1958)
  if (!phi_mean) return GGS_ERR_BAD_ARG;
  int rc = bind_device(h);
  if (rc) return rc;
  return phi_out(h, h->d_phi_mean, h->K, phi_mean, (double)h->n_sampled_phi);
}
int ggs_get_theta(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *theta) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (doc_begin < 0 || doc_end > h->D || doc_begin > doc_end || (!theta && doc_end > doc_begin)) return set_err(h, GGS_ERR_BAD_ARG, "bad document range");
  if (counts_only(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightcollapsed and scheme=adlda keep no theta");
  if (no_theta(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=lightpcldaw2 keeps no theta");
  return copy_out(h, theta, h->d_theta + (size_t)doc_begin * h->K, sizeof(double) * (size_t)(doc_end - doc_begin) * h->K);
}
int ggs_get_doc_topic_counts(ggs_handle *h, int64_t doc_begin, int64_t doc_end, int32_t *n_dk) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (doc_begin < 0 || doc_end > h->D || doc_begin > doc_end || (!n_dk && doc_end > doc_begin)) return set_err(h, GGS_ERR_BAD_ARG, "bad document range");
  const int64_t nd = doc_end - doc_begin;
  if (nd == 0) return GGS_OK;
  const size_t bytes = (size_t)nd * h->K * sizeof(int32_t);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  hipLaunchKernelGGL(doc_topic_kernel, dim3((unsigned)nd), dim3(64), 0, h->stream, h->d_doc_ptr, h->d_z, doc_begin, h->K, static_cast<int32_t *>(h->d_scratch));
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, n_dk, h->d_scratch, bytes);
}
// the diagnostics' theta of a scheme that keeps none (lightpcldaw2): allocated when the log posterior or the document distances first draw one
static int ensure_diag_theta(ggs_handle *h) {
  if (h->d_theta) return GGS_OK;
  const int rc = dev_alloc(h, &h->d_theta, (size_t)h->D * h->K + 2);
  if (rc) return rc;
  HIP_TRY(h, hipMemset(h->d_theta, 0, sizeof(double) * ((size_t)h->D * h->K + 2)));
  return GGS_OK;
}
// ll_docs_kernel and lp_docs_kernel keep four K-long histograms per block in LDS (ggs_loglik.hpp)
static int ll_check_topics(ggs_handle *h) {
  if (h->K > kLLMaxTopics)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the model log likelihood and the log posterior keep four documents' topic counts in LDS: at most " +
                                               std::to_string(kLLMaxTopics) + " topics fit its 160 KiB, this model has " + std::to_string(h->K));
  return GGS_OK;
}
int ggs_model_log_likelihood(ggs_handle *h, double *doc_side, double *topic_side) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!doc_side || !topic_side) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = launch_magnitude(h))) return rc;       // corpus-wide counts gathered, tokensPerTopic in step with them
  const int K = h->K;
  if ((rc = ll_check_topics(h))) return rc;
  const int64_t doc_blocks = (h->D + kLLBlock / 64 - 1) / (kLLBlock / 64), type_blocks = 1024;
  const size_t bytes = 32 + sizeof(double) * (size_t)(doc_blocks + type_blocks);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_out = static_cast<double *>(h->d_scratch);                       // [0] document side, [1] topic side
  auto *d_nz = reinterpret_cast<unsigned long long *>(d_out + 2);
  double *d_doc = d_out + 4, *d_type = d_doc + doc_blocks;
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, 32, h->stream));
  double alpha_sum = 0;
  for (int k = 0; k < K; ++k) alpha_sum += h->alpha[k];
  if (doc_blocks)
    hipLaunchKernelGGL(ll_docs_kernel, dim3((unsigned)doc_blocks), dim3(kLLBlock), ll_docs_lds_bytes(K), h->stream, h->d_doc_ptr,
                       h->d_z, h->d_alpha, alpha_sum, h->D, K, d_doc);
  hipLaunchKernelGGL(ll_types_kernel, dim3((unsigned)type_blocks), dim3(kLLBlock), 0, h->stream, h->d_n_wk, (int64_t)K * h->V, h->beta, d_type, d_nz);
  hipLaunchKernelGGL(ll_finish_kernel, dim3(1), dim3(kLLBlock), 0, h->stream, d_doc, doc_blocks, d_type, type_blocks, h->d_n_k, K, h->beta * h->V,
                     alpha_sum, h->beta, h->D, d_nz, d_out);
  HIP_TRY(h, hipGetLastError());
  double out[2];
  if ((rc = copy_out(h, out, d_out, sizeof out))) return rc;
  *doc_side = out[0]; *topic_side = out[1];
  return GGS_OK;
}
int ggs_log_posterior(ggs_handle *h, double *doc_side, double *topic_side) {
  int rc = require_ready(h, true);
  if (rc) return rc;
  if (!doc_side || !topic_side) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if (count_form(h->scheme)) return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed and scheme=lightcollapsed have no Phi: the log posterior of UPLDA:1573-1634 does not apply");
  if ((rc = ll_check_topics(h))) return rc;
  if (pcgs_family(h->scheme)) {
    // UPLDA:710-714: every scheme but ggs draws theta_d ~ Dir(n_d. + alpha) afresh for the diagnostics
    // (LDAUtils.drawDirichlets); here: the theta draw of GGS:57-72 under the stream GGS_PURPOSE_THETA at the current iteration
    if ((rc = drop_theta_ahead(h)) || (rc = ensure_diag_theta(h)) || (rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  const int K = h->K;
  const int64_t doc_blocks = (h->D + kLLBlock / 64 - 1) / (kLLBlock / 64), phi_blocks = 1024;
  const size_t bytes = 32 + sizeof(double) * (size_t)(doc_blocks + phi_blocks);
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_out = static_cast<double *>(h->d_scratch);
  double *d_doc = d_out + 4, *d_phi = d_doc + doc_blocks;
  if (doc_blocks)
    hipLaunchKernelGGL(lp_docs_kernel, dim3((unsigned)doc_blocks), dim3(kLLBlock), ll_docs_lds_bytes(K), h->stream, h->d_doc_ptr,
                       h->d_tok, h->d_z, h->d_alpha, h->d_theta, h->d_phiT, h->D, K, h->Kp, d_doc);
  hipLaunchKernelGGL(lp_phi_kernel, dim3((unsigned)phi_blocks), dim3(kLLBlock), 0, h->stream, h->d_phiT, (int64_t)h->V, K, h->Kp, d_phi);
  hipLaunchKernelGGL(lp_finish_kernel, dim3(1), dim3(kLLBlock), 0, h->stream, d_doc, doc_blocks, d_phi, phi_blocks, h->beta, d_out);
  HIP_TRY(h, hipGetLastError());
  double out[2];
  if ((rc = copy_out(h, out, d_out, sizeof out))) return rc;
  *doc_side = out[0]; *topic_side = out[1];
  return GGS_OK;
}
// ---- min document / topic distances (csrc/ggs_distances.hpp) ---------------------------------------------------------------
namespace {
// One launch covers at most 2^30 tiles (GGS_DEBUG_DIST_BAND_TILES: fewer): bands of whole tile rows.
constexpr int64_t kDistBandTiles = (int64_t)1 << 30;
int64_t dist_band_rows(int64_t tiles_b) {
  return std::max<int64_t>(1, debug_shrunk("GGS_DEBUG_DIST_BAND_TILES", kDistBandTiles) / std::max<int64_t>(tiles_b, 1));
}
// min_bits[n] (preset by the caller) <- the minimal sums of the rows of A [n][len] over the rows of B [m][len]; B == A with diag
void launch_min_row_dist(hipStream_t st, const double *A, int64_t n, const double *B, int64_t m, int64_t len, bool diag, unsigned long long *min_bits) {
  if (n <= 0 || m <= 0) return;
  constexpr int T = dist_tile_edge(kDistRowR);
  const int64_t ta = (n + T - 1) / T, tb = (m + T - 1) / T, band = dist_band_rows(tb);
  for (int64_t t0 = 0; t0 < ta; t0 += band)
    hipLaunchKernelGGL(min_row_dist_kernel, dim3((unsigned)(std::min(band, ta - t0) * tb)), dim3(kDistBlock), 0, st, A, n, B, m, len, diag ? 1 : 0, t0 * tb, tb, min_bits);
}
// the same for the columns of A [len][pitch] against each other
void launch_min_topic_dist(hipStream_t st, const double *A, int64_t n, int64_t pitch, int64_t len, unsigned long long *min_bits) {
  if (n <= 1) return;
  constexpr int T = dist_tile_edge(kDistTopR);
  const int64_t ta = (n + T - 1) / T, band = dist_band_rows(ta);
  for (int64_t t0 = 0; t0 < ta; t0 += band)
    hipLaunchKernelGGL(min_topic_dist_kernel, dim3((unsigned)(std::min(band, ta - t0) * ta)), dim3(kDistBlock), 0, st, A, n, pitch, len, t0 * ta, ta, min_bits);
}
constexpr size_t kDistPieceBytes = (size_t)64 << 20;   // a foreign block travels to scratch in pieces of at most this
size_t dist_piece_bytes() { return (size_t)debug_shrunk("GGS_DEBUG_DIST_PIECE_BYTES", (int64_t)kDistPieceBytes); }   // tests: several pieces
}  // namespace

int ggs_min_doc_distances(ggs_handle *h, const double *other, int64_t n_other, double *min_dist) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme))
    return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, lightcollapsed and adlda draw no theta: the document distances of UPLDA:723-753 do not apply");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  const int64_t D = h->D, K = h->K;
  if (n_other < 0 || (!other && n_other != 0) || (!min_dist && D > 0)) return set_err(h, GGS_ERR_BAD_ARG, "null output or negative size");
  if (D == 0) return GGS_OK;
  if (pcgs_family(h->scheme)) {
    // UPLDA:710-714: one fresh theta per diagnostic iteration for the distances and the log posterior together; here both
    // calls redraw the same bits (the stream GGS_PURPOSE_THETA at the current iteration), as ggs_log_posterior does
    if ((rc = drop_theta_ahead(h)) || (rc = ensure_diag_theta(h)) || (rc = launch_theta(h, h->stream, h->d_theta, h->iteration))) return rc;
  }
  const int64_t piece_rows = other ? std::max<int64_t>(1, std::min<int64_t>(n_other, (int64_t)(dist_piece_bytes() / (sizeof(double) * (size_t)K)))) : 0;
  const size_t head = sizeof(double) * 2 * (size_t)D;     // [D] minimal sums as bit patterns, [D] distances
  if ((rc = ensure_scratch(h, head + sizeof(double) * (size_t)piece_rows * (size_t)K))) return rc;
  auto *d_bits = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_out = reinterpret_cast<double *>(d_bits + D);
  double *d_piece = d_out + D;
  const int grid = grid_for(D, 256);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid), dim3(256), 0, h->stream, d_bits, D);
  if (!other) launch_min_row_dist(h->stream, h->d_theta, D, h->d_theta, D, K, true, d_bits);
  for (int64_t r0 = 0; other && r0 < n_other; r0 += piece_rows) {
    const int64_t rows = std::min(piece_rows, n_other - r0);
    HIP_TRY(h, hipMemcpyAsync(d_piece, other + r0 * K, sizeof(double) * (size_t)rows * (size_t)K, hipMemcpyHostToDevice, h->stream));
    launch_min_row_dist(h->stream, h->d_theta, D, d_piece, rows, K, false, d_bits);
    if (r0 + piece_rows < n_other) HIP_TRY(h, hipStreamSynchronize(h->stream));   // the piece is overwritten next
  }
  hipLaunchKernelGGL(min_dist_finish_kernel, dim3(grid), dim3(256), 0, h->stream, d_bits, D, d_out, static_cast<double *>(nullptr));
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, min_dist, d_out, sizeof(double) * (size_t)D);
}

int ggs_min_topic_distance(ggs_handle *h, double *min_dist) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (count_form(h->scheme))
    return set_err(h, GGS_ERR_UNSUPPORTED, "scheme=collapsed, lightcollapsed and adlda draw no Phi: the topic distances of UPLDA:778-806 do not apply");
  if (!h->have_phi) return set_err(h, GGS_ERR_STATE, "no Phi: call ggs_init_phi / ggs_set_z / ggs_set_phi first");
  if (!min_dist) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  const int64_t K = h->K;
  if ((rc = ensure_scratch(h, sizeof(double) * ((size_t)K + 1)))) return rc;
  auto *d_bits = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_out = reinterpret_cast<double *>(d_bits + K);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid_for(K, 256)), dim3(256), 0, h->stream, d_bits, K);
  launch_min_topic_dist(h->stream, h->d_phiT, K, h->Kp, h->V, d_bits);
  hipLaunchKernelGGL(min_dist_reduce_kernel, dim3(1), dim3(kDistBlock), 0, h->stream, d_bits, K, d_out);
  HIP_TRY(h, hipGetLastError());
  return copy_out(h, min_dist, d_out, sizeof(double));
}
// ---- top words per topic (csrc/ggs_topic_summaries.hpp) --------------------------------------------------------------------
namespace {
// the device work space of one call, carved from one allocation
struct TsPlan {
  int32_t V = 0, K = 0, n = 0, nseg = 0, sum_nseg = 0, tot_nseg = 0;
  size_t mass = 0, total = 0, rowsum = 0, k1mass = 0, pw = 0, logpw = 0, guess = 0, fn = 0, tguess = 0, tfn = 0, cand_s = 0, cand_i = 0, idx = 0, score = 0, bytes = 0;
  TsPlan(int32_t V, int32_t K, int32_t n);
};
TsPlan::TsPlan(int32_t V, int32_t K, int32_t n) {
  TsPlan &q = *this;
  q.V = V; q.K = K; q.n = n;
  q.nseg = (V + kTsSegWords - 1) / kTsSegWords;
  q.sum_nseg = (V + kSumSegRows - 1) / kSumSegRows;
  q.tot_nseg = (int32_t)(((int64_t)V * K + kSumSegRows - 1) / kSumSegRows);
  size_t at = 0;
  auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
  q.mass = take(8 * (size_t)K); q.total = take(8);
  q.rowsum = take(8 * (size_t)V); q.k1mass = take(8 * (size_t)V); q.pw = take(8 * (size_t)V); q.logpw = take(8 * (size_t)V);
  q.guess = take(8 * ((size_t)q.sum_nseg + 1) * K); q.fn = take(32 * (size_t)q.sum_nseg * K);
  q.tguess = take(8 * ((size_t)q.tot_nseg + 1)); q.tfn = take(32 * (size_t)q.tot_nseg);
  q.cand_s = take(8 * (size_t)q.nseg * n * K); q.cand_i = take(4 * (size_t)q.nseg * n * K);
  q.idx = take(4 * (size_t)K * n); q.score = take(8 * (size_t)K * n);
  q.bytes = at;
}
int ts_check_args(ggs_handle *h, int32_t V, int32_t K, double beta, int32_t kind, int32_t n, double lambda, const int32_t *idx) {
  if (!idx) return set_err(h, GGS_ERR_BAD_ARG, "null idx");
  if (kind < 0 || kind >= kTsKinds) return set_err(h, GGS_ERR_BAD_ARG, "unknown kind: 0 top, 1 relevance, 2 distinctive, 3 salient, 4 k1");
  if (n < 1 || n > V) return set_err(h, GGS_ERR_BAD_ARG, "Asked for more words (" + std::to_string(n) + ") than there are types (unique words = noTypes = " + std::to_string(V) + ").");
  if (!std::isfinite(lambda)) return set_err(h, GGS_ERR_BAD_ARG, "lambda must be finite");
  if (kind != kTsTop && !(beta > 0.0)) return set_err(h, GGS_ERR_BAD_ARG, "beta must be positive for the probability rankings (the scores of empty cells are NaN otherwise)");
  if (n > kTsMaxWords) return set_err(h, GGS_ERR_UNSUPPORTED, "at most " + std::to_string(kTsMaxWords) + " words per topic");
  if ((int64_t)V * K > ((int64_t)1 << 31) - 256 || (V + kTsSegWords - 1) / kTsSegWords > 16000)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the topic summaries index the V * K cells with 32 bits and keep V / 256 list heads in LDS");
  return GGS_OK;
}
// cnt [V][K] on the device -> idx / score in the work space; norms: the normalisers and the words' statistics whatever the kind
// ev (or NULL): five events recorded around mass_k | total | the words' statistics | selection and merge
void ts_launch(hipStream_t st, bool exact_sum, const int32_t *cnt, double beta, double lambda, int32_t kind, const TsPlan &q, char *work, bool norms, double *all_scores,
               hipEvent_t *ev = nullptr) {
  auto mark = [&](int i) { if (ev) (void)hipEventRecord(ev[i], st); };
  auto D = [&](size_t o) { return reinterpret_cast<double *>(work + o); };
  TsParams p{};
  p.cnt = cnt; p.mass = D(q.mass); p.total = D(q.total); p.rowsum = D(q.rowsum); p.k1mass = D(q.k1mass); p.pw = D(q.pw); p.logpw = D(q.logpw);
  p.cand_score = D(q.cand_s); p.cand_id = reinterpret_cast<int32_t *>(work + q.cand_i); p.idx = reinterpret_cast<int32_t *>(work + q.idx); p.score = D(q.score);
  p.all_scores = all_scores; p.beta = beta; p.lambda = lambda; p.one_minus_lambda = 1 - lambda;
  p.pitch = q.K; p.V = q.V; p.K = q.K; p.kind = kind; p.n = q.n; p.nseg = q.nseg;
  if (norms || kind != kTsTop) {
    // mass_k: the Dirichlet magnitude sum; total: the same sum over the one column of the V * K cells flattened.  Unguided, in
    // work space of their own: the handle's running sums (the Phi phase's guess) are neither read nor written.
    ggs_handle col;
    col.K = q.K; col.V = q.V; col.beta = beta; col.stream = st; col.exact_sum = exact_sum; col.sum_nseg = q.sum_nseg;
    mark(0);
    launch_column_sum<int32_t, true>(&col, cnt, q.K, q.K, D(q.mass), nullptr, false, false, D(q.guess), D(q.fn));
    mark(1);
    col.K = 1; col.V = (int32_t)((int64_t)q.V * q.K); col.sum_nseg = q.tot_nseg;
    launch_column_sum<int32_t, true>(&col, cnt, 1, 1, D(q.total), nullptr, false, false, D(q.tguess), D(q.tfn));
    mark(2);
    hipLaunchKernelGGL(ts_words_kernel, dim3((unsigned)((q.V + 63) / 64)), dim3(64), 0, st, p);
  } else {
    mark(0); mark(1); mark(2);
  }
  mark(3);
  if (all_scores) hipLaunchKernelGGL(ts_scores_kernel, dim3((unsigned)((q.K + 255) / 256), (unsigned)std::min(q.V, 4096)), dim3(256), 0, st, p);
  const dim3 grid((unsigned)q.nseg, (unsigned)((q.K + kTsTopics - 1) / kTsTopics));
  if (q.n <= kTsLdsWords) hipLaunchKernelGGL(ts_select_kernel<true>, grid, dim3(64), (size_t)q.n * 64 * 12, st, p);
  else hipLaunchKernelGGL(ts_select_kernel<false>, grid, dim3(64), 0, st, p);
  hipLaunchKernelGGL(ts_merge_kernel, dim3((unsigned)q.K), dim3(64), sizeof(int32_t) * (size_t)q.nseg, st, p);
  mark(4);
}
}  // namespace

int ggs_top_words(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t *idx, double *score) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if ((rc = ts_check_args(h, h->V, h->K, h->beta, kind, n_words, lambda, idx))) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  const TsPlan q(h->V, h->K, n_words);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  ts_launch(h->stream, h->exact_sum, h->d_n_wk, h->beta, lambda, kind, q, work, false, nullptr);
  HIP_TRY(h, hipGetLastError());
  if ((rc = copy_out(h, idx, work + q.idx, sizeof(int32_t) * (size_t)h->K * n_words))) return rc;
  return score ? copy_out(h, score, work + q.score, sizeof(double) * (size_t)h->K * n_words) : GGS_OK;
}
int ggs_debug_top_words_phases(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t element_chain, double *ms) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  int32_t dummy = 0;
  if (!ms) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = ts_check_args(h, h->V, h->K, h->beta, kind, n_words, lambda, &dummy))) return rc;
  if ((rc = ensure_global_counts(h))) return rc;
  const TsPlan q(h->V, h->K, n_words);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  hipEvent_t ev[5] = {};
  for (auto &e : ev) HIP_TRY(h, hipEventCreate(&e));
  ts_launch(h->stream, element_chain ? false : h->exact_sum, h->d_n_wk, h->beta, lambda, kind, q, static_cast<char *>(h->d_scratch), false, nullptr, ev);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(h->stream);
  for (int i = 0; i < 4 && err == hipSuccess; ++i) { float f = 0; err = hipEventElapsedTime(&f, ev[i], ev[i + 1]); ms[i] = f; }
  for (auto &e : ev) (void)hipEventDestroy(e);
  HIP_TRY(h, err);
  return GGS_OK;
}
// ---- topic diagnostics (csrc/ggs_topic_diagnostics.hpp) ---------------------------------------------------------------------
namespace {
constexpr size_t kTdPieceBytes = (size_t)64 << 20;     // the dense rows of a piece of documents / the sort buffers of a group of topics
// what both planners below size by, wherever they are constructed (a handle's call or its ggs_debug_* twin)
size_t td_piece_bytes() { return (size_t)debug_shrunk("GGS_DEBUG_TD_PIECE_BYTES", (int64_t)kTdPieceBytes); }   // tests: several pieces / groups
// events between the phases of a call (ggs_debug_topic_diagnostics_phases); without it, nothing is recorded
struct TdTimer {
  hipStream_t st;
  std::vector<std::pair<int, hipEvent_t>> marks;       // (phase that ends here, or -1 for a start; event)
  void mark(int phase) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return;
    (void)hipEventRecord(e, st);
    marks.emplace_back(phase, e);
  }
  // after a synchronize: adds every span to ms[phase]
  void collect(double *ms) {
    for (size_t i = 1; i < marks.size(); ++i) {
      float f = 0;
      if (marks[i].first >= 0 && hipEventElapsedTime(&f, marks[i - 1].second, marks[i].second) == hipSuccess) ms[marks[i].first] += f;
    }
  }
  ~TdTimer() { for (auto &m : marks) (void)hipEventDestroy(m.second); }
};
inline void td_mark(TdTimer *t, int phase) { if (t) t->mark(phase); }
enum { kTdPhMembership = 0, kTdPhDocs = 1, kTdPhColumns = 2, kTdPhChain = 3, kTdPhTotals = 4, kTdPhSorted = 5, kTdPhSmall = 6, kTdPhases = 7 };

int td_check_args(ggs_handle *h, int32_t V, int32_t K, int32_t n, const int32_t *idx) {
  if (n < 1 || n > V) return set_err(h, GGS_ERR_BAD_ARG, "Asked for more words (" + std::to_string(n) + ") than there are types (unique words = noTypes = " + std::to_string(V) + ").");
  if (n > kTdMaxWords) return set_err(h, GGS_ERR_UNSUPPORTED, "at most " + std::to_string(kTdMaxWords) + " words per topic");
  if (idx)
    for (size_t i = 0; i < (size_t)K * n; ++i)
      if (idx[i] < 0 || idx[i] >= V) return set_err(h, GGS_ERR_BAD_ARG, "idx holds a word id outside [0, V)");
  return GGS_OK;
}
int td_check_topics(ggs_handle *h, int32_t K) {
  if (K > kTdMaxTopics)
    return set_err(h, GGS_ERR_UNSUPPORTED, "the topic diagnostics keep a document's topic counts and top-word masks in LDS (20 bytes per topic): at most " +
                                               std::to_string(kTdMaxTopics) + " topics fit 60 KiB, this model has " + std::to_string(K));
  return GGS_OK;
}

// the device work space of ggs_topic_doc_statistics
struct TdDocPlan {
  int64_t D = 0, piece = 0;
  int32_t V = 0, K = 0, n = 0;
  size_t mem_ptr = 0, mem = 0, codoc = 0, stats = 0, clogc = 0, maxtopic = 0, crow = 0, addend = 0, bytes = 0;
  TdDocPlan(int64_t D_, int32_t V_, int32_t K_, int32_t n_) : D(D_), V(V_), K(K_), n(n_) {
    // a piece's dense rows (4 + 8 bytes per cell) stay within kTdPieceBytes, but hold at least one wave's 256 documents
    piece = (int64_t)(td_piece_bytes() / (12 * (size_t)K)) / kTdSegDocs * kTdSegDocs;
    piece = std::max<int64_t>(piece, kTdSegDocs);
    piece = std::min<int64_t>(piece, std::max<int64_t>(D, 1));
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
    mem_ptr = take(4 * ((size_t)V + 1)); mem = take(4 * (size_t)K * n); codoc = take(4 * (size_t)K * n * n); stats = take(4 * (size_t)K * kTdStats);
    clogc = take(8 * (size_t)K); maxtopic = take(4 * (size_t)piece); crow = take(4 * (size_t)piece * K); addend = take(8 * (size_t)piece * K);
    bytes = at;
  }
};
// idx [K][n] (host) -> the CSR by word of the (topic, position) pairs
void td_membership(const int32_t *idx, int32_t V, int32_t K, int32_t n, std::vector<int32_t> &ptr, std::vector<int32_t> &mem) {
  ptr.assign((size_t)V + 1, 0);
  mem.assign((size_t)K * n, 0);
  for (size_t i = 0; i < (size_t)K * n; ++i) ptr[(size_t)idx[i] + 1] += 1;
  for (int32_t w = 0; w < V; ++w) ptr[(size_t)w + 1] += ptr[w];
  std::vector<int32_t> cur(ptr.begin(), ptr.end() - 1);
  for (int32_t k = 0; k < K; ++k)
    for (int32_t r = 0; r < n; ++r) mem[(size_t)cur[idx[(size_t)k * n + r]]++] = k * 128 + r;
}
// Enqueues the whole document pass; the results are left in work (q.codoc, q.stats, q.clogc).  The uploads are synchronous.
hipError_t td_doc_launch(hipStream_t st, const TdDocPlan &q, char *work, const int64_t *d_doc_ptr, const int32_t *d_tok, const int32_t *d_z, const double *d_alpha,
                         double alpha_sum, const int32_t *idx, const double *clogc_in, TdTimer *tm) {
  td_mark(tm, -1);
  std::vector<int32_t> ptr, mem;
  td_membership(idx, q.V, q.K, q.n, ptr, mem);
  hipError_t e;
  if ((e = hipMemcpyAsync(work + q.mem_ptr, ptr.data(), 4 * ptr.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.mem, mem.data(), 4 * mem.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(work + q.codoc, 0, q.stats + 4 * (size_t)q.K * kTdStats - q.codoc, st)) != hipSuccess) return e;
  if (clogc_in) e = hipMemcpyAsync(work + q.clogc, clogc_in, 8 * (size_t)q.K, hipMemcpyHostToDevice, st);
  else e = hipMemsetAsync(work + q.clogc, 0, 8 * (size_t)q.K, st);
  if (e != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;           // ptr / mem / clogc_in are pageable host memory
  td_mark(tm, kTdPhMembership);
  TdDocParams p{};
  p.doc_ptr = d_doc_ptr; p.tok = d_tok; p.z = d_z;
  p.mem_ptr = reinterpret_cast<int32_t *>(work + q.mem_ptr); p.mem = reinterpret_cast<int32_t *>(work + q.mem);
  p.crow = reinterpret_cast<int32_t *>(work + q.crow); p.maxtopic = reinterpret_cast<int32_t *>(work + q.maxtopic);
  p.codoc = reinterpret_cast<int32_t *>(work + q.codoc); p.alpha = d_alpha; p.alpha_sum = alpha_sum;
  p.addend = reinterpret_cast<double *>(work + q.addend); p.doc_stats = reinterpret_cast<int32_t *>(work + q.stats);
  p.K = q.K; p.n = q.n;
  double *clogc = reinterpret_cast<double *>(work + q.clogc);
  const unsigned kblocks = (unsigned)((q.K + 63) / 64);
  for (int64_t d0 = 0; d0 < q.D; d0 += q.piece) {
    p.d0 = d0; p.nd = std::min<int64_t>(q.piece, q.D - d0);
    hipLaunchKernelGGL(td_docs_kernel, dim3((unsigned)std::min<int64_t>(p.nd, 4096)), dim3(64), (size_t)kTdLdsPerTopic * q.K, st, p);
    td_mark(tm, kTdPhDocs);
    hipLaunchKernelGGL(td_columns_kernel, dim3(kblocks, (unsigned)((p.nd + kTdSegDocs - 1) / kTdSegDocs)), dim3(64), 0, st, p);
    td_mark(tm, kTdPhColumns);
    hipLaunchKernelGGL(td_clogc_kernel, dim3(kblocks), dim3(64), 0, st, p.addend, p.nd, q.K, clogc);
    td_mark(tm, kTdPhChain);
  }
  hipLaunchKernelGGL(td_mirror_kernel, dim3((unsigned)grid_for((int64_t)q.K * q.n * q.n, 256)), dim3(256), 0, st, p.codoc, q.K, q.n);
  td_mark(tm, kTdPhDocs);
  return hipGetLastError();
}

// the device work space of ggs_topic_scores
struct TdScorePlan {
  int32_t V = 0, K = 0, n = 0, group = 0;
  size_t n_k = 0, wtc = 0, idx = 0, codoc = 0, stats = 0, clogc = 0, head = 0, ts = 0, ws = 0, key_a = 0, id_a = 0, key_b = 0, id_b = 0, bytes = 0;
  TdScorePlan(int32_t V_, int32_t K_, int32_t n_) : V(V_), K(K_), n(n_) {
    group = (int32_t)std::min<size_t>((size_t)K, std::max<size_t>(1, td_piece_bytes() / (16 * (size_t)V)));   // the sort's four [group][V] buffers within kTdPieceBytes
    size_t at = 0;
    auto take = [&](size_t b) { const size_t o = at; at += (b + 255) & ~(size_t)255; return o; };
    n_k = take(4 * (size_t)K); wtc = take(4 * (size_t)V); idx = take(4 * (size_t)K * n); codoc = take(4 * (size_t)K * n * n); stats = take(4 * (size_t)K * kTdStats);
    clogc = take(8 * (size_t)K); head = take(4 * (size_t)K * n); ts = take(8 * (size_t)kTdScoreRows * K); ws = take(8 * (size_t)kTdWordRows * K * n);
    const size_t buf = 4 * (size_t)group * V;
    key_a = take(buf); id_a = take(buf); key_b = take(buf); id_b = take(buf);
    bytes = at;
  }
};
hipError_t td_score_launch(hipStream_t st, const TdScorePlan &q, char *work, const int32_t *d_cnt, int32_t pitch, double beta, const int32_t *idx, const int32_t *codoc,
                           const int32_t *doc_stats, const double *clogc, bool words, TdTimer *tm) {
  hipError_t e;
  td_mark(tm, -1);
  if ((e = hipMemcpyAsync(work + q.idx, idx, 4 * (size_t)q.K * q.n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.codoc, codoc, 4 * (size_t)q.K * q.n * q.n, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.stats, doc_stats, 4 * (size_t)q.K * kTdStats, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(work + q.clogc, clogc, 8 * (size_t)q.K, hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(work + q.n_k, 0, 4 * (size_t)q.K, st)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
  td_mark(tm, -1);
  auto I = [&](size_t o) { return reinterpret_cast<int32_t *>(work + o); };
  TdScoreParams p{};
  p.cnt = d_cnt; p.n_k = I(q.n_k); p.wtc = I(q.wtc); p.idx = I(q.idx); p.codoc = I(q.codoc); p.doc_stats = I(q.stats);
  p.clogc = reinterpret_cast<double *>(work + q.clogc); p.key_a = I(q.key_a); p.id_a = I(q.id_a); p.key_b = I(q.key_b); p.id_b = I(q.id_b);
  p.sorted_head = I(q.head); p.topic_scores = reinterpret_cast<double *>(work + q.ts); p.word_scores = words ? reinterpret_cast<double *>(work + q.ws) : nullptr;
  p.beta = beta; p.pitch = pitch; p.V = q.V; p.K = q.K; p.n = q.n;
  hipLaunchKernelGGL(td_nk_kernel, dim3((unsigned)((q.K + 63) / 64), (unsigned)std::min(q.V, 256)), dim3(64), 0, st, p);
  hipLaunchKernelGGL(td_wtc_kernel, dim3((unsigned)std::min(q.V, 8192)), dim3(64), 0, st, p);
  td_mark(tm, kTdPhTotals);
  for (int32_t k0 = 0; k0 < q.K; k0 += q.group) {
    p.k0 = k0;
    hipLaunchKernelGGL(td_sorted_kernel, dim3((unsigned)std::min(q.group, q.K - k0)), dim3(64), 0, st, p);
  }
  td_mark(tm, kTdPhSorted);
  hipLaunchKernelGGL(td_small_kernel, dim3((unsigned)q.K), dim3(64), 0, st, p);
  td_mark(tm, kTdPhSmall);
  return hipGetLastError();
}
double td_alpha_sum(const double *alpha, int32_t K) {
  double s = 0;
  for (int32_t k = 0; k < K; ++k) s += alpha[k];
  return s;
}
// idx, or the handle's own top words into own
int td_resolve_idx(ggs_handle *h, int32_t n, const int32_t *&idx, std::vector<int32_t> &own) {
  int rc = td_check_args(h, h->V, h->K, n, idx);
  if (rc || idx) return rc;
  own.resize((size_t)h->K * n);
  if ((rc = ggs_top_words(h, GGS_TOP_WORDS, n, 0.0, own.data(), nullptr))) return rc;
  idx = own.data();
  return GGS_OK;
}
int td_doc_statistics(ggs_handle *h, int32_t n, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats, double *clogc_out, TdTimer *tm) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!codoc || !doc_stats || !clogc_out) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  std::vector<int32_t> own;
  if ((rc = td_resolve_idx(h, n, idx, own)) || (rc = td_check_topics(h, h->K))) return rc;
  const TdDocPlan q(h->D, h->V, h->K, n);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  HIP_TRY(h, td_doc_launch(h->stream, q, work, h->d_doc_ptr, h->d_tok, h->d_z, h->d_alpha, td_alpha_sum(h->alpha.data(), h->K), idx, clogc_in, tm));
  if ((rc = copy_out(h, codoc, work + q.codoc, 4 * (size_t)h->K * n * n)) || (rc = copy_out(h, doc_stats, work + q.stats, 4 * (size_t)h->K * kTdStats))) return rc;
  return copy_out(h, clogc_out, work + q.clogc, 8 * (size_t)h->K);
}
int td_scores(ggs_handle *h, int32_t n, const int32_t *idx, const int32_t *codoc, const int32_t *doc_stats, const double *clogc, double *topic_scores,
              double *word_scores, TdTimer *tm) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!codoc || !doc_stats || !clogc || !topic_scores) return set_err(h, GGS_ERR_BAD_ARG, "null argument");
  std::vector<int32_t> own;
  if ((rc = td_resolve_idx(h, n, idx, own)) || (rc = ensure_global_counts(h))) return rc;
  const TdScorePlan q(h->V, h->K, n);
  if ((rc = ensure_scratch(h, q.bytes))) return rc;
  char *work = static_cast<char *>(h->d_scratch);
  HIP_TRY(h, td_score_launch(h->stream, q, work, h->d_n_wk, h->K, h->beta, idx, codoc, doc_stats, clogc, word_scores != nullptr, tm));
  if ((rc = copy_out(h, topic_scores, work + q.ts, 8 * (size_t)kTdScoreRows * h->K))) return rc;
  return word_scores ? copy_out(h, word_scores, work + q.ws, 8 * (size_t)kTdWordRows * h->K * n) : GGS_OK;
}
}  // namespace

int ggs_topic_doc_statistics(ggs_handle *h, int32_t n_words, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats, double *clogc_out) {
  return td_doc_statistics(h, n_words, idx, clogc_in, codoc, doc_stats, clogc_out, nullptr);
}
int ggs_topic_scores(ggs_handle *h, int32_t n_words, const int32_t *idx, const int32_t *codoc, const int32_t *doc_stats, const double *clogc, double *topic_scores,
                     double *word_scores) {
  return td_scores(h, n_words, idx, codoc, doc_stats, clogc, topic_scores, word_scores, nullptr);
}
int ggs_debug_topic_diagnostics_phases(ggs_handle *h, int32_t n_words, double *ms) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!ms) return set_err(h, GGS_ERR_BAD_ARG, "null output");
  if ((rc = td_check_args(h, h->V, h->K, n_words, nullptr))) return rc;
  const size_t K = (size_t)h->K, n = (size_t)n_words;
  std::vector<int32_t> idx(K * n), codoc(K * n * n), stats(K * kTdStats);
  std::vector<double> clogc(K), ts(kTdScoreRows * K);
  if ((rc = ggs_top_words(h, GGS_TOP_WORDS, n_words, 0.0, idx.data(), nullptr))) return rc;
  for (int i = 0; i < kTdPhases; ++i) ms[i] = 0;
  {
    TdTimer tm{h->stream, {}};
    if ((rc = td_doc_statistics(h, n_words, idx.data(), nullptr, codoc.data(), stats.data(), clogc.data(), &tm))) return rc;
    tm.collect(ms);
  }
  TdTimer tm{h->stream, {}};
  if ((rc = td_scores(h, n_words, idx.data(), codoc.data(), stats.data(), clogc.data(), ts.data(), nullptr, &tm))) return rc;
  tm.collect(ms);
  return GGS_OK;
}
int ggs_set_test_corpus(ggs_handle *h, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, int64_t doc_base) {
  if (!h || D < 0 || !doc_ptr || doc_base < 0) return set_err(h, GGS_ERR_BAD_ARG, "bad test corpus arguments");
  if (doc_ptr[0] != 0) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr[0] must be 0");
  for (int64_t d = 0; d < D; ++d) {
    if (doc_ptr[d + 1] < doc_ptr[d]) return set_err(h, GGS_ERR_BAD_ARG, "doc_ptr must be non-decreasing");
    if (doc_ptr[d + 1] - doc_ptr[d] > ((int64_t)1 << 25))
      return set_err(h, GGS_ERR_UNSUPPORTED, "a test document has more than 2^25 tokens (one Philox stream per particle: 2^24 blocks of two uniforms)");
  }
  const int64_t N = doc_ptr[D];
  if (N > 0 && !tokens) return set_err(h, GGS_ERR_BAD_ARG, "tokens is null");
  for (int64_t i = 0; i < N; ++i)
    if (tokens[i] < 0) return set_err(h, GGS_ERR_BAD_ARG, "negative token id");    // ids >= num_types are out of vocabulary (MPE:341-345)
  int rc = bind_device(h);
  if (rc) return rc;
  HIP_TRY(h, hipStreamSynchronize(h->stream));
  if ((rc = dev_alloc(h, &h->d_test_ptr, (size_t)D + 1)) || (rc = dev_alloc(h, &h->d_test_tok, (size_t)N)) || (rc = dev_alloc(h, &h->d_test_ll, (size_t)D))) return rc;
  HIP_TRY(h, hipMemcpy(h->d_test_ptr, doc_ptr, sizeof(int64_t) * (size_t)(D + 1), hipMemcpyHostToDevice));
  if (N) HIP_TRY(h, hipMemcpy(h->d_test_tok, tokens, sizeof(int32_t) * (size_t)N, hipMemcpyHostToDevice));
  h->test_ptr.assign(doc_ptr, doc_ptr + D + 1);
  // by the width a particle's per-topic counts need: one byte (documents of at most 255 tokens), two (65 535), four
  h->test_short.clear(); h->test_long.clear(); h->test_huge.clear();
  for (int64_t d = 0; d < D; ++d) {
    const int64_t len = doc_ptr[d + 1] - doc_ptr[d];
    (len <= 255 ? h->test_short : len <= 65535 ? h->test_long : h->test_huge).push_back((int32_t)d);
  }
  if ((rc = dev_alloc(h, &h->d_test_docs, (size_t)D))) return rc;
  {
    size_t at = 0;
    for (const std::vector<int32_t> *ids : {&h->test_short, &h->test_long, &h->test_huge}) {
      if (!ids->empty()) HIP_TRY(h, hipMemcpy(h->d_test_docs + at, ids->data(), sizeof(int32_t) * ids->size(), hipMemcpyHostToDevice));
      at += ids->size();
    }
  }
  h->test_doc_base = doc_base;
  h->have_test = true;
  return GGS_OK;
}

int ggs_heldout_log_likelihood(ggs_handle *h, int32_t num_particles, double *doc_ll, double *total) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  if (!h->have_test) return set_err(h, GGS_ERR_STATE, "no test set: call ggs_set_test_corpus first");
  if (num_particles < 1 || !total) return set_err(h, GGS_ERR_BAD_ARG, "num_particles < 1 or null output");
  if ((rc = launch_magnitude(h))) return rc;       // corpus-wide counts gathered, tokensPerTopic in step with them
  const int K = h->K;
  const int64_t D = (int64_t)h->test_ptr.size() - 1;
  // LDS: alpha, the denominators and the coefficient table once per block; per wave the word's cell list and 1 or 2 bytes
  // per (particle, topic).  The block shape that puts most waves on a CU wins (the kernel is issue-bound).
  const size_t Kpad = (size_t)(K + 63) / 64 * 64;
  auto lds_of = [&](int w, int cnt_bytes, int cap) { return (size_t)(16 + 8 * cap) * K + (size_t)w * (Kpad * 8 + (size_t)K * 64 * cnt_bytes); };
  struct Shape { int waves = 0, per_cu = 0, cap = 0; };
  auto shape_for = [&](int cnt_bytes, int cap) {
    Shape s; s.cap = cap;
    for (int w = kHeldoutMaxWaves; w >= 1; w >>= 1) {
      const size_t alloc = (lds_of(w, cnt_bytes, cap) + 2047) / 2048 * 2048;   // LDS is handed out in 2 KiB granules
      const int per_cu = alloc <= (size_t)160 * 1024 ? std::min((int)((size_t)160 * 1024 / alloc) * w, 32) : 0;
      if (per_cu && per_cu >= s.per_cu) { s.per_cu = per_cu; s.waves = w; }       // ties: the smaller block (documents differ in length)
    }
    return s;
  };
  // the deepest coefficient table that costs no wave (measured at K=100: 16 -> 31 ms, 32 -> 26, 48 -> 24.6 per evaluation)
  auto best_shape = [&](int cnt_bytes) {
    const int n_caps = (int)(sizeof(kHeldoutCoefCaps) / sizeof(kHeldoutCoefCaps[0]));
    const Shape floor = shape_for(cnt_bytes, kHeldoutCoefCaps[n_caps - 1]);
    for (int i = 0; i < n_caps; ++i) {
      const Shape s = shape_for(cnt_bytes, kHeldoutCoefCaps[i]);
      if (s.per_cu && s.per_cu >= floor.per_cu) return s;
    }
    return floor;
  };
  // a class of documents whose per-particle counts do not fit LDS (more than 1704 topics with one-byte counts, 1024 with
  // two; four-byte counts always) keeps them in global memory: the LDS then holds the tables and the cell lists only
  const Shape shape8 = best_shape(1), shape16 = best_shape(2), shape_spill = best_shape(0);
  const bool spill8 = !h->test_short.empty() && !shape8.waves, spill16 = !h->test_long.empty() && !shape16.waves, spill32 = !h->test_huge.empty();
  if ((spill8 || spill16 || spill32) && !shape_spill.waves)
    return set_err(h, GGS_ERR_UNSUPPORTED, "num_topics too large for the held-out estimator's tables in LDS (about 6000 topics)");
  const int64_t spill_blocks = (int64_t)h->num_cus * std::max(1, shape_spill.waves ? shape_spill.per_cu / shape_spill.waves : 1);   // a persistent grid: what is resident
  if (spill8 || spill16 || spill32) {
    const size_t need = (size_t)spill_blocks * shape_spill.waves * (size_t)K * 64 * (spill32 ? 4 : spill16 ? 2 : 1);
    if (h->heldout_spill_bytes < need) {
      if (h->d_heldout_spill) (void)hipFree(h->d_heldout_spill);
      h->d_heldout_spill = nullptr; h->heldout_spill_bytes = 0;
      HIP_TRY(h, hipMalloc(&h->d_heldout_spill, need));
      h->heldout_spill_bytes = need;
    }
  }
  const void *kernels[] = {reinterpret_cast<const void *>(heldout_particles_kernel<uint8_t, false>), reinterpret_cast<const void *>(heldout_particles_kernel<uint16_t, false>),
                           reinterpret_cast<const void *>(heldout_particles_kernel<uint8_t, true>), reinterpret_cast<const void *>(heldout_particles_kernel<uint16_t, true>),
                           reinterpret_cast<const void *>(heldout_particles_kernel<uint32_t, true>)};
  for (const void *f : kernels) HIP_TRY(h, hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes));
  // wordProbabilities of a batch of documents: tokens x particles doubles, at most ~4 GiB at a time (one launch for
  // the 2 M-token test set of the benchmark: every extra launch has its own tail of half-empty CUs)
  int64_t want_cells = (int64_t)1 << 29;
  if (const char *e = debug_env("GGS_DEBUG_HELDOUT_CELLS")) want_cells = std::max<int64_t>(1, std::atoll(e));   // tests: force several batches
  int64_t longest = 1;
  for (int64_t d = 0; d < D; ++d) longest = std::max(longest, h->test_ptr[d + 1] - h->test_ptr[d]);
  const int64_t cap_cells = std::max<int64_t>(want_cells, longest * num_particles);                                 // a document is never split
  int64_t max_cells = 0;
  std::vector<int64_t> cuts{0};
  for (int64_t d = 0; d < D;) {
    int64_t e = d;
    while (e < D && (h->test_ptr[e + 1] - h->test_ptr[d]) * num_particles <= cap_cells) ++e;
    max_cells = std::max(max_cells, (h->test_ptr[e] - h->test_ptr[d]) * num_particles);
    cuts.push_back(e);
    d = e;
  }
  const size_t tab_bytes = sizeof(double) * (size_t)(2 * K + 2);
  if ((rc = ensure_scratch(h, tab_bytes + sizeof(double) * (size_t)std::max<int64_t>(max_cells, 1)))) return rc;
  HeldoutParams hp{};
  hp.doc_ptr = h->d_test_ptr; hp.tok = h->d_test_tok; hp.n_wk = h->d_n_wk;
  auto *tab = static_cast<double *>(h->d_scratch);
  hp.tab = tab; hp.probs = tab + 2 * K + 2; hp.doc_ll = h->d_test_ll; hp.status = h->d_status;
  hp.beta = h->beta;
  double alpha_sum = 0;
  for (int k = 0; k < K; ++k) alpha_sum += h->alpha[k];
  hp.alpha_sum = alpha_sum;
  hp.seed = h->seed; hp.iteration = (uint32_t)h->iteration; hp.doc_base = h->test_doc_base;
  hp.K = K; hp.V = h->V; hp.P = num_particles; hp.blocks_per_doc = (num_particles + 63) / 64;
  hipLaunchKernelGGL(heldout_setup_kernel, dim3(1), dim3(64), 0, h->stream, h->d_alpha, h->d_n_k, h->beta, h->beta * h->V, K, tab);
  for (size_t b = 0; b + 1 < cuts.size(); ++b) {
    hp.d0 = cuts[b]; hp.d1 = cuts[b + 1];
    if (hp.d1 == hp.d0) continue;
    // the batch's short and long documents: sub-ranges of the two ascending id lists
    auto range = [&](const std::vector<int32_t> &ids, size_t &lo, size_t &hi) {
      lo = std::lower_bound(ids.begin(), ids.end(), (int32_t)hp.d0) - ids.begin();
      hi = std::lower_bound(ids.begin(), ids.end(), (int32_t)hp.d1) - ids.begin();
    };
    // one launch per class of documents present in the batch: counts in LDS where they fit, in global memory otherwise
    struct Class { const std::vector<int32_t> *ids; size_t offset; int bytes; bool spill; Shape shape; };
    const Class classes[] = {{&h->test_short, 0, 1, spill8, spill8 ? shape_spill : shape8},
                             {&h->test_long, h->test_short.size(), 2, spill16, spill16 ? shape_spill : shape16},
                             {&h->test_huge, h->test_short.size() + h->test_long.size(), 4, true, shape_spill}};
    for (const Class &c : classes) {
      size_t lo, hi;
      range(*c.ids, lo, hi);
      if (hi <= lo) continue;
      hp.docs = h->d_test_docs + c.offset + lo; hp.n_docs = (int64_t)(hi - lo); hp.waves = c.shape.waves; hp.cap = c.shape.cap;
      hp.cnt_spill = c.spill ? h->d_heldout_spill : nullptr;
      const int64_t units = hp.n_docs * hp.blocks_per_doc, blocks = (units + hp.waves - 1) / hp.waves;
      const dim3 grid((unsigned)(c.spill ? std::min(blocks, spill_blocks) : blocks)), block((unsigned)(hp.waves * 64));
      const size_t lds = lds_of(hp.waves, c.spill ? 0 : c.bytes, hp.cap);
      const void *f = c.spill ? (c.bytes == 1 ? kernels[2] : c.bytes == 2 ? kernels[3] : kernels[4]) : (c.bytes == 1 ? kernels[0] : kernels[1]);
      void *args[] = {&hp};
      HIP_TRY(h, hipLaunchKernel(f, grid, block, args, lds, h->stream));
    }
    hipLaunchKernelGGL(heldout_reduce_kernel, dim3((unsigned)((hp.d1 - hp.d0 + 3) / 4)), dim3(256), 0, h->stream, hp);
  }
  HIP_TRY(h, hipGetLastError());
  std::vector<double> ll((size_t)D);
  if (D) HIP_TRY(h, hipMemcpyAsync(ll.data(), h->d_test_ll, sizeof(double) * (size_t)D, hipMemcpyDeviceToHost, h->stream));
  if ((rc = check_status(h))) return rc;                    // synchronises; MPE:416,447,455,464-469 surface here
  double t = 0;
  for (int64_t d = 0; d < D; ++d) t += ll[(size_t)d];       // MPE:116: in document order
  *total = t;
  if (doc_ll && D) std::memcpy(doc_ll, ll.data(), sizeof(double) * (size_t)D);
  return GGS_OK;
}

int ggs_get_timings(ggs_handle *h, ggs_timings *out) { if (!h || !out) return GGS_ERR_BAD_ARG; *out = h->tm; return GGS_OK; }
int ggs_reset_timings(ggs_handle *h) { if (!h) return GGS_ERR_BAD_ARG; h->tm = ggs_timings{}; return GGS_OK; }

int ggs_check_invariants(ggs_handle *h) {
  int rc = require_ready(h, false);
  if (rc) return rc;
  const int K = h->K;
  const size_t bytes = 16 + sizeof(int32_t) * (size_t)K;
  if ((rc = ensure_global_counts(h))) return rc;
  if ((rc = ensure_scratch(h, bytes))) return rc;
  auto *d_total = static_cast<unsigned long long *>(h->d_scratch);
  auto *d_flags = reinterpret_cast<uint32_t *>(static_cast<char *>(h->d_scratch) + 8);
  auto *d_col = reinterpret_cast<int32_t *>(static_cast<char *>(h->d_scratch) + 16);
  HIP_TRY(h, hipMemsetAsync(h->d_scratch, 0, bytes, h->stream));
  const int64_t kv = (int64_t)K * h->V;
  hipLaunchKernelGGL(invariants_kernel, dim3(grid_for(kv, 256)), dim3(256), 0, h->stream, h->d_n_wk, kv, K, d_total, d_col, d_flags);
  HIP_TRY(h, hipGetLastError());
  if ((rc = launch_magnitude(h))) return rc;
  std::vector<unsigned char> host(bytes);
  std::vector<int32_t> nk((size_t)K);
  if ((rc = copy_out(h, host.data(), h->d_scratch, bytes))) return rc;
  if ((rc = copy_out(h, nk.data(), h->d_n_k, sizeof(int32_t) * (size_t)K))) return rc;
  unsigned long long total; uint32_t fl;
  std::memcpy(&total, host.data(), 8); std::memcpy(&fl, host.data() + 8, 4);
  const int32_t *col = reinterpret_cast<const int32_t *>(host.data() + 16);
  if (fl & 1u) return set_err(h, GGS_ERR_INVARIANT, "negative type-topic count");
  if ((int64_t)total != (h->global_tokens >= 0 ? h->global_tokens : h->N)) return set_err(h, GGS_ERR_INVARIANT, "type-topic counts do not sum to the corpus size");
  for (int k = 0; k < K; ++k)
    if (col[k] != nk[(size_t)k]) return set_err(h, GGS_ERR_INVARIANT, "column sum differs from tokensPerTopic");
  return GGS_OK;
}

int ggs_get_launch_info(ggs_handle *h, int64_t *num_chunks, int32_t *lds_bytes_z, int32_t *docs_per_block_theta) {
  if (!h) return GGS_ERR_BAD_ARG;
  const LaunchPlan &pl = h->plan;
  const bool pcgs = pcgs_family(h->scheme);            // what launch_pcgs_z launches, over what
  if (num_chunks) *num_chunks = pcgs ? h->pcgs_items : pl.sliced() ? h->Cs + h->Cw : h->C;
  if (lds_bytes_z) *lds_bytes_z = pcgs ? h->pcgs_z.lds : pl.sliced() ? sliced_fused_lds(h->K, pl.hot_cap) : pl.z.lds;
  if (docs_per_block_theta) *docs_per_block_theta = h->cfg->theta_docs;
  return GGS_OK;
}

int ggs_get_num_hot_words(ggs_handle *h, int32_t *num_hot) {
  if (!h || !num_hot) return GGS_ERR_BAD_ARG;
  *num_hot = h->plan.sliced() ? h->num_hot + h->num_warm : 0;
  return GGS_OK;
}

int ggs_get_z_parts(ggs_handle *h, int32_t *parts) {
  if (!h || !parts) return GGS_ERR_BAD_ARG;
  const int32_t P = (int32_t)h->part_doc.size() - 1;
  *parts = (h->plan.stream() && h->overlap_theta && P > 1) ? P : 1;
  return GGS_OK;
}

int ggs_get_warm_tiers(ggs_handle *h, int32_t *tiers, int32_t *warm_words, int32_t *docs_per_chunk) {
  if (!h) return GGS_ERR_BAD_ARG;
  const bool on = h->have_corpus && h->plan.sliced();
  if (tiers) *tiers = on ? h->warm_tiers : 0;
  if (warm_words) *warm_words = on ? h->num_warm : 0;
  if (docs_per_chunk) *docs_per_chunk = on && h->warm_tiers ? h->plan.warm_docs : 0;
  return GGS_OK;
}

int ggs_get_z_form(ggs_handle *h, int32_t *kernel, int32_t *form, int32_t *calibrated) {
  if (!h) return GGS_ERR_BAD_ARG;
  const bool splittable = h->plan.sliced() && h->Cs > h->Cc && h->Cc > 0;
  const int32_t own = row_of(h->scheme).z_kernel;
  if (kernel) *kernel = own ? own : pcgs_family(h->scheme) ? (h->pcgs_wave ? 5 : 4) : h->plan.kernel;
  if (form) *form = h->plan.sliced() ? (splittable && h->z_split ? 1 : 2) : 0;
  if (calibrated) *calibrated = (splittable && h->z_split_tried && !h->plan.split_forced && h->plan.split) ? 1 : 0;
  return GGS_OK;
}

int ggs_java_lcg_next_ints(int32_t seed, int32_t bound, int64_t n, int32_t *out) {
  if (bound <= 0 || n < 0 || (n > 0 && !out)) return GGS_ERR_BAD_ARG;
  java_lcg_next_ints(seed, bound, n, out);
  return GGS_OK;
}

// ---- primitives for the parity tests ---------------------------------------------
namespace {
struct TmpDev {
  std::vector<void *> p;
  ~TmpDev() { for (void *q : p) if (q) (void)hipFree(q); }
  void *get(size_t bytes) { void *q = nullptr; if (hipMalloc(&q, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr; p.push_back(q); return q; }
};
}  // namespace

int ggs_debug_philox(int32_t device_id, int64_t n, const uint32_t *ctr, const uint32_t *key, uint32_t *out) {
  if (n <= 0 || !ctr || !key || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *dc = static_cast<uint32_t *>(t.get(n * 16)); auto *dk = static_cast<uint32_t *>(t.get(n * 8)); auto *dou = static_cast<uint32_t *>(t.get(n * 16));
  if (!dc || !dk || !dou) return GGS_ERR_HIP;
  if (hipMemcpy(dc, ctr, n * 16, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dk, key, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_philox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, n, dc, dk, dou);
  if (hipMemcpy(out, dou, n * 16, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_math(int32_t device_id, int32_t op, int64_t n, const double *x, const double *y, double *out) {
  if (n <= 0 || !x || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *dx = static_cast<double *>(t.get(n * 8)); auto *dy = static_cast<double *>(t.get(n * 8)); auto *dou = static_cast<double *>(t.get(n * 8));
  if (!dx || !dy || !dou) return GGS_ERR_HIP;
  if (hipMemcpy(dx, x, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemcpy(dy, y ? y : x, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, op, n, dx, dy, dou);
  if (hipMemcpy(out, dou, n * 8, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_draw(int32_t device_id, int32_t kind, uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0, int64_t n,
                   const double *shape, double *out, int32_t *status) {
  if (n <= 0 || !out || (kind == 2 && !shape) || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *ds = static_cast<double *>(t.get(n * 8)); auto *dou = static_cast<double *>(t.get(n * 8)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!ds || !dou || !dst) return GGS_ERR_HIP;
  if (shape && hipMemcpy(ds, shape, n * 8, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemset(dst, 0, 16) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_draw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, kind, seed, iteration, purpose, elem0, n, ds, dou, dst);
  uint32_t st = 0;
  if (hipMemcpy(out, dou, n * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  if (status) *status = (int32_t)st;
  return GGS_OK;
}

int ggs_debug_poisson(int32_t device_id, double beta, int32_t threshold, uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0, int64_t n,
                      const int32_t *counts, int32_t *out) {
  const int32_t L = threshold == 0 ? 100 : threshold;
  if (n <= 0 || !counts || !out || !(beta > 0) || L < 1 || L > kPoissonMaxThreshold || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  for (int64_t i = 0; i < n; ++i)
    if (counts[i] < 0) return GGS_ERR_BAD_ARG;
  std::vector<double> T;
  build_poisson_table(beta, L, T);
  TmpDev t;
  auto *dt = static_cast<double *>(t.get(T.size() * 8)); auto *dc = static_cast<int32_t *>(t.get(n * 4));
  auto *dou = static_cast<int32_t *>(t.get(n * 4)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!dt || !dc || !dou || !dst) return GGS_ERR_HIP;
  if (hipMemcpy(dt, T.data(), T.size() * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dc, counts, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(dst, 0, 16) != hipSuccess)
    return GGS_ERR_HIP;
  hipLaunchKernelGGL(debug_poisson_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, seed, iteration, purpose, elem0, n, dc, L, beta, dt, T[0],
                     dou, dst);
  uint32_t st = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpy(out, dou, n * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return st ? GGS_ERR_RNG_EXHAUSTED : GGS_OK;
}

int ggs_debug_alias(int32_t device_id, int32_t V, int32_t K, const double *phi, const double *alpha, double *ps, int32_t *a, double *type_norm) {
  if (V <= 0 || K <= 0 || K > kPcgsWaveMaxTopics || !phi || !alpha || !ps || !a || !type_norm || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  const size_t kv = (size_t)K * V;
  std::vector<double> phiT(kv);                         // [V][K], as the handle keeps it (pitch K here)
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) phiT[(size_t)v * K + k] = phi[(size_t)k * V + v];
  TmpDev t;
  auto *dphi = static_cast<double *>(t.get(kv * 8)); auto *dal = static_cast<double *>(t.get((size_t)K * 8));
  auto *dps = static_cast<double *>(t.get(kv * 8)); auto *da = static_cast<int32_t *>(t.get(kv * 4)); auto *dtn = static_cast<double *>(t.get((size_t)V * 8));
  if (!dphi || !dal || !dps || !da || !dtn) return GGS_ERR_HIP;
  if (hipMemcpy(dphi, phiT.data(), kv * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dal, alpha, (size_t)K * 8, hipMemcpyHostToDevice) != hipSuccess)
    return GGS_ERR_HIP;
  AliasParams ap{};
  ap.phiT = dphi; ap.alpha = dal; ap.ps = dps; ap.a = da; ap.type_norm = dtn; ap.V = V; ap.K = K; ap.Kp = K; ap.wpb = alias_words_per_block(K);
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(alias_build_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLdsBytes) != hipSuccess) return GGS_ERR_HIP;
  hipLaunchKernelGGL(alias_build_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)V + ap.wpb - 1) / ap.wpb, 4096)), dim3(64), alias_lds_bytes(K, ap.wpb), nullptr, ap);
  if (hipGetLastError() != hipSuccess || hipMemcpy(ps, dps, kv * 8, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(a, da, kv * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(type_norm, dtn, (size_t)V * 8, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_vs_indicators(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, const double *prev_phi, double beta, double pi, uint64_t seed,
                            uint32_t iteration, const double *u, uint8_t *drawn_out, int32_t *s_end, int32_t *rounds) {
  if (V <= 0 || K <= 0 || !counts || !prev_phi || !drawn_out || !s_end || !rounds || !(beta > 0) || !(pi > 0.0 && pi < 1.0) || hipSetDevice(device_id) != hipSuccess)
    return GGS_ERR_BAD_ARG;
  const Knobs kn;
  const bool global = V > kVsLdsMaxV || (kn.vs_global.set && kn.vs_global.v != 0);
  const size_t kv = (size_t)K * V;
  const int32_t W = (V + 31) / 32;
  const size_t kw = (size_t)K * W;
  std::vector<int32_t> cntT(kv), n_k((size_t)K, 0);     // [V][K], as the handle keeps them
  std::vector<double> phiT(kv);
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) {
      const int32_t c = counts[(size_t)k * V + v];
      if (c < 0) return GGS_ERR_BAD_ARG;
      cntT[(size_t)v * K + k] = c; n_k[(size_t)k] += c;
      phiT[(size_t)v * K + k] = prev_phi[(size_t)k * V + v];
    }
  TmpDev t;
  auto *dc = static_cast<int32_t *>(t.get(kv * 4)); auto *dphi = static_cast<double *>(t.get(kv * 8)); auto *dnk = static_cast<int32_t *>(t.get((size_t)K * 4));
  auto *dcz = static_cast<uint32_t *>(t.get(kw * 4)); auto *dpz = static_cast<uint32_t *>(t.get(kw * 4)); auto *dun = static_cast<uint32_t *>(t.get(kw * 4));
  auto *dwork = static_cast<int32_t *>(t.get(global ? 2 * kw * 4 : 16)); auto *du = static_cast<double *>(t.get(u ? kv * 8 : 16));
  auto *dse = static_cast<int32_t *>(t.get((size_t)K * 4)); auto *dro = static_cast<int32_t *>(t.get((size_t)K * 4)); auto *dst = static_cast<uint32_t *>(t.get(16));
  if (!dc || !dphi || !dnk || !dcz || !dpz || !dun || !dwork || !du || !dse || !dro || !dst) return GGS_ERR_HIP;
  if (hipMemcpy(dc, cntT.data(), kv * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dphi, phiT.data(), kv * 8, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(dnk, n_k.data(), (size_t)K * 4, hipMemcpyHostToDevice) != hipSuccess || (u && hipMemcpy(du, u, kv * 8, hipMemcpyHostToDevice) != hipSuccess) ||
      hipMemset(dst, 0, 16) != hipSuccess)
    return GGS_ERR_HIP;
  VsBitsParams bp{};
  bp.cnt = dc; bp.phiT = dphi; bp.cz = dcz; bp.pz = dpz; bp.cnt_pitch = K; bp.Kp = K; bp.k0 = 0; bp.Ks = K; bp.V = V; bp.W = W;
  hipLaunchKernelGGL(vs_bits_kernel, dim3((unsigned)std::min<int64_t>((int64_t)W * ((K + 63) / 64), 4096)), dim3(64), 0, nullptr, bp);
  VsChainParams cp{};
  cp.cz = dcz; cp.pz = dpz; cp.und = dun; cp.work = dwork; cp.n_k = dnk; cp.u = u ? du : nullptr; cp.s_end = dse; cp.rounds = dro; cp.status = dst;
  cp.seed = seed; cp.iteration = iteration; cp.Ks = K; cp.k0 = 0; cp.V = V; cp.W = W; cp.beta = beta; cp.odds = pi / (1 - pi);
  if (global) hipLaunchKernelGGL(vs_chain_kernel<true>, dim3((unsigned)K), dim3(kVsBlock), 0, nullptr, cp);
  else hipLaunchKernelGGL(vs_chain_kernel<false>, dim3((unsigned)K), dim3(kVsBlock), vs_chain_lds_bytes(W), nullptr, cp);
  std::vector<uint32_t> und(kw);
  uint32_t st = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpy(und.data(), dun, kw * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(s_end, dse, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(rounds, dro, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&st, dst, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  for (int32_t k = 0; k < K; ++k)
    for (int32_t v = 0; v < V; ++v) drawn_out[(size_t)k * V + v] = (uint8_t)(((und[(size_t)k * W + (v >> 5)] >> (v & 31)) & 1u) ^ 1u);
  return (st & ST_INVARIANT) ? GGS_ERR_INVARIANT : GGS_OK;
}

int ggs_debug_column_sum_guided(int32_t device_id, int32_t V, int32_t K, const double *x, const int32_t *counts, double beta, const double *guess,
                                double *out, double *pref_out, int32_t *n_k_out) {
  if (V <= 0 || K <= 0 || (!x == !counts) || !out || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const size_t kv = (size_t)V * K;
  ggs_handle tmp;                                     // only the fields launch_column_sum reads
  tmp.K = K; tmp.V = V; tmp.beta = beta; tmp.stream = nullptr; tmp.exact_sum = true;
  tmp.sum_nseg = (V + kSumSegRows - 1) / kSumSegRows;
  const size_t pref_bytes = ((size_t)tmp.sum_nseg + 1) * K * 8;
  tmp.d_sum_pref = static_cast<double *>(t.get(pref_bytes));
  tmp.d_sum_fn = static_cast<double *>(t.get((size_t)tmp.sum_nseg * K * 32));
  void *dsrc = t.get(kv * (x ? 8 : 4));
  auto *dou = static_cast<double *>(t.get((size_t)K * 8));
  auto *dnk = static_cast<int32_t *>(t.get((size_t)K * 4));
  int rc = GGS_OK;
  if (!tmp.d_sum_pref || !tmp.d_sum_fn || !dsrc || !dou || !dnk) rc = GGS_ERR_HIP;
  else if (hipMemcpy(dsrc, x ? (const void *)x : (const void *)counts, kv * (x ? 8 : 4), hipMemcpyHostToDevice) != hipSuccess) rc = GGS_ERR_HIP;
  else if (guess && hipMemcpy(tmp.d_sum_pref, guess, pref_bytes, hipMemcpyHostToDevice) != hipSuccess) rc = GGS_ERR_HIP;
  else {
    if (x) launch_column_sum<double, false>(&tmp, static_cast<const double *>(dsrc), K, K, dou, nullptr, guess != nullptr, true);
    else launch_column_sum<int32_t, true>(&tmp, static_cast<const int32_t *>(dsrc), K, K, dou, dnk, guess != nullptr, true);
    if (hipGetLastError() != hipSuccess || hipMemcpy(out, dou, (size_t)K * 8, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
    else if (pref_out && hipMemcpy(pref_out, tmp.d_sum_pref, pref_bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
    else if (n_k_out && counts && hipMemcpy(n_k_out, dnk, (size_t)K * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = GGS_ERR_HIP;
  }
  tmp.d_sum_pref = nullptr; tmp.d_sum_fn = nullptr;   // owned by t
  return rc;
}

int ggs_debug_column_sum(int32_t device_id, int32_t V, int32_t K, const double *x, const int32_t *counts, double beta, double *out) {
  return ggs_debug_column_sum_guided(device_id, V, K, x, counts, beta, nullptr, out, nullptr, nullptr);
}

int ggs_debug_min_distances(int32_t device_id, const double *a, int64_t n, const double *b, int64_t m, int64_t len, int32_t element_major, double *min_dist,
                            double *min_sq) {
  if (!a || !min_dist || n <= 0 || len <= 0 || (b && m <= 0) || (element_major && b) || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  auto *da = static_cast<double *>(t.get(sizeof(double) * (size_t)n * (size_t)len));
  auto *db = b ? static_cast<double *>(t.get(sizeof(double) * (size_t)m * (size_t)len)) : da;
  auto *dbits = static_cast<unsigned long long *>(t.get(sizeof(double) * (size_t)n));
  auto *dout = static_cast<double *>(t.get(sizeof(double) * (size_t)n)), *dsq = static_cast<double *>(t.get(sizeof(double) * (size_t)n));
  if (!da || !db || !dbits || !dout || !dsq) return GGS_ERR_HIP;
  if (hipMemcpy(da, a, sizeof(double) * (size_t)n * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (b && hipMemcpy(db, b, sizeof(double) * (size_t)m * (size_t)len, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(min_dist_preset_kernel, dim3(grid), dim3(256), 0, nullptr, dbits, n);
  if (element_major) launch_min_topic_dist(nullptr, da, n, n, len, dbits);
  else launch_min_row_dist(nullptr, da, n, db, b ? m : n, len, b == nullptr, dbits);
  hipLaunchKernelGGL(min_dist_finish_kernel, dim3(grid), dim3(256), 0, nullptr, dbits, n, dout, dsq);
  if (hipGetLastError() != hipSuccess || hipMemcpy(min_dist, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  if (min_sq && hipMemcpy(min_sq, dsq, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_summaries(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, double beta, double lambda, int32_t kind, int32_t n_words,
                              int32_t *idx, double *score, double *mass_k, double *rowsum_w, double *total, double *all_scores) {
  if (V <= 0 || K <= 0 || !counts || hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  int rc = ts_check_args(nullptr, V, K, beta, kind, n_words, lambda, idx);
  if (rc) return rc;
  TmpDev t;
  const TsPlan q(V, K, n_words);
  const size_t kv = (size_t)V * K;
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dcnt = static_cast<int32_t *>(t.get(kv * 4));
  double *dall = all_scores ? static_cast<double *>(t.get(kv * 8)) : nullptr;
  if (!work || !dcnt || (all_scores && !dall)) return GGS_ERR_HIP;
  if (hipMemcpy(dcnt, counts, kv * 4, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  // GGS_DEBUG_CHAIN=1: both column sums walked element by element
  ts_launch(nullptr, !Knob("GGS_DEBUG_CHAIN").is(1), dcnt, beta, lambda, kind, q, work, true, dall);
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  if (hipGetLastError() != hipSuccess || !fetch(idx, work + q.idx, 4 * (size_t)K * n_words) || !fetch(score, work + q.score, 8 * (size_t)K * n_words) ||
      !fetch(mass_k, work + q.mass, 8 * (size_t)K) || !fetch(rowsum_w, work + q.rowsum, 8 * (size_t)V) || !fetch(total, work + q.total, 8) ||
      !fetch(all_scores, dall, kv * 8))
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_doc_statistics(int32_t device_id, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, const int32_t *z, int32_t V, int32_t K,
                                   const double *alpha, int32_t n_words, const int32_t *idx, const double *clogc_in, int32_t *codoc, int32_t *doc_stats,
                                   double *clogc_out) {
  if (D < 0 || V <= 0 || K <= 0 || !doc_ptr || !alpha || !idx || !codoc || !doc_stats || !clogc_out || doc_ptr[0] != 0) return GGS_ERR_BAD_ARG;
  for (int64_t d = 0; d < D; ++d)
    if (doc_ptr[d + 1] < doc_ptr[d]) return GGS_ERR_BAD_ARG;
  const int64_t N = doc_ptr[D];
  if (N > 0 && (!tokens || !z)) return GGS_ERR_BAD_ARG;
  for (int64_t t = 0; t < N; ++t)
    if (tokens[t] < 0 || tokens[t] >= V || z[t] < 0 || z[t] >= K) return GGS_ERR_BAD_ARG;
  int rc = td_check_args(nullptr, V, K, n_words, idx);
  if (rc || (rc = td_check_topics(nullptr, K))) return rc;
  if (hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const TdDocPlan q(D, V, K, n_words);
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dptr = static_cast<int64_t *>(t.get(8 * ((size_t)D + 1)));
  auto *dtok = static_cast<int32_t *>(t.get(4 * (size_t)N)), *dz = static_cast<int32_t *>(t.get(4 * (size_t)N));
  auto *dalpha = static_cast<double *>(t.get(8 * (size_t)K));
  if (!work || !dptr || !dtok || !dz || !dalpha) return GGS_ERR_HIP;
  if (hipMemcpy(dptr, doc_ptr, 8 * ((size_t)D + 1), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dalpha, alpha, 8 * (size_t)K, hipMemcpyHostToDevice) != hipSuccess ||
      (N > 0 && (hipMemcpy(dtok, tokens, 4 * (size_t)N, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(dz, z, 4 * (size_t)N, hipMemcpyHostToDevice) != hipSuccess)))
    return GGS_ERR_HIP;
  if (td_doc_launch(nullptr, q, work, dptr, dtok, dz, dalpha, td_alpha_sum(alpha, K), idx, clogc_in, nullptr) != hipSuccess) return GGS_ERR_HIP;
  if (hipMemcpy(codoc, work + q.codoc, 4 * (size_t)K * n_words * n_words, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(doc_stats, work + q.stats, 4 * (size_t)K * kTdStats, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(clogc_out, work + q.clogc, 8 * (size_t)K, hipMemcpyDeviceToHost) != hipSuccess)
    return GGS_ERR_HIP;
  return GGS_OK;
}

int ggs_debug_topic_scores(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, double beta, int32_t n_words, const int32_t *idx, const int32_t *codoc,
                           const int32_t *doc_stats, const double *clogc, double *topic_scores, double *word_scores, int32_t *sorted_ids) {
  if (V <= 0 || K <= 0 || !counts || !idx || !codoc || !doc_stats || !clogc || !topic_scores) return GGS_ERR_BAD_ARG;
  int rc = td_check_args(nullptr, V, K, n_words, idx);
  if (rc) return rc;
  if ((int64_t)V * K > ((int64_t)1 << 31) - 256) return GGS_ERR_UNSUPPORTED;
  for (size_t i = 0; i < (size_t)V * K; ++i)
    if (counts[i] < 0) return GGS_ERR_BAD_ARG;
  if (hipSetDevice(device_id) != hipSuccess) return GGS_ERR_BAD_ARG;
  TmpDev t;
  const TdScorePlan q(V, K, n_words);
  const size_t kv = (size_t)V * K;
  char *work = static_cast<char *>(t.get(q.bytes));
  auto *dcnt = static_cast<int32_t *>(t.get(kv * 4));
  if (!work || !dcnt) return GGS_ERR_HIP;
  if (hipMemcpy(dcnt, counts, kv * 4, hipMemcpyHostToDevice) != hipSuccess) return GGS_ERR_HIP;
  if (td_score_launch(nullptr, q, work, dcnt, K, beta, idx, codoc, doc_stats, clogc, word_scores != nullptr, nullptr) != hipSuccess) return GGS_ERR_HIP;
  auto fetch = [&](void *dst, const void *src, size_t bytes) { return !dst || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess; };
  if (!fetch(topic_scores, work + q.ts, 8 * (size_t)kTdScoreRows * K) || !fetch(word_scores, work + q.ws, 8 * (size_t)kTdWordRows * K * n_words) ||
      !fetch(sorted_ids, work + q.head, 4 * (size_t)K * n_words))
    return GGS_ERR_HIP;
  return GGS_OK;
}

}  // extern "C"
