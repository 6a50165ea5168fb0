/*
 * ggs_hip.h -- C-ABI of libggs_hip.so, the MI355X (gfx950) implementation of
 * the LDA Grouped Gibbs Sampler hot path.
 *
 * The reference (clintpgeorge/LDAGroupedGibbsSampler) is 100 % Java and has no
 * FFI; this header is the boundary a thin JNI shim binds (INTEGRATION.md shows
 * the shim).  Every entry point names the reference method(s) whose work it
 * replaces; paths are relative to src/main/java/cc/mallet/ in the reference:
 *   GGS   = topics/LDAGroupedGibbsSampler.java
 *   UPLDA = topics/UncollapsedParallelLDA.java
 *   MSLDA = topics/ModifiedSimpleLDA.java
 *
 * Conventions: plain pointers and sizes only; every function returns
 * GGS_OK (0) or a GGS_ERR_* code, with text available from ggs_last_error();
 * the caller owns every host buffer, which is only touched during the call; a
 * handle is driven by ONE coordinator thread (as the Java sampler is,
 * UPLDA:552-943).  Host layouts mirror the Java getters: counts are
 * int32 [V][K] (getTypeTopicMatrix), Phi is double [K][V] (getPhi).
 * The library reads no environment variable in normal use; its GGS_DEBUG_* knobs (kernel selection, proof margins,
 * overlaps: tests and experiments) are honoured only when GGS_DEBUG=1 is set as well.
 *
 * One handle = one GPU.  Several live handles on the SAME device in one process are correct but slow: each brings
 * three streams and the runtime multiplexes all of them onto the device's few hardware queues (measured: a second
 * handle's sweeps ran 6x slower beside an idle first one) -- destroy a handle before building its successor.
 *
 * Several GPUs: documents are sharded contiguously, one handle per shard (doc_base / tok_base of ggs_set_corpus), and
 * the handles are joined by an EXCHANGE (section "multi-GPU" below): ggs_attach_rccl* (RCCL over xGMI, one process per
 * GPU or one process for all), or ggs_attach_exchange (caller-supplied transport).  With an exchange attached the
 * sweep itself contains the per-sweep merge of the reference (UPLDA:1107-1221; ADLDA.java:302-332), in the form
 * SURVEY.md 8e prefers: reduce-scatter of the int32 counts by TOPIC SLICE (even-split rule of
 * randomscan/topic/EvenSplitTopicBatchBuilder.java:28-39), Phi drawn for the rank's own topics only (the topic-parallel
 * samplePhi of GGS:139-171 with one batch per GPU), all-gather of the fp64 Phi slices.  Results are bit-identical to
 * one handle over the whole corpus: the Philox element ids are global (token, document*K+k, k*V+v).
 */
#ifndef GGS_HIP_H
#define GGS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GGS_ABI_VERSION 6

typedef struct ggs_handle ggs_handle;

enum {
  GGS_OK = 0,
  GGS_ERR_NEGATIVE_COUNT = 1, /* IllegalStateException "Invalid count!" GGS:84-85; UPLDA:475-481 */
  GGS_ERR_INVALID_TOPIC = 2,  /* IllegalStateException "Topic sampled is invalid!" GGS:116-118    */
  GGS_ERR_RNG_EXHAUSTED = 3,  /* a rejection loop used more than GGS_MAX_BLOCKS Philox blocks      */
  GGS_ERR_BAD_ARG = 4,        /* IllegalArgumentException (e.g. ParallelRandoms.java:61-63)        */
  GGS_ERR_HIP = 5,            /* a HIP runtime call failed; text has the hipError string           */
  GGS_ERR_STATE = 6,          /* call order violated (e.g. sweep before set_corpus)                */
  GGS_ERR_UNSUPPORTED = 7,
  GGS_ERR_INVARIANT = 8       /* paranoid check failed (UPLDA:299-338)                             */
};

enum {
  GGS_FLAG_PARANOID = 1 << 0,     /* run ggs_check_invariants after every sweep
                                     (ParanoidUncollapsedParallelLDA.java:14-55)   */
  GGS_FLAG_SAVE_PHI_MEAN = 1 << 1,/* cfg key save_phi_mean, UPLDA:205,1331-1335    */
  GGS_FLAG_COLLAPSED = 1 << 3,    /* scheme=collapsed (SerialCollapsedLDA; the conditional is MSLDA:158-226): no theta, no Phi:
                                     score = (alpha_k + n_dk)*((beta + n_wk)/(betaSum + n_k)).  ggs_sweep runs the PARALLEL
                                     schedule -- documents side by side against the sweep-start counts minus the token
                                     itself, merged after the sweep (AD-LDA semantics, ADLDA.java:176-332; approximate as
                                     ADLDA is, and what a doc-sharded run exchanges is again the count buffer);
                                     ggs_collapsed_serial_sweep runs the reference's own serial chain.  ggs_get_phi returns
                                     the point estimate (beta + n_wk)/(betaSum + n_k); ggs_get_theta, ggs_log_posterior and
                                     ggs_sample_z_given_phi do not apply.  K up to 4096, any document length (as pcgs). */
  GGS_FLAG_PCGS = 1 << 2,         /* scheme=pcgs (LDAPartiallyCollapsedGibbsSampler): the z step is UPLDA:1466-1544,
                                     score = (n_dk + alpha_k)*phi[k][w], sequential inside a document; no theta draw;
                                     counts, Phi draw and exchange exactly as for ggs.  Any K up to 4096 and any
                                     document length: up to 176 topics (scheme collapsed: 96 -- the measured break-even
                                     points) one LANE owns a document (64 documents per wave, int16 counts in LDS); above
                                     that, or when a document has 32768 tokens or more, one WAVE owns a document (int32
                                     counts, the topics spread over the lanes). */
  GGS_FLAG_POLYAURN = 1 << 4,     /* scheme=polyaurn (PolyaUrnSpaliasLDA, ParallelLDA.java:444-447; ABI version 6): the z step of
                                     pcgs (implied: GGS_FLAG_PCGS is set internally), except that a document of one token, or
                                     a token whose scores sum to 0 (its word's Phi column is all zero), draws floor(U * K) with
                                     the token's own uniform U (PolyaUrnSpaliasLDA.java:261-278).  Phi (initial and per sweep)
                                     is drawn as Poisson counts X_kv ~ Poisson(beta + n_kv) normalised by their integer row sum,
                                     a row of sum 0 all zero (PolyaUrnDirichletFixedCoeffPoisson.java:17-40; UPLDA:1287-1294 for
                                     the initial draw): n_kv < alias_poisson_threshold by inverse CDF over the pmf truncated to
                                     2 * threshold terms and renormalised, larger counts as max(0, floor(sqrt(l) * g + l + 0.5))
                                     with l = beta + n_kv and the element's Gaussian g (PolyaUrnDirichlet.java:102-107, the
                                     negative draw clamped to 0).  Phi has exact zeros.  With GGS_FLAG_COLLAPSED: GGS_ERR_BAD_ARG. */
  GGS_FLAG_SPALIAS = 1 << 5,      /* scheme=spalias (SpaliasUncollapsedParallelLDA, ParallelLDA.java:439-442): the pcgs model
                                     (implied: GGS_FLAG_PCGS is set internally; Phi, counts, phi mean and exchange exactly as pcgs)
                                     with the z step's conditional split into alpha_k * phi[k][w], drawn in O(1) from a Walker alias
                                     table per word, and n_dk * phi[k][w], walked over the document's non-zero topics only: the
                                     same distribution, O(nnz_d) per token, a different draw from the same uniform.  The tables are
                                     rebuilt whenever Phi changes (ggs_init_phi, every sweep, ggs_set_phi); ggs_get_alias_tables
                                     reads them back.  K up to 4096, any document length.  With GGS_FLAG_COLLAPSED or
                                     GGS_FLAG_POLYAURN: GGS_ERR_BAD_ARG.  A new bit, not a new ABI version. */
  GGS_FLAG_LIGHTPCLDA = 1 << 6,   /* scheme=lightpclda (LightPCLDA, ParallelLDA.java:469-473; LightPCLDA.java:86-221): the pcgs model
                                     (implied: GGS_FLAG_PCGS is set internally; Phi, counts, phi mean and exchange exactly as pcgs)
                                     with a Metropolis-Hastings z step, O(1) per token: a proposal from the word's alias table
                                     and one from the document's own indicator array, each accepted on a ratio of a few numbers.
                                     The tables are spalias's, pi[k] = phi[k][w] * alpha[k] (the reference's PhiTableBuilderFactory,
                                     LightPCLDA.java:50-83, is never installed), rebuilt wherever spalias rebuilds them;
                                     ggs_get_alias_tables reads them back, ggs_get_mh_stats the acceptance counters.  The four
                                     uniforms of a token are the two doubles of Philox block 0 and the two of block 1 of its Z
                                     stream, taken whether or not the branch that uses them runs.  When the document proposal
                                     equals the current topic the new topic is the token's OLD one, as in the reference
                                     (LightPCLDA.java:115, 175).  An alias draw or an alpha-branch topic equal to K is
                                     GGS_ERR_INVALID_TOPIC.  The chain is approximate by design and is not repaired.
                                     K up to 4096, any document length.  With GGS_FLAG_COLLAPSED, GGS_FLAG_POLYAURN or
                                     GGS_FLAG_SPALIAS: GGS_ERR_BAD_ARG.  A new bit, not a new ABI version. */
  GGS_FLAG_POLYAURN_SPARSE = 1 << 7,/* scheme=polyaurn_sparse (PolyaUrnSpaliasLDA.sampleTopicAssignmentsParallel,
                                     PolyaUrnSpaliasLDA.java:180-334): polyaurn's model (implied: GGS_FLAG_PCGS is set internally; Phi
                                     initial and per sweep, counts, tokensPerTopic, phi mean and exchange exactly as under
                                     GGS_FLAG_POLYAURN, alias_poisson_threshold read the same way) with the doubly sparse z step the
                                     reference builds for Phi's exact zeros.  After every Phi (ggs_init_phi, every sweep, ggs_set_phi)
                                     spalias's alias tables are rebuilt and, per word w, nzw[w] = the topics k with
                                     phi[k][w] != 0.0 in ascending k, nw[w] their number (ggs_get_word_topic_lists);
                                     ggs_sample_z_given_phi reuses what ggs_set_phi built.  The document keeps spalias's state:
                                     counts cnt[K] and the list of its non-zero topics (a topic appended on first occurrence, a
                                     removed topic replaced by the last entry).  Per token, with its uniform U (purpose Z, element =
                                     global token index), all in fp64 in this order: the old topic is removed; nd = the document
                                     list's length; the candidates c_0..c_{n-1} are nzw[w] if nw[w] < nd (:261-267), otherwise, a tie
                                     included, the document's list.  n == 0 (a one-token document, an all-zero Phi column):
                                     topic = min((int)(U * K), K - 1) (:276-277; the reference does not clamp, it throws when
                                     floor(U * K) reaches K).  Otherwise cum[0] = (double)cnt[c_0] * phi[c_0][w],
                                     cum[i] = (double)cnt[c_i] * phi[c_i][w] + cum[i-1], sum = cum[n-1], tn = typeNorm[w]; if
                                     U < tn / (tn + sum) the topic is the alias draw sample(w, U + (sum * U) / tn) (i == K:
                                     GGS_ERR_INVALID_TOPIC); else ul = U * (tn + sum) - tn and the topic is the candidate at the
                                     smallest i with ul <= cum[i], the last candidate if there is none (ours, as under
                                     GGS_FLAG_SPALIAS; so for 0 / 0, which fails the first comparison).  A word-list candidate
                                     with cnt == 0 scores 0.0 and is walked like any other.  ggs_get_sparse_stats counts which list
                                     the tokens took.  K up to 4096, any document length.  With GGS_FLAG_COLLAPSED,
                                     GGS_FLAG_POLYAURN, GGS_FLAG_SPALIAS or GGS_FLAG_LIGHTPCLDA: GGS_ERR_BAD_ARG.  A new bit, not a
                                     new ABI version. */
  GGS_FLAG_LIGHTCOLLAPSED = 1 << 8, /* scheme=lightcollapsed (CollapsedLightLDA, ParallelLDA.java:429-433): the collapsed model --
                                     no theta, no Phi; counts, tokensPerTopic, merge, exchange, ggs_get_phi (the point estimate),
                                     the likelihoods and ggs_check_invariants exactly as under GGS_FLAG_COLLAPSED -- under the
                                     LightLDA z step: per token a word proposal from the word's alias table over the counts and
                                     a document proposal from the document's indicator array, each accepted on a product of
                                     count quotients (calculateWordAcceptanceProbability, calculateDocumentAcceptanceProbability,
                                     CollapsedLightLDA.java:1050-1128; the formulas term by term in ggs_z_lightcollapsed.hpp).  The
                                     schedule is GGS_FLAG_COLLAPSED's parallel one, AD-LDA with one worker per document: a token
                                     is sampled against the sweep-start counts with only itself moved.  At the head of every
                                     sweep, per word w: the ascending list of its topics with n_wk > 0 (ggs_get_word_topic_lists),
                                     p_i = n_wk / ((double)n_k + betaSum), type_norm[w] = their i-order sum, and the alias table
                                     of the nw[w] values p_i / type_norm[w] (ggs_get_alias_tables).  The uniforms are
                                     GGS_FLAG_LIGHTPCLDA's four; ggs_get_mh_stats keeps the same three counters.  A table draw with
                                     i == nw[w] and a beta- or alpha-branch topic == K: GGS_ERR_INVALID_TOPIC.
                                     ggs_sample_z_given_phi, ggs_log_posterior, ggs_set_phi and ggs_get_theta:
                                     GGS_ERR_UNSUPPORTED; ggs_collapsed_serial_sweep: GGS_ERR_STATE.  The chain is approximate as
                                     the reference writes it and is not repaired.  K up to 4096, any document
                                     length.  With any of GGS_FLAG_COLLAPSED, GGS_FLAG_PCGS, GGS_FLAG_POLYAURN, GGS_FLAG_SPALIAS,
                                     GGS_FLAG_LIGHTPCLDA, GGS_FLAG_POLYAURN_SPARSE: GGS_ERR_BAD_ARG.  A new bit, not a new ABI
                                     version. */
  GGS_FLAG_NZVSSPALIAS = 1 << 9,  /* scheme=nzvsspalias (NZVSSpaliasUncollapsedParallelLDA, ParallelLDA.java; types/VSDirichlet.java:34-112):
                                     the pcgs model (implied: GGS_FLAG_PCGS is set internally; initial Phi, counts and alias tables as
                                     under GGS_FLAG_SPALIAS) with a VARIABLE-SELECTION Dirichlet for Phi, which has exact zeros.
                                     Phi of a sweep, per topic k: n_k = the topic's int token count, s = the zeros of the old row; the
                                     cells are visited in index order.  A cell with a count is drawn and leaves s alone.  A cell
                                     without one computes a = s * beta, r = exp(lgS(a + beta) + lgS(a + n_k) - lgS(a + beta + n_k)
                                     - lgS(a)) * (pi / (1 - pi)), p = r / (1 + r) (lgS = Dirichlet.logGammaStirling, exp = StrictMath's)
                                     and takes U, the first uniform of the stream GGS_PURPOSE_VS, element k*V + v: U > p leaves it
                                     UNDRAWN, +0.0 (s++ if the old cell was not 0.0), otherwise it is drawn (s-- if it was).  s == 0:
                                     p = 0 with n_k > 0 (lgS(0) = +inf), NaN with n_k == 0, and U > NaN is false: drawn.  p > 1 or
                                     p < 0 (the reference throws): GGS_ERR_INVARIANT.  A drawn cell holds Gamma(n + beta) from the stream
                                     GGS_PURPOSE_PHI of element k*V + v (an undrawn cell uses none of it), no clamp: an underflow to 0.0
                                     is a drawn cell that holds 0.0.  Every cell is divided by the row's index-order sum; ours: a row
                                     whose sum is 0 becomes all +0.0 (the reference writes NaN).  pi is
                                     ggs_set_variable_selection_prior's, 0.5 by default.  The device solves the chain in parallel and
                                     proves the sequential result (csrc/ggs_phi_vs.hpp); ggs_get_vs_stats counts its rounds.
                                     Lists (ggs_get_word_topic_lists): after a sweep nzw[w] = the topics whose cell (k, w) was DRAWN,
                                     ascending -- not phi != 0.0; after ggs_init_phi and the redraw of ggs_set_z every list is empty, as
                                     in the reference, so the first z step draws from the alias tables alone; after ggs_set_phi
                                     (ours; the reference leaves them stale) the cells with phi != 0.0.
                                     The z step is GGS_FLAG_POLYAURN_SPARSE's, formula for formula, except that a token without a
                                     candidate (n == 0) draws sample(w, U) from its word's alias table (:252-254; i == K:
                                     GGS_ERR_INVALID_TOPIC).  ggs_get_sparse_stats counts such tokens in out[2].
                                     With GGS_FLAG_SAVE_PHI_MEAN the mean stays zero while n_sampled advances: the reference's
                                     loopOverTopics override never adds to it.  With an exchange a rank runs the indicator chain of
                                     its own topic slice (counts [V][Ksm] from the reduce-scatter, the old Phi from its full phiT)
                                     and every topic's drawn set reaches every rank inside the all-gathers of the gammas: an undrawn
                                     cell travels as -0.0, a drawn one that underflowed as +0.0, and the sign is cleared on arrival.
                                     Results are bit-identical to one handle.  K up to 4096, any document length.  With any of GGS_FLAG_COLLAPSED,
                                     GGS_FLAG_POLYAURN, GGS_FLAG_SPALIAS, GGS_FLAG_LIGHTPCLDA, GGS_FLAG_POLYAURN_SPARSE,
                                     GGS_FLAG_LIGHTCOLLAPSED: GGS_ERR_BAD_ARG.  A new bit, not a new ABI version. */
  GGS_FLAG_ADLDA = 1 << 10,       /* scheme=adlda (ADLDA, ParallelLDA.java:409-412; MyWorkerRunnable.sampleTopicsForOneDoc,
                                     MyWorkerRunnable.java:32-409): the collapsed model -- no theta, no Phi; ggs_get_phi, the exchange,
                                     the likelihoods and ggs_check_invariants exactly as under GGS_FLAG_COLLAPSED -- under the SparseLDA
                                     bucket z step of Yao, Mimno and McCallum: the exact conditional of GGS_FLAG_COLLAPSED's parallel
                                     schedule (AD-LDA, one worker per document, every token against the counts N, T of the sweep start
                                     minus itself) at O(nnz_d + nnz_w) per token.  At the head of every sweep: den0[k] = (double)T[k] +
                                     betaSum; S0 = the k-order sum from 0.0 of (alpha_k * beta) / den0[k]; per word the ascending list
                                     L_w of its topics with N[w][k] > 0 (ggs_get_word_topic_lists).  Per token (word w, old topic z0,
                                     U the first uniform of Philox block 0 of its GGS_PURPOSE_Z stream; counts converted to double,
                                     every expression left to right): n_d[z0]-- (a count of 0 leaves the document's list, the last
                                     entry fills the hole); den(k) = (double)(T[k] - [k == z0]) + betaSum, G'(k) = N[w][k] - [k == z0];
                                     S = S0 - (alpha_z0 * beta) / den0[z0] + (alpha_z0 * beta) / den(z0); R = the list-order sum of
                                     (beta * n_d[c]) / den(c) over the document's list; Q = the list-order sum over L_w of score_j =
                                     ((alpha_k + n_d[k]) / den(k)) * G'(k); sample = U * (S + R + Q).  sample < Q: i = -1, while
                                     sample > 0: i++, sample -= score_i; the topic is L_w[i] (past the last entry:
                                     GGS_ERR_INVALID_TOPIC, clamped to it).  Else sample -= Q; sample < R: sample /= beta, over the
                                     document's list sample -= n_d[c] / den(c), the first c with sample <= 0.0, K - 1 if none (no
                                     error).  Else sample -= R, sample /= beta, k = 0, sample -= alpha_0 / den(0), while sample > 0.0:
                                     k++, sample -= alpha_k / den(k) (k == K: GGS_ERR_INVALID_TOPIC, clamped to K - 1).  Then
                                     n_d[new]++, z = new.  ggs_get_sparse_stats counts the buckets.  ggs_sample_z_given_phi,
                                     ggs_get_alias_tables and ggs_get_mh_stats: GGS_ERR_UNSUPPORTED; ggs_collapsed_serial_sweep:
                                     GGS_ERR_STATE.  Sharded runs are bit-identical to one handle.  K up to 4096, any document
                                     length.  With any of GGS_FLAG_COLLAPSED, GGS_FLAG_PCGS, GGS_FLAG_POLYAURN, GGS_FLAG_SPALIAS,
                                     GGS_FLAG_LIGHTPCLDA, GGS_FLAG_POLYAURN_SPARSE, GGS_FLAG_LIGHTCOLLAPSED, GGS_FLAG_NZVSSPALIAS:
                                     GGS_ERR_BAD_ARG.  A new bit, not a new ABI version. */
  GGS_FLAG_LIGHTPCLDAW2 = 1 << 11 /* scheme=lightpcldaw2 (LightPCLDAtypeTopicProposal, ParallelLDA.createModel's "lightpcldaw2";
                                     LightPCLDAtypeTopicProposal.java:101-274): the pcgs model (implied: GGS_FLAG_PCGS is set
                                     internally; Phi, counts, merge, phi mean and exchange exactly as pcgs) under the LightLDA z step
                                     with GGS_FLAG_LIGHTCOLLAPSED's word proposal.  At the head of every z step, on the corpus-wide
                                     sweep-start counts (with an exchange: gathered there), per word w: the ascending list of its
                                     topics with n_wk > 0 (ggs_get_word_topic_lists), p_i = n_wk / ((double)n_k + betaSum),
                                     type_norm[w] their i-order sum, the alias table of the nw[w] values p_i / type_norm[w]
                                     (ggs_get_alias_tables) and tokensPerType[w] -- the tables the class declares
                                     (TypeTopicTableBuilderFactory, :72-77; a JVM run never installs them).  Per
                                     token, G = the sweep-start counts, nothing moved for the token in flight, bhat[k] =
                                     (double)n_k + betaSum: the word proposal t as under GGS_FLAG_LIGHTCOLLAPSED; if t != s,
                                     pi_w = (phi[t][w] * (alpha[s] + ni[t]) * (beta + G[w][s]) * bhat[t]) /
                                     (phi[s][w] * (alpha[s] + ni[s]) * (beta + G[w][t]) * bhat[s]), each product left to right
                                     (:270-272); then GGS_FLAG_LIGHTPCLDA's document proposal, word for word, the token returning
                                     to its OLD topic when the proposal equals the current one.  The uniforms are
                                     GGS_FLAG_LIGHTPCLDA's four; ggs_get_mh_stats keeps the same three counters.  A table draw with
                                     i == nw[w] and a beta- or alpha-branch topic == K: GGS_ERR_INVALID_TOPIC.
                                     ggs_sample_z_given_phi as under GGS_FLAG_LIGHTPCLDA, the tables rebuilt from the merged counts
                                     at the head of each iteration.  ggs_get_theta: GGS_ERR_UNSUPPORTED (no theta is kept; the
                                     diagnostics that draw one allocate it when first asked).  The chain is approximate as the
                                     reference writes it and is not repaired.  Sharded runs are bit-identical to one handle.
                                     K up to 4096, any document length.  With any other scheme flag but GGS_FLAG_PCGS:
                                     GGS_ERR_BAD_ARG, answered before a device is asked for.  A new bit, not a new ABI version. */
};

/* RNG stream addressing.  The reference draws from ThreadLocalRandom and a
 * nanoTime-seeded xorshift (GGS:107, util/XORShiftRandom.java:7) and is not
 * reproducible; this library defines a counter-based stream instead:
 * Philox4x32-10, key = (seed lo, seed hi),
 * counter = (elem lo, elem hi, purpose << 24 | block, iteration). */
enum {
  GGS_PURPOSE_Z = 1,       /* elem = global token index          */
  GGS_PURPOSE_THETA = 2,   /* elem = global doc index * K + k    */
  GGS_PURPOSE_PHI = 3,     /* elem = k * V + v                   */
  GGS_PURPOSE_INIT_PHI = 4,/* elem = k * V + v                   */
  GGS_PURPOSE_HELDOUT = 5, /* elem = global test doc * numParticles + particle; one uniform per in-vocabulary token */
  GGS_PURPOSE_VS = 6       /* elem = k * V + v; one uniform: the variable-selection indicator (GGS_FLAG_NZVSSPALIAS) */
};
#define GGS_MAX_BLOCKS 4096

typedef struct ggs_config {
  int32_t struct_size;    /* = sizeof(ggs_config), for ABI growth                              */
  int32_t num_topics;     /* cfg key "topics"; MSLDA:126-127                                   */
  int32_t num_types;      /* alphabet size V; UPLDA:361                                        */
  int32_t device_id;      /* HIP device ordinal this handle lives on                           */
  const double *alpha;    /* K values, or NULL to use alpha_scalar for every topic (MSLDA:129-135) */
  double alpha_scalar;    /* cfg key "alpha"                                                   */
  double beta;            /* cfg key "beta"; MSLDA:136                                         */
  uint64_t seed;          /* key of the Philox streams                                         */
  int32_t flags;          /* GGS_FLAG_*                                                        */
  int32_t phi_burn_in;    /* iterations: (phi_mean_burnin/100)*iterations, UPLDA:206-207       */
  int32_t phi_mean_thin;  /* cfg key phi_mean_thin, UPLDA:208                                  */
  int32_t alias_poisson_threshold; /* cfg key alias_poisson_threshold (ParsedLDAConfiguration.java:480-482; default 100,
                             LDAConfiguration.java:44): counts below it draw their Poisson variate from a table.  Read only
                             under GGS_FLAG_POLYAURN and GGS_FLAG_POLYAURN_SPARSE: 0 means 100, 1..512 allowed, anything else GGS_ERR_BAD_ARG.  (The
                             field was `reserved` before ABI version 6; layout and struct_size are unchanged.) */
} ggs_config;

typedef struct ggs_timings {
  double theta_ms;  /* cumulative: per-document theta draw (GGS:57-72)                         */
  double z_ms;      /* cumulative: token loop (GGS:79-130)                                     */
  double merge_ms;  /* cumulative: count rebuild, the device form of updateCounts (UPLDA:1107-1221) */
  double phi_ms;    /* cumulative: samplePhi (GGS:139-198); with an exchange: this rank's topic slice + the repack */
  int64_t sweeps;
  int64_t tokens_sampled;
  double exchange_ms; /* cumulative: the collectives of an attached exchange (count reduce-scatter + Phi all-gather);
                         0 without one.  ABI version 2. */
  double exchange_rs_ms; /* ... of which the count reduce-scatter.  ABI version 3. */
  double exchange_ag_ms; /* ... of which what the sweep WAITS for of the Phi all-gathers: the first half of the gammas
                            travels under the draw of the second half, so this is the time from the end of the slice's
                            draw to both halves being in.  exchange_ms = exchange_rs_ms + exchange_ag_ms.  ABI version 3. */
} ggs_timings;

/* ---- lifecycle ------------------------------------------------------------ */
/* replaces: new LDAGroupedGibbsSampler(config) (GGS:25-27, UPLDA ctor :134-215) */
int ggs_create(const ggs_config *cfg, ggs_handle **out);
void ggs_destroy(ggs_handle *h);
const char *ggs_last_error(const ggs_handle *h);
int ggs_abi_version(void);
/* Run every kernel on this hipStream_t (NULL = the legacy default stream). */
int ggs_set_stream(ggs_handle *h, void *hip_stream);

/* ---- corpus and initial state --------------------------------------------- */
/* replaces: the data part of addInstances (UPLDA:357-456, GGS:33-37): CSR of
 * FeatureSequence.getFeatures() in instance order.  doc_base / tok_base are the
 * global indices of this shard's first document / token (0 for one GPU); they
 * only enter the RNG element ids, so a doc-sharded run draws exactly what a
 * one-GPU run draws. */
int ggs_set_corpus(ggs_handle *h, int64_t num_docs, const int64_t *doc_ptr /*D+1*/,
                   const int32_t *tokens /*N*/, int64_t doc_base, int64_t tok_base);
/* replaces: initialDrawTopicIndicator loop (UPLDA:398-406,458-460): z0 =
 * java.util.Random(seed).nextInt(K) in (doc, position) order, counts rebuilt.
 * Sequential stream => only valid on an unsharded corpus (tok_base == 0). */
int ggs_init_z_java_lcg(ggs_handle *h, int32_t seed);
/* Host utility: the first n values of java.util.Random(seed).nextInt(bound) -- what a
 * doc-sharded start-up slices per rank before ggs_set_z (the stream is sequential). */
int ggs_java_lcg_next_ints(int32_t seed, int32_t bound, int64_t n, int32_t *out);
/* replaces: setZIndicators (UPLDA:1797-1843): rebuild counts from z, zero the
 * deltas and (redraw_phi != 0) re-draw Phi as initialSamplePhi does. */
int ggs_set_z(ggs_handle *h, const int32_t *z /*N*/, int32_t redraw_phi);
/* replaces: initialSamplePhi (UPLDA:1287-1294 -> MarsagliaSparseDirichlet.java:31-55) */
int ggs_init_phi(ggs_handle *h);
/* currentIteration (UPLDA:646); enters the RNG counters as their fourth word.  Iterations are 0 ... INT32_MAX:
 * ggs_set_iteration with a negative number returns GGS_ERR_BAD_ARG and leaves the handle as it was.  Every call that steps
 * the iteration (ggs_sweep, ggs_sweep_begin, ggs_sample_z_given_phi, ggs_collapsed_serial_sweep, ggs_group_sweep) returns
 * GGS_ERR_STATE, launches nothing and changes nothing when iteration + its number of steps would pass INT32_MAX -- a call
 * of several sweeps is refused as a whole, not after the sweeps that still fit. */
int ggs_set_iteration(ggs_handle *h, int32_t iteration);
int ggs_get_iteration(const ggs_handle *h, int32_t *iteration);
/* ---- a handle with a history: resume, rewind, reuse --------------------------------------------------------------------
 * The streams are keyed by (seed, iteration, purpose, element), so a chain is continued exactly from its EXPORTED STATE:
 * z (ggs_get_z), Phi (ggs_get_phi) and the iteration number -- on a fresh handle of the same configuration (flags, alpha, beta,
 * seed, alias_poisson_threshold, the topic priors, the variable-selection prior) and corpus, on the handle itself, or on the
 * ranks of an exchange (each rank its slice of z, every rank the whole Phi): ggs_set_z(z, 0), ggs_set_phi, ggs_set_iteration,
 * in any order, then sweeps.  The count-form schemes (collapsed, lightcollapsed, adlda) have no Phi: their state is z and the
 * iteration number, and ggs_init_phi (tokensPerTopic; with an exchange the merge of the ranks' counts) follows ggs_set_z.
 * theta is not state: it is drawn from z for the iteration at hand; one drawn ahead, beside the previous sweep's Phi draw,
 * is used only by a z step of the iteration it was drawn for and is dropped by ggs_set_z, ggs_init_z_java_lcg and
 * ggs_set_corpus.  What each call does to the rest of a handle that has run before:
 *   the iteration number  is the caller's: only the sweeps (+1 each) and ggs_set_iteration change it.  ggs_set_corpus, ggs_set_z
 *       and ggs_set_phi leave it: a second corpus goes on counting where the first stopped unless ggs_set_iteration is called.
 *   the phi mean and n_sampled (GGS_FLAG_SAVE_PHI_MEAN)  belong to one corpus' chain on one handle: ggs_set_corpus zeroes both;
 *       ggs_set_phi restarts the running sum while n_sampled keeps counting (UPLDA:1897-1902), so the mean reported after it is
 *       (the Phi accepted since) / (all Phi accepted since ggs_set_corpus); ggs_set_z and ggs_set_iteration leave both.  A Phi is
 *       accepted when phi_burn_in > 0, iteration > phi_burn_in and iteration % phi_mean_thin == 0, whatever came before.
 *   the topic priors and the variable-selection prior  are configuration: they survive ggs_set_corpus, ggs_set_z and
 *       ggs_set_iteration; they can be set (again) whenever the handle has no Phi, which after ggs_set_corpus it has not.
 *   the cumulative counters (ggs_get_mh_stats, ggs_get_sparse_stats)  start at 0 at ggs_set_corpus and only grow: none of
 *       ggs_set_z, ggs_set_phi, ggs_set_iteration resets them.  (ggs_get_vs_stats describes the last draw, see there.)
 *   alias tables and the words' lists  follow every Phi, a set one included; nzvsspalias' lists are the drawn cells after a
 *       sweep and the cells with phi != 0.0 after ggs_set_phi: the resumed chain is the exporting handle's exactly when no drawn
 *       cell holds 0.0 (a gamma draw that underflowed: beta of 0.5 does not, beta of 0.001 does), otherwise a token may walk
 *       the other list and the chains may part.
 *   ggs_set_corpus  besides: no Phi and no sweep in progress, the global token count back to the handle's own, the z form
 *       timed again, every table, list and launch geometry the new corpus'.  A run on a reused handle is, bit for bit and in
 *       everything the getters return, the run of a fresh handle that was given the same iteration number.
 *   ggs_set_hyperparameters  changes the configuration itself: from the next z step on the handle is a fresh handle of the NEW alpha,
 *       beta and betaSum that was given this handle's exported state.  It drops a theta drawn ahead (drawn under the old alpha), as
 *       ggs_set_z does; tables over alpha * phi are rebuilt from the Phi that stands; the iteration, the phi mean, the priors and the
 *       cumulative counters are left alone.
 * tests/test_handle_lifecycle_gpu.py pins each of these for every scheme. */

/* ---- the sweep ------------------------------------------------------------- */
/* replaces one loop body of sample() (UPLDA:645-687) n_sweeps times:
 * loopOverBatches (GGS:47-132 for every document), updateCounts, samplePhi.
 * Returns after the device is idle.  n_sweeps = 1 keeps the Java per-iteration
 * abort / exec_time / diagnostics loop in the caller. */
int ggs_sweep(ggs_handle *h, int32_t n_sweeps);
/* The same, split where a doc-sharded run exchanges counts:
 *   begin = ++iteration, theta draw + z draw + this shard's counts (UPLDA:660, and the
 *           local half of updateCounts)
 *   [caller sum-all-reduces the counts buffer across shards -- see ggs_counts_device_ptr]
 *   end   = samplePhi on the corpus-wide counts (UPLDA:664-687) */
int ggs_sweep_begin(ggs_handle *h);
int ggs_sweep_end(ggs_handle *h);
/* ggs_sweep_end without the wait: the Phi draw is enqueued and the call returns; errors the sweep flags on the
 * device (they are sticky) and its phase times surface at the next ggs_sweep_end / ggs_sweep / ggs_synchronize-
 * then-getter.  For a doc-sharded loop that exchanges counts every sweep but looks at the result every n. */
int ggs_sweep_end_async(ggs_handle *h);
/* replaces: SerialCollapsedLDA.sample's loop over documents (SerialCollapsedLDA.java:159-172 -> sampleTopicsForOneDoc,
 * MSLDA:158-226) n_sweeps times, in the reference's own SERIAL schedule: one chain over all tokens, counts moved in
 * place, uniforms from the sampler's ONE java.util.Random: after ggs_init_z_java_lcg(h, seed) the stream simply
 * continues where the initial topics left it -- SerialCollapsedLDA draws both from the same Randoms(seed) object
 * (SerialCollapsedLDA.java:60-65,789; MSLDA:206) -- and java_seed is not looked at; after ggs_set_z a new
 * Random(java_seed) is created at the first call and carried on.  Needs GGS_FLAG_COLLAPSED, an unsharded corpus and no exchange.  One wave does it all: for parity on small
 * corpora (BASELINE config 1), not for throughput. */
int ggs_collapsed_serial_sweep(ggs_handle *h, int32_t java_seed, int32_t n_sweeps);
/* replaces: sampleZGivenPhi (UPLDA:975-1014): z step + updateCounts, Phi kept */
int ggs_sample_z_given_phi(ggs_handle *h, int32_t n_sweeps);
/* Device pointer / element count of the int32 [V][K] type-topic counts
 * (typeTopicCounts, MSLDA:73) -- the ONE buffer a doc-sharded run exchanges.  After
 * ggs_sweep_begin (and after ggs_set_z(h, z, 0) at start-up) it holds THIS shard's counts;
 * the caller sum-all-reduces it in place over the shards (RCCL) and then calls ggs_sweep_end
 * (resp. ggs_init_phi).  This replaces the Java merge of the thread-shared AtomicInteger
 * deltas (batchLocalTopicTypeUpdates, UPLDA:102,1107-1221; ADLDA's sumTypeTopicCounts,
 * ADLDA.java:302): n_wk(new) = n_wk(old) + sum of deltas = sum over shards of the local
 * (word, z) histograms -- the same integers. */
int ggs_counts_device_ptr(ggs_handle *h, void **dev_ptr, int64_t *num_elems);   /* GGS_ERR_STATE with an exchange attached */
/* Corpus-wide token count (all shards); what ggs_check_invariants expects the
 * counts to sum to.  Defaults to this handle's own token count. */
int ggs_set_global_token_count(ggs_handle *h, int64_t n_tokens);
/* Block until everything queued on the handle's stream has finished; surfaces
 * device-side error flags (what Java throws from the worker threads). */
int ggs_synchronize(ggs_handle *h);

/* ---- multi-GPU: the exchange --------------------------------------------------------------------------------------
 * Replaces the thread-shared merge of the reference -- updateCounts/updateTopics (UPLDA:1107-1221), the blocking queue
 * of topic batches in samplePhi (GGS:139-171), ADLDA's sumTypeTopicCounts + copy-back (ADLDA.java:302-332) -- by three
 * collectives over `nranks` handles, rank r owning the documents of shard r and the TOPICS of slice r
 * (sizes K/nranks + (K % nranks > r), EvenSplitTopicBatchBuilder.java:28-39; Ksm = the largest slice):
 *   reduce_scatter_i32  send int32 [nranks][V][Ksm] (this shard's (word, topic) histogram, slice-major, zero padded)
 *                       -> recv int32 [V][Ksm] = the corpus-wide counts of the rank's own topics.  Once per sweep, on the
 *                       handle's stream.  (Or the sparse form in its place: all_gather_i32 of nranks pair counts, then
 *                       all_to_all_v_i32 of (cell, count) pairs -- ggs_set_count_exchange.)
 *   all_gather_f64      TWICE per Phi phase when the vocabulary has 16 or more 64-row segments (V >= 961), with DIFFERENT
 *                       counts and on DIFFERENT streams of the one handle, never concurrently: what travels is the rank's
 *                       UNNORMALISED gamma draws [V][Ksm] in two halves of the vocabulary -- first the rows below v_split
 *                       (send_count = v_split * Ksm) on the handle's high-priority COMMUNICATION stream, under the draw of
 *                       the second half; then, behind it on the handle's own stream, the rows from v_split on followed by
 *                       the slice's Ksm column sums (send_count = (V - v_split) * Ksm + Ksm).  The receiver divides by the
 *                       owner's sum while repacking (the division of ParallelDirichlet.java:60-66 on the same operands).
 *                       A short vocabulary goes in one call of (V * Ksm + Ksm) elements.  A transport must therefore take
 *                       count and stream from each call (no cached stream, no staging sized for one fixed count).
 *   all_gather_i32      the same for the count slices ([V][Ksm] per rank) -- only when a getter / diagnostic needs corpus-wide
 *                       counts -- and, with the sparse count exchange, for the nranks pair counts of every sweep
 * Attach after ggs_create and before ggs_set_corpus.  From then on ggs_sweep / ggs_sweep_end / ggs_init_phi /
 * ggs_set_z(redraw) / ggs_sample_z_given_phi contain the collectives, and every call that reads corpus-wide counts
 * (ggs_get_type_topic_counts, ggs_get_topic_totals, ggs_check_invariants, ggs_model_log_likelihood,
 * ggs_heldout_log_likelihood) gathers them first: all of these are COLLECTIVE calls -- every rank makes them in the
 * same order.  The handle then runs on a stream of its own (not the legacy default stream) and orders the collectives
 * on it; nothing relies on another library's current-stream convention. */
typedef struct ggs_exchange_ops {
  int32_t struct_size;   /* = sizeof(ggs_exchange_ops) */
  int32_t reserved;
  void *ctx;
  /* Each callback enqueues (or performs) the collective in order behind the work already queued on hip_stream and
   * returns 0 on success; counts are ELEMENTS per rank. */
  int (*reduce_scatter_i32)(void *ctx, const void *send, void *recv, int64_t recv_count, void *hip_stream);
  int (*all_gather_f64)(void *ctx, const void *send, void *recv, int64_t send_count, void *hip_stream);
  int (*all_gather_i32)(void *ctx, const void *send, void *recv, int64_t send_count, void *hip_stream);
  /* Optional (ABI version 4; may be NULL, and a table of the version-3 size -- without this member -- is accepted): the
   * SPARSE count exchange.  Rank r receives the recv_counts[s] int32 elements rank s addressed to it, at recv + recv_offsets[s];
   * it sends send_counts[d] elements from send + send_offsets[d] to every rank d (its own block included: a local copy).
   * The four arrays have nranks entries, live in HOST memory and are only read during the call; the counts agree pairwise
   * (the library exchanges them beforehand with all_gather_i32).  Used when a rank's (word, topic) histogram is sparse --
   * BASELINE config 5: 3 % of the cells of a shard are non-zero -- instead of reduce_scatter_i32 over the dense
   * [nranks][V][Ksm] buffer: what travels are (cell, count) pairs of the non-zero cells.  See ggs_set_count_exchange. */
  int (*all_to_all_v_i32)(void *ctx, const void *send, const int64_t *send_offsets, const int64_t *send_counts, void *recv,
                          const int64_t *recv_offsets, const int64_t *recv_counts, void *hip_stream);
} ggs_exchange_ops;
#define GGS_EXCHANGE_OPS_V3_SIZE ((int32_t)(sizeof(ggs_exchange_ops) - sizeof(void *)))
/* Caller-supplied transport (tests: gloo through host staging; a JVM with its own collectives). */
int ggs_attach_exchange(ggs_handle *h, int32_t rank, int32_t nranks, const ggs_exchange_ops *ops);
/* RCCL, one process per GPU: rank 0 calls ggs_rccl_unique_id and hands the 128 bytes to every rank (any channel);
 * every rank then calls ggs_attach_rccl, which is ncclCommInitRank on the handle's device (collective, blocking).
 * librccl is dlopen'ed on first use (librccl.so.1: the copy already in the process if there is one).
 * ONE RCCL per process: a host that later maps a SECOND copy of librccl (measured: PyTorch's wheel brings its own; loaded
 * after this library had dlopen'ed ROCm's, the process aborted at exit with "double free or corruption" in the two
 * copies' teardown) must load its copy first, so that this dlopen resolves to it -- ldagroupedgibbssampler_amd/_lib.py
 * imports torch before the first exchange for exactly that reason; a JVM host has only the one copy. */
#define GGS_RCCL_UNIQUE_ID_BYTES 128
int ggs_rccl_unique_id(void *out_id /* GGS_RCCL_UNIQUE_ID_BYTES */);
int ggs_attach_rccl(ggs_handle *h, int32_t rank, int32_t nranks, const void *unique_id);
/* The same with a communicator the caller created (ncclComm_t; not destroyed by ggs_destroy). */
int ggs_attach_rccl_comm(ggs_handle *h, int32_t rank, int32_t nranks, void *nccl_comm);
/* RCCL, ONE process driving n GPUs (the JVM of the reference is one process): creates n handles on device_ids[0..n)
 * from cfg (cfg->device_id ignored), joined by ncclCommInitAll.  The group entry points take the handles in rank
 * order and issue every phase for all devices from the calling thread, the collectives inside ncclGroupStart/End. */
int ggs_group_create(const ggs_config *cfg, int32_t n, const int32_t *device_ids, ggs_handle **out_handles /* n */);
void ggs_group_destroy(ggs_handle **handles, int32_t n);
int ggs_group_set_z(ggs_handle **handles, int32_t n, const int32_t *const *z /* n pointers, each shard's N */, int32_t redraw_phi);
int ggs_group_sweep(ggs_handle **handles, int32_t n, int32_t n_sweeps);
/* The same group entry points over a CALLER-SUPPLIED transport (a JVM with collectives of its own): handles 0..n-1, each
 * created by ggs_create and joined with ggs_attach_exchange(h_i, i, n, ops_i), are adopted as a one-process group.  The
 * library then issues every collective step for handle 0, 1, .. n-1 in turn before any handle goes on to the next step
 * -- the order ncclGroupStart/End gives the RCCL group -- so a transport that completes a collective only when all n
 * handles have called it is never kept waiting by the calling thread (tests/test_native_exchange_gpu.py drives two
 * handles from ONE thread this way). */
int ggs_group_adopt(ggs_handle **handles, int32_t n);
/* Corpus-wide counts onto every handle of the group.  The per-handle getters that need them (ggs_get_type_topic_counts,
 * ggs_get_topic_totals, ggs_check_invariants, the log likelihoods) would each start a collective of their own --
 * from one thread, for one device at a time, that cannot complete -- so a one-process driver calls this first; the
 * getters then find the counts in place.  (GGS_FLAG_PARANOID's per-sweep check is not run by ggs_group_sweep.) */
int ggs_group_gather_counts(ggs_handle **handles, int32_t n);
/* Timing aid, NOT a sampler: behaves as rank `rank` of `nranks` with the peers' contributions missing (the collectives
 * become local copies), so that one GPU can time the per-rank compute phases of an N-GPU split.  Counts and Phi are
 * then wrong by construction (ggs_check_invariants fails). */
int ggs_attach_null_exchange(ggs_handle *h, int32_t rank, int32_t nranks);
/* How the counts travel (typeTopicCounts of the reference; BASELINE config 5 names its rows sparse; the reference itself
 * tracks the touched cells per topic, UPLDA:1166-1176): mode 0 = by rule (sparse where the dense buffer is large and mostly
 * zero: V*K >= 2^26 cells and fewer tokens per rank than half of them -- both known alike on every rank, so all ranks
 * agree), 1 = always the dense reduce-scatter, 2 = always the (cell, count) pairs.  Every rank must make the same call
 * (before the first sweep).  Sparse needs all_to_all_v_i32 and a handle of its own process or thread (not the one-process
 * group entry points, whose collectives are collected step by step): otherwise the dense form runs.  Results are the
 * same integers either way. */
int ggs_set_count_exchange(ggs_handle *h, int32_t mode);
/* *sparse = 1 if the next count exchange of this handle ships (cell, count) pairs; *pairs_last (or NULL) = pairs this rank
 * sent in the last one, *cells (or NULL) = V * Ksm * nranks, the dense buffer's cells. */
int ggs_get_count_exchange(const ggs_handle *h, int32_t *sparse, int64_t *pairs_last, int64_t *cells);
/* rank, nranks and the rank's topic slice [k_begin, k_end) (0, 1, 0, K without an exchange) */
int ggs_get_exchange_info(const ggs_handle *h, int32_t *rank, int32_t *nranks, int32_t *k_begin, int32_t *k_end);
/* Who carries the collectives: *provider = 0 none, 1 RCCL, 2 the caller's callbacks, 3 the null timing aid; for RCCL
 * *comm_nranks / *comm_rank are read back from the communicator itself (ncclCommCount / ncclCommUserRank: what RCCL
 * saw, not what the caller passed to the attach call; -1 if the query fails), otherwise the attach call's values.
 * A benchmark line quotes these beside its number.  ABI version 4. */
int ggs_get_exchange_provider(const ggs_handle *h, int32_t *provider, int32_t *comm_nranks, int32_t *comm_rank);

/* ---- state copy-back (the Java getters) ------------------------------------
 * Wherever a getter or a diagnostic below names alpha, alphaSum, beta or betaSum it means the handle's CURRENT values
 * (ggs_get_hyperparameters): the configuration's until ggs_set_hyperparameters gives others. */
int ggs_get_z(ggs_handle *h, int32_t *z /*N*/);                         /* getZIndicators, MSLDA:464-477 */
int ggs_get_type_topic_counts(ggs_handle *h, int32_t *n_wk /*[V][K]*/); /* getTypeTopicMatrix, UPLDA:226-234 */
int ggs_get_topic_totals(ggs_handle *h, int32_t *n_k /*K*/);            /* getTopicTotals, MSLDA:976 */
int ggs_get_phi(ggs_handle *h, double *phi /*[K][V]*/);                 /* getPhi, UPLDA:1946-1948 */
int ggs_set_phi(ggs_handle *h, const double *phi /*[K][V]*/);           /* setPhi, UPLDA:1897-1926 */
int ggs_get_phi_mean(ggs_handle *h, double *phi_mean /*[K][V]*/, int32_t *n_sampled); /* getPhiMeans, UPLDA:1954-1966 */
int ggs_get_theta(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *theta /*[(end-begin)][K]*/); /* thetaMatrix, GGS:72, UPLDA:716-720 */
int ggs_get_doc_topic_counts(ggs_handle *h, int64_t doc_begin, int64_t doc_end, int32_t *n_dk); /* getDocumentTopicMatrix, MSLDA:536-547 */
int ggs_get_timings(ggs_handle *h, ggs_timings *out);                   /* zSamplingTimeCum / phiSamplingTimeCum, UPLDA:642-693 */

/* ---- hyperparameter optimisation (hyperparam_optim_interval, symmetric_alpha; UPLDA:647-649, 891-902) -------------------------
 * The step of MALLET's --optimize-interval: two histograms of the current state (from the device, a few KB of bins), the two
 * estimators of MALLET's Dirichlet (host, no GPU), and the setter that hands the learned values back to the handle.
 *
 * Rules of both histograms:
 *   bin range   n_bins must exceed every value that occurs: the caller passes longestDocLength + 1 and maxTypeCount + 1, as Java
 *               sizes its arrays.  If a value is >= n_bins the call returns GGS_ERR_BAD_ARG and writes NOTHING to its outputs (the
 *               device flags the value, it never indexes with it).
 *   Java ints   every bin is a Java int.  Bin 0 of the symmetric document histogram counts D * K pairs and can pass 2^31: it wraps
 *               modulo 2^32 as Java's would; neither estimator reads bin 0.  Every other bin is exact.
 *   schemes     both calls work under every scheme flag: they read only z, doc_ptr and the counts.
 *   empty documents count n_dk == 0 for every topic, and length 0.
 *
 * topicDocCounts of MSLDA:815-845 from the device-resident z of THIS handle's documents (a shard's own; the caller sums shards).
 * rows = symmetric ? 1 : K; hist is int32 [rows][n_bins]. hist[k][c] = documents with n_dk == c. symmetric: all topics into row 0.
 * doc_lengths (or NULL) is int32 [n_bins]: documents of that length (docLengthCounts, UPLDA:377-432); with it, a document of
 * n_bins tokens or more is out of range too.  More than ~9000 topics (four rows of K counts pass the LDS): GGS_ERR_UNSUPPORTED. */
int ggs_doc_topic_histogram(ggs_handle *h, int32_t symmetric, int64_t n_bins, int32_t *hist, int32_t *doc_lengths);
/* countHistogram of MSLDA:867-880 over the corpus-wide int32 [V][K] counts: hist[c] = cells with n_wk == c, int32 [n_bins].
 * With an exchange this is a COLLECTIVE call, as ggs_get_type_topic_counts is. The counts are gathered first and every rank returns
 * the corpus histogram. */
int ggs_type_topic_count_histogram(ggs_handle *h, int64_t n_bins, int32_t *hist);
/* alpha: K values, or NULL to keep the current ones. beta > 0. beta_sum: the Java field betaSum, or 0.0 for beta * V.
 * From the next z step on the handle is, bit for bit and in everything the getters return, a handle created with these values
 * and given this handle's exported state (z, Phi, iteration).  (After optimizeBeta the Java field betaSum is the learned value and
 * beta = betaSum / numTypes, MSLDA:897-901: not the bits of beta * V, hence the third argument.)
 * A non-finite or non-positive alpha_k or beta, or a negative or non-finite beta_sum, returns GGS_ERR_BAD_ARG and leaves the handle
 * untouched; a call between ggs_sweep_begin and ggs_sweep_end returns GGS_ERR_STATE.  With an exchange every rank makes the same
 * call with the same values; this is NOT checked.
 * One deviation, ours: the reference builds spalias's alias tables inside samplePhi with the old alpha and optimises afterwards, so
 * its next z step runs on alpha_old * phi tables.  Here the tables follow the setter -- one rule for every scheme. */
int ggs_set_hyperparameters(ggs_handle *h, const double *alpha, double beta, double beta_sum);
/* the current values: alpha (K values, or NULL), beta, betaSum (each or NULL) */
int ggs_get_hyperparameters(const ggs_handle *h, double *alpha /*K or NULL*/, double *beta, double *beta_sum);
/* MALLET 2.0.8's Dirichlet.learnSymmetricConcentration and Dirichlet.learnParameters, on the host (no GPU, like
 * ggs_java_lcg_next_ints).  The jar is not in the reference tree, so THIS TEXT is the specification (parity against a JVM is
 * unpinned).  All arithmetic is fp64, left to right, in exactly this order; log is the host libm's.
 *   digamma(z): if z < 1e-6 return -0.5772156649015328606065121 - 1/z.  psi = 0; while z < 9.5 { psi -= 1/z; z++ }; x = 1/z; y = x*x;
 *     psi += log(z) - .5*x - y*(1/12. - y*(1/120. - y*(1/252. - y*(1/240. - y*(1/132. - y*(691/32760. - y*(1/12.))))))).
 *   ggs_learn_symmetric_concentration: largest = the largest i with count_hist[i] > 0, or 0; nz = the ascending indices with
 *     obs_lengths > 0.  200 iterations, always: cp = current / num_dimensions; dg = 0, num = 0; for i = 1 .. largest:
 *     dg += 1.0 / (cp + i - 1), num += count_hist[i] * dg.  dg = 0, den = 0, prev = 0, cached = digamma(current); for each len in nz:
 *     if len - prev > 20: dg = digamma(current + len) - cached, else for i = prev .. len-1: dg += 1.0 / (current + i); then
 *     den += dg * obs_lengths[len], prev = len.  current = cp * num / den.  *out = current.
 *   ggs_learn_parameters: parametersSum = the k-order sum of params; nonZeroLimit[k] = the largest i with obs[k][i] > 0, or -1.
 *     Per iteration: denominator = 0, dg = 0; for i = 1 .. n_len-1: dg += 1 / (parametersSum + i - 1), denominator +=
 *     obs_lengths[i] * dg; denominator -= 1 / scale; parametersSum = 0; for each k: old = params[k], p = 0, dg = 0; for i = 1 ..
 *     nonZeroLimit[k]: dg += 1 / (old + i - 1), p += obs[k][i] * dg; params[k] = old * (p + shape) / denominator,
 *     parametersSum += params[k].  *sum_out = parametersSum.
 * A null pointer or a size < 1 returns GGS_ERR_BAD_ARG. */
int ggs_learn_symmetric_concentration(const int32_t *count_hist, int64_t n_hist, const int32_t *obs_lengths, int64_t n_len,
                                      int32_t num_dimensions, double current, double *out);
int ggs_learn_parameters(double *params /*K, in/out*/, int32_t K, const int32_t *obs /*[K][n_bins]*/, int64_t n_bins,
                         const int32_t *obs_lengths, int64_t n_len, double shape, double scale, int32_t iterations, double *sum_out);
int ggs_reset_timings(ggs_handle *h);
/* replaces: ensureConsistentTopicTypeCounts (UPLDA:299-338): counts >= 0, they sum to the
 * corpus size, column sums == tokensPerTopic.  (The reference's other paranoid assert, "all
 * deltas zero at postSample", ParanoidUncollapsedParallelLDA.java:42-55, has no device
 * counterpart: there is no delta matrix, the counts are rebuilt from z every sweep.) */
int ggs_check_invariants(ggs_handle *h);
/* Launch geometry of the z kernel the handle launches (ggs_get_z_form names it), for bench.py's roofline accounting.
 * lds_bytes_z: the dynamic LDS of that launch (score-register kernels: of the fused form with a full hot table; schemes
 * spalias and polyaurn_sparse: of the current corpus, since their lists are sized by the longest document).  num_chunks: the work items the
 * persistent grid strides -- chunks for scheme ggs; for the other schemes entries of the document order (wave per
 * document) or groups of 64 of them (lane per document); 0 before ggs_set_corpus. */
int ggs_get_launch_info(ggs_handle *h, int64_t *num_chunks, int32_t *lds_bytes_z, int32_t *docs_per_block_theta);
/* Words whose phiT rows the z kernels keep in LDS tables for the current corpus -- the hot-word table plus the warm
 * tiers' tables (0 for K > 192 and scheme pcgs): tokens of these, the most frequent words of the handle's corpus, read
 * no phiT row from memory -- bench.py's cold-row byte accounting. */
int ggs_get_num_hot_words(ggs_handle *h, int32_t *num_hot);
/* The warm tiers of the current corpus (z_warm_kernel: the words next in frequency after the hot table's, one LDS table
 * per tier, their chunks drawn from up to *docs_per_chunk documents): tiers kept, their words in all (part of what
 * ggs_get_num_hot_words reports).  All 0 where the score-register kernels do not run.  ABI version 5. */
int ggs_get_warm_tiers(ggs_handle *h, int32_t *tiers, int32_t *warm_words, int32_t *docs_per_chunk);
/* Launches of the z kernel per sweep for the current corpus: 1, or the number of document parts the streaming kernel's
 * step is cut into (K > 192; the next theta of a part is drawn beside the following parts) -- bench.py scales the
 * per-launch PMC counters of a profile by it. */
int ggs_get_z_parts(ggs_handle *h, int32_t *parts);
/* Which z kernel(s) the sweeps of the current corpus run, so that a benchmark line can NAME what it timed instead of
 * assuming it: *kernel = 0 whole-row tile kernel, 1 score-register kernels (K <= 160), 2 one-pass streaming kernel,
 * 3 its two-pass cross-check, 4 pcgs lane-per-document, 5 pcgs wave-per-document, 6 spalias wave-per-document,
 * 7 lightpclda wave-per-document, 8 polyaurn_sparse wave-per-document, 9 lightcollapsed wave-per-document,
 * 10 nzvsspalias wave-per-document, 11 adlda wave-per-document, 12 lightpcldaw2 wave-per-document; *form (kernel 1 only, else 0) =
 * 1 split (cold chunks and hot chunks as two kernels side by side), 2 fused (one kernel takes both in turn);
 * *calibrated = 1 once the first z step of the corpus has timed both forms and kept the faster (0 before that, and
 * when a form is forced or there is nothing to split).  ABI version 4. */
int ggs_get_z_form(ggs_handle *h, int32_t *kernel, int32_t *form, int32_t *calibrated);
/* The hot words of the current corpus as pair-chunks (z_pairs_kernel: each (document, hot word) pair scored once, its tokens
 * drawn from that): *enabled = 1 where the split form launches z_pairs_kernel in z_hot_kernel's place (0 with
 * GGS_DEBUG_HOT_PAIRS=0, in the fused form and where the score-register kernels do not run), and the pair-chunks, pairs and
 * hot tokens of the lists (0 where they are not built). */
int ggs_get_hot_pairs(ggs_handle *h, int32_t *enabled, int64_t *pair_chunks, int64_t *pairs, int64_t *tokens);
/* ---- primitives, exported so the parity tests can pin each layer ----------- */
int ggs_debug_philox(int32_t device_id, int64_t n, const uint32_t *ctr /*n*4*/, const uint32_t *key /*n*2*/, uint32_t *out /*n*4*/);
int ggs_debug_math(int32_t device_id, int32_t op /*0 log,1 pow,2 sqrt,3 div,4 exp,5 pow as the gamma draws call it,6 u53 of the words x,y*/, int64_t n, const double *x, const double *y, double *out);
int ggs_debug_draw(int32_t device_id, int32_t kind /*0 uniform,1 gaussian,2 gamma (general loops),3 gamma as the kernels draw it: first try then general,4 as 3 with first-try results negated*/, uint64_t seed, uint32_t iteration,
                   uint32_t purpose, uint64_t elem0, int64_t n, const double *shape, double *out, int32_t *status);
/* scheme=polyaurn's Poisson draw (PoissonFixedCoeffSampler.java:31-50, PolyaUrnDirichlet.java:102-107; GGS_FLAG_POLYAURN):
 * out[i] = X of element elem0 + i with count counts[i] >= 0, exactly as the Phi kernel draws it under (beta, threshold) --
 * threshold 0 means 100, 1..512 allowed.  ABI version 6. */
int ggs_debug_poisson(int32_t device_id, double beta, int32_t threshold, uint64_t seed, uint32_t iteration, uint32_t purpose, uint64_t elem0,
                      int64_t n, const int32_t *counts, int32_t *out);
/* scheme=spalias's alias tables (reGenerateAliasTable, util/OptimizedGentleAliasMethod.java; GGS_FLAG_SPALIAS), built by the
 * product kernel from phi [K][V] and alpha [K]: ps [V][K], a [V][K] and type_norm [V] = the k-order sum of phi[k][w] * alpha[k].
 * A draw x in [0, 1) from word w's table: ups = x * K, i = (int)ups, topic = (ups - i) > ps[w][i] ? a[w][i] : i.  K up to 4096. */
int ggs_debug_alias(int32_t device_id, int32_t V, int32_t K, const double *phi, const double *alpha, double *ps, int32_t *a, double *type_norm);
/* the tables of the handle's current Phi (GGS_FLAG_SPALIAS, GGS_FLAG_LIGHTPCLDA, GGS_FLAG_POLYAURN_SPARSE or GGS_FLAG_NZVSSPALIAS; GGS_ERR_STATE
 * otherwise or before the first Phi); any of the three outputs may be null.  GGS_FLAG_LIGHTCOLLAPSED and GGS_FLAG_LIGHTPCLDAW2: the tables of the handle's
 * current counts, which the next sweep builds at its head (after ggs_set_corpus, outside a split sweep): the call itself
 * rebuilds all V lists and tables from the corpus-wide counts, overwriting those the last z step used, and with an exchange
 * attached gathering the counts is a collective -- every rank makes the call, in the same order.  The first nw[w] entries of row w are
 * the word's table over its list (a draw x: ups = x * nw[w], i = (int)ups, topics[w][(ups - i) > ps[w][i] ? a[w][i] : i]), the
 * entries behind them read ps = 1.0, a = their index; type_norm[w] = typeMass, 0.0 for a word without tokens */
int ggs_get_alias_tables(ggs_handle *h, double *ps /*[V][K]*/, int32_t *a /*[V][K]*/, double *type_norm /*[V]*/);
/* scheme=spalias_priors (SpaliasUncollapsedParallelWithPriors, ParallelLDA.java:464-468; LDASamplerWithPriors): topic priors,
 * "anchor words".  No flag of its own and no new ABI version: a GGS_FLAG_SPALIAS handle on which ggs_set_topic_priors has been
 * called (any other handle: GGS_ERR_STATE).  Without the call a spalias handle plans, allocates and launches exactly what it did
 * before; everything the priors need is planned and allocated by the call.
 *   ggs_set_topic_priors  the n_zero cells (topic[i], word[i]) get prior 0.0, every other cell 1.0.  Duplicates are allowed,
 *       n_zero == 0 too ("a priors file that names nothing": the conditional draw below over an all-ones matrix, NOT bit-equal to
 *       plain spalias, as in the reference whenever a file is named).  Legal before or after ggs_set_corpus but only while the
 *       handle has no Phi (before ggs_init_phi, ggs_set_z with redraw, ggs_set_phi: afterwards GGS_ERR_STATE); a later call
 *       replaces an earlier one.  GGS_ERR_BAD_ARG, the handle left as it was: a topic or word out of range, a topic with all V
 *       words zero, a word with all K topics zero (ensureConsistentPriors).  With an exchange attached every rank makes the
 *       same call; it is not a collective.  On the device the priors are one bit per (word, topic).
 *   ggs_get_topic_priors  getTopicPriors: priors[k][v] = 1.0 or 0.0; all 1.0 when none were set.
 * With priors set:
 *   the initial Phi (ggs_init_phi, ggs_set_z with redraw) is the usual draw, run to its end, then phi[k][v] *= prior[k][v]; rows
 *       are not renormalised;
 *   the Phi of a sweep is the conditional draw over each topic's allowed words (ConditionalDirichlet.nextConditionalDistribution):
 *       g = Gamma(shape) on the Philox stream of element k*V + v as ever (a zeroed cell's stream is not used), g <= 0 -> 0.0001,
 *       sum_gamma and sum_phi (of the OLD row) in index order, phi[k][v] = (g / sum_gamma) * sum_phi; zeroed cells stay +0.0.  Rows
 *       therefore keep the mass their allowed words had in the initial draw;
 *   the z step is spalias's, unchanged: the reference's factor prior[k][w] on the list scores has the bits of the product without
 *       it as long as Phi is exactly 0 wherever the prior is.  So that nothing can break that, ggs_set_phi returns
 *       GGS_ERR_BAD_ARG for a Phi with a non-zero value in a zeroed cell (our decision: the reference copies the matrix). */
int ggs_set_topic_priors(ggs_handle *h, int64_t n_zero, const int32_t *topic, const int32_t *word);
int ggs_get_topic_priors(ggs_handle *h, double *priors /*[K][V]*/);
/* scheme=lightpclda's Metropolis-Hastings counters, cumulative since ggs_set_corpus (the three the reference keeps
 * commented out, LightPCLDA.java:28-44), every token in exactly one: out[0] tokens whose word proposal was accepted and
 * kept, out[1] tokens whose document proposal was accepted, out[2] tokens left on their old topic.  The same three classes
 * under GGS_FLAG_LIGHTCOLLAPSED and GGS_FLAG_LIGHTPCLDAW2.  GGS_ERR_STATE without one of these flags. */
int ggs_get_mh_stats(ggs_handle *h, int64_t out[3]);
/* scheme=polyaurn_sparse's word lists of the handle's current Phi: nw[w] = the number of topics with phi[k][w] != 0.0,
 * topics[w][0 .. nw[w]) those topics in ascending order, -1 behind them.  Either output may be null.  GGS_ERR_STATE without
 * GGS_FLAG_POLYAURN_SPARSE or before the first Phi.  GGS_FLAG_LIGHTCOLLAPSED and GGS_FLAG_LIGHTPCLDAW2: the lists of the handle's current counts, nw[w] = the
 * number of topics with n_wk > 0 (0 for a word without tokens); the same rebuild and, with an exchange, the same collective as
 * ggs_get_alias_tables under that flag.  GGS_FLAG_ADLDA: the same lists of the current counts.  GGS_FLAG_NZVSSPALIAS: the lists
 * as that flag defines them (the drawn cells). */
int ggs_get_word_topic_lists(ggs_handle *h, int32_t *nw /*V*/, int32_t *topics /*[V][K]*/);
/* scheme=polyaurn_sparse's counters, cumulative since ggs_set_corpus, every token in exactly one of the first three:
 * out[0] tokens that walked the word's list, out[1] tokens that walked the document's list, out[2] tokens drawn uniformly
 * (no candidate), out[3] the sum of n, the number of candidates, over all tokens.  GGS_ERR_STATE without
 * GGS_FLAG_POLYAURN_SPARSE or GGS_FLAG_NZVSSPALIAS (there out[2] counts the tokens drawn from the alias table for want of a
 * candidate).  GGS_FLAG_ADLDA: out[0] tokens drawn from the word bucket Q, out[1] from the document bucket R, out[2] from the
 * smoothing bucket S, out[3] the sum of nnz_w + nnz_d (the document's list after the token's removal) over all tokens. */
int ggs_get_sparse_stats(ggs_handle *h, int64_t out[4]);
/* scheme=nzvsspalias: pi, the prior probability that a cell without tokens keeps its place in the topic (vsPrior of
 * VSDirichlet; 0.5 until set).  Callable until the handle has a Phi (afterwards GGS_ERR_STATE); pi outside (0, 1):
 * GGS_ERR_BAD_ARG; without GGS_FLAG_NZVSSPALIAS: GGS_ERR_STATE. */
int ggs_set_variable_selection_prior(ggs_handle *h, double pi);
/* out[0] the cells the last variable-selection draw left undrawn (0 before the first sweep), out[1] the cells of the
 * current Phi that are 0.0, out[2] the largest number of rounds a topic's indicator chain took in that draw (with an exchange:
 * of the rank's own topics; out[0] and out[1] cover all topics on every rank).  out[0] and out[2] are 0 again after
 * ggs_init_phi, the redraw of ggs_set_z and ggs_set_phi.  GGS_ERR_STATE without GGS_FLAG_NZVSSPALIAS or before the first Phi. */
int ggs_get_vs_stats(ggs_handle *h, int64_t out[3]);
/* The indicator chain on its own (csrc/ggs_phi_vs.hpp): counts [K][V] >= 0 and prev_phi [K][V] as the Java arrays,
 * drawn_out [K][V] = 1 where the cell is drawn (every cell with a count is), s_end [K] = the chain's s behind the last
 * cell, rounds [K] = the rounds each topic took.  u [K][V], if given, replaces the Philox uniforms (tests put U on
 * p(s) and one ulp above it).  GGS_ERR_INVARIANT where the reference's range check would throw. */
int ggs_debug_vs_indicators(int32_t device_id, int32_t V, int32_t K, const int32_t *counts, const double *prev_phi, double beta, double pi, uint64_t seed,
                            uint32_t iteration, const double *u /*or NULL*/, uint8_t *drawn_out, int32_t *s_end, int32_t *rounds);
/* replaces: modelLogLikelihood (UPLDA:1644-1758), the Dirichlet-multinomial log likelihood of the current topic
 * assignments, split where a doc-sharded run splits it: doc_side covers THIS handle's documents (sum_d [...] +
 * D*lgS(alphaSum), UPLDA:1674-1694) and topic_side the (replicated) type-topic counts (UPLDA:1701-1747); the model's
 * value is the sum of every shard's doc_side plus one topic_side.  lgS = MALLET Dirichlet.logGammaStirling.  A
 * diagnostic: partial sums are reduced in a fixed tree, so the value is run-to-run identical and not bit-equal to the Java
 * loop's running sum: each side lies within (c + 2) * 2^-53 * sum|term| of the exact sum of the Java loop's terms, c the
 * longest chain of additions in the tree (a few dozen; csrc/ggs_loglik.hpp), where the running sum itself is only within
 * (terms - 1) * 2^-53 * sum|term| of it.  Needs tokensPerTopic up to date (any completed sweep, ggs_init_phi or ggs_set_z
 * with redraw).  GGS_ERR_UNSUPPORTED beyond 10238 topics (four documents' topic counts are kept in LDS); so for
 * ggs_log_posterior. */
int ggs_model_log_likelihood(ggs_handle *h, double *doc_side, double *topic_side);
/* replaces: computeLogPosterior (UPLDA:1573-1634, the LDA log posterior of Doss and George 2025, logged every
 * diagnostic iteration, UPLDA:820-821) for scheme ggs: doc_side = sum over THIS handle's tokens of
 * log(phi[z][w] + 1e-12) + sum_d sum_k (n_dk + alpha_k - 1) log(theta[d][k] + 1e-12) with theta = the rows the last z
 * step used (thetaMatrix); topic_side = (beta - 1) sum_{k,v} log(phi[k][v] + 1e-12); the value is the sum over the
 * shards' doc_side plus one topic_side.  (The Java loop fills a dense K x V matrix per document -- D*K*V operations
 * -- to compute what is a sum over tokens.)  Same accuracy contract as ggs_model_log_likelihood.
 * Scheme pcgs keeps no thetaMatrix: the reference draws theta_d ~ Dirichlet(n_d. + alpha) afresh for this diagnostic
 * (UPLDA:710-714, LDAUtils.drawDirichlets) from a clock-seeded MALLET generator; here that draw is the one of GGS:57-72
 * under the Philox stream GGS_PURPOSE_THETA at the current iteration (reproducible; ggs_get_theta returns it afterwards).
 * GGS_ERR_UNSUPPORTED for scheme collapsed (no Phi). */
int ggs_log_posterior(ggs_handle *h, double *doc_side, double *topic_side);
/* replaces: the two distance loops of the diagnostics (compute_doc_topic_distances; UPLDA:723-753 "Quantity A" and :778-806
 * "Quantity B"; the same code in SerialCollapsedLDA.java:221-305 and ADLDA.java:414 ff.), on the device-resident state.
 * Per pair: s = 0.0; for k in index order t = a[k] - b[k], s = s + t * t (product and sum rounded separately, never fused:
 * Math.pow(t, 2.0) is t * t on HotSpot from JDK 9 on -- an assumption for older JVMs and StrictMath); dist = sqrt(s); the minimum
 * starts at 1e+20 and is replaced only when dist < min, so a NaN distance never enters and a row without a partner reports 1e+20.
 * sqrt is correctly rounded, hence monotone: the kernels minimise the sums and take one square root per output
 * (csrc/ggs_distances.hpp).  Bit-identical to that loop.
 * ggs_min_doc_distances: min_dist[d], d in [0, D): the smallest distance of this handle's theta row d to
 *   other == NULL (n_other must be 0): every OTHER row of this handle's theta -- the reference's loop (min_doc_distances.csv);
 *   other given: the n_other rows of the foreign block other [n_other][K] (host memory; nothing is skipped).  A doc-sharded run
 *   calls once with NULL and once per foreign shard's theta block and takes the element-wise minimum: bit-identical to one handle.
 *   The block travels to the device in pieces of at most 64 MiB.
 * theta: scheme ggs -- the thetaMatrix of the last z step (UPLDA:716-720); the pcgs family -- the diagnostic draw of
 * ggs_log_posterior (UPLDA:710-714: the stream GGS_PURPOSE_THETA at the current iteration; both calls redraw the same bits, and
 * ggs_get_theta returns them afterwards).  D == 0 writes nothing.
 * ggs_min_topic_distance: *min_dist = the smallest distance between two rows of the current Phi (min_topic_distances.csv), 1e+20
 * for K == 1.  Phi is replicated on every rank of an exchange: any rank's value is the model's.
 * Both: GGS_ERR_UNSUPPORTED for schemes collapsed, lightcollapsed and adlda (their augmented theta and Phi draws,
 * LDAUtils.drawDirichlets, are not part of this library); GGS_ERR_STATE before a corpus and a Phi exist; GGS_ERR_BAD_ARG for a
 * null output or a negative size. */
int ggs_min_doc_distances(ggs_handle *h, const double *other /*[n_other][K] host, or NULL*/, int64_t n_other, double *min_dist /*[D]*/);
int ggs_min_topic_distance(ggs_handle *h, double *min_dist);
/* replaces: the loops of similarity/LDADistancer.distance (LDADistancer.java:79-99), tui/LDASimilarity.java:175-183 and
 * classify/KLDivergenceClassifier.classify (:71-78): the distance classes of cc/mallet/similarity between training documents and
 * unseen ones, and the n nearest training documents (csrc/ggs_similarity.hpp).  New symbols, not a new ABI version.
 * Distance.calculate(v1, v2) is always called with v1 = the training row (or class centroid) and v2 = the query row.  Each class is
 * restated in Java operation order: sums from 0.0 in index order, every product, quotient and sum rounded on its own,
 * Math.pow(x, 2) = x * x, Math.log = StrictMath.log, sqrt and / correctly rounded.  Bit-identical to those loops restated
 * (tests/similarity_restatement.py).  cc.mallet.util.Maths.klDivergence is MALLET's and not in the reference tree; it is taken as
 *   klDiv = 0; for i: if p1[i] == 0 continue; if p2[i] == 0 return +Infinity; klDiv += p1[i] * Math.log(p1[i] / p2[i]);
 *   return klDiv / Math.log(2)
 * (DESIGN.md 2), which is as far as metrics 7, 8 and 9 are pinned against a JVM. */
#define GGS_DISTANCE_MANHATTAN 0      /* ManhattanDistance */
#define GGS_DISTANCE_EUCLIDIAN 1      /* EuclidianDistance */
#define GGS_DISTANCE_HELLINGER 2      /* HellingerDistance: the sum of (sqrt(a) - sqrt(b))^2 itself, no root, no 1/2, as written */
#define GGS_DISTANCE_COSINE 3         /* CosineDistance: 1 + (-(dot / (sqrt(normA) * sqrt(normB)))) */
#define GGS_DISTANCE_CANBERRA 4       /* CanberraDistance: a term with denom == 0.0 is 0.0 */
#define GGS_DISTANCE_CHEBYCHEV 5      /* ChebychevDistance: Math.max, a NaN element gives NaN */
#define GGS_DISTANCE_JACCARD 6        /* JaccardDistance: intersection > 0.0 ? 1 - (i / u) : 0.0, a NaN intersection gives 0.0 */
#define GGS_DISTANCE_KL 7             /* KLDistance: (kl(v1, v2) + kl(v2, v1)) / 2 */
#define GGS_DISTANCE_JENSEN_SHANNON 8 /* JensenShannonDistance: (KLDistance(v1, avg) + KLDistance(v2, avg)) / 2 */
#define GGS_DISTANCE_UBER 9           /* UberDistance: Canberra, Chebychev, Cosine, Euclidian, Jaccard, KL, Manhattan summed, / 7 */
#define GGS_DISTANCE_STATISTICAL 10   /* StatisticalDistance: -(correlation - 1), the covariance a running mean */
#define GGS_DISTANCE_BHATTACHARYYA 11 /* BhattacharyyaDistance, as written (var2 / var2) */
#define GGS_DISTANCE_COUNT 12
#define GGS_NEAREST_MAX 16
/* The training side of the two calls below: per document of the handle, from its device-resident z.
 * ggs_get_theta_estimate: ModifiedSimpleLDA.getThetaEstimate (MSLDA:709-753): (n_dk + alpha_k) / sum_k (n_dk + alpha_k), the
 *   normaliser summed in k order, with the handle's CURRENT alpha (after ggs_set_hyperparameters: the new one).
 * ggs_get_zbar: getZbar (MSLDA:647-668): n_dk / N_d, zeros for an empty document.
 * out is [doc_end - doc_begin][K]; the rows are made on the device in pieces whose work space does not grow with D.  Every scheme.
 * GGS_ERR_STATE before a corpus, and with a corpus that has tokens before ggs_init_z_java_lcg or ggs_set_z gave it a z (so
 * that the all-zero z ggs_set_corpus leaves is never taken for a state); the same for the two calls below.  GGS_ERR_BAD_ARG for
 * a bad range or a null output. */
int ggs_get_theta_estimate(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *out);
int ggs_get_zbar(ggs_handle *h, int64_t doc_begin, int64_t doc_end, double *out);
/* The distances of the handle's documents (their theta estimate rows: v1) to Q query rows (v2).  The rule of LDADistancer.java:84-87
 * is part of the distance: both documents empty 0.0, exactly one empty +Infinity; the training lengths are the handle's, query_len
 * [Q] the queries' (NULL: none is empty).
 * ggs_nearest_documents: idx / dist [Q][n_nearest], ordered by (distance rising, document index rising).  Distances compare by
 *   value (-0.0 and 0.0 tie, the index decides); only a distance < +Infinity is a candidate (NaN and +Infinity never enter); unfilled
 *   places hold index -1 and distance +Infinity.  n_nearest = 1 is the loop of LDASimilarity.java:175-183 (strict minDist > d: the
 *   first minimum).  The indices are global: the handle's doc_base + the local document, so the lists of the shards of a corpus merge
 *   by the same order into the list of the whole.  1 <= n_nearest <= GGS_NEAREST_MAX.
 * ggs_document_distances: dist [Q][D], every value as calculate() returns it (NaN included).
 * Every scheme.  Training rows, queries and the [Q][D] output travel in pieces of at most 64 MiB.  Nothing a sweep reads is written.
 * GGS_ERR_STATE before a corpus and a z exist; GGS_ERR_BAD_ARG: an unknown metric, n_nearest outside its range, a negative size or length, a null
 * output or query.  Q == 0 writes nothing; D == 0 writes the "nothing found" values. */
int ggs_nearest_documents(ggs_handle *h, int32_t metric, const double *query /*[Q][K] host*/, const int64_t *query_len /*[Q], or NULL*/, int64_t Q,
                          int32_t n_nearest, int64_t *idx /*[Q][n_nearest]*/, double *dist /*[Q][n_nearest]*/);
int ggs_document_distances(ggs_handle *h, int32_t metric, const double *query, const int64_t *query_len, int64_t Q, double *dist /*[Q][D]*/);
/* The handle-free primitive over the same kernels: out[j][i] = calculate(a[i], b[j]) for the rows of a [n][len] (v1) and b [m][len]
 * (v2), no length rule.  KLDivergenceClassifier's Q x C step.  GGS_ERR_BAD_ARG: an unknown metric, a negative n or m, len < 1, a null
 * pointer with work to do. */
int ggs_row_distances(int32_t device_id, int32_t metric, const double *a /*[n][len]: v1*/, const double *b /*[m][len]: v2*/, int64_t n, int64_t m, int64_t len,
                      double *out /*[m][n]*/);
/* replaces: LDAUtils.getTopWords / getTopWordIndices (LDAUtils.java:874-911; TopWords.txt, tui/ParallelLDA.java:272-283),
 * getTopRelevanceWords (:566-590; RelevanceWords.txt, ParallelLDA.java:285-296), getTopDistinctiveWords (:592-617),
 * getTopSalientWords (:619-644) and getK1ReWeightedWords (:752-801) on the handle's CURRENT corpus-wide type-topic counts (with
 * an exchange: gathered as ggs_get_type_topic_counts gathers them -- a collective call; every rank returns the model's answer).
 * Works under every scheme.  idx[k][r], r in [0, n_words): the word ids of topic k in IDSorter's order -- falling score, equal
 * scores (-0.0 == +0.0) by FALLING id; score (or NULL): their scores.  The score of (word w, topic k) by kind:
 *   GGS_TOP_WORDS        (double) n_wk
 *   GGS_TOP_RELEVANCE    lambda * L + (1 - lambda) * (L - log(p_w[w])), L = log(p_wk)            (Sievert & Shirley)
 *   GGS_TOP_DISTINCTIVE  0.0 + P * log(P / p_w[w]), P = p_wk * (mass_k / total) / p_w[w] left to right
 *   GGS_TOP_SALIENT      p_w[w] * distinctive
 *   GGS_TOP_K1           p_wk / (sum over k in index order, from 0.0, of p_wk)
 * with p_wk = (n_wk + beta) / mass_k, p_w[w] = rowsum_w / total and the three Java running sums, each from 0.0 over
 * (double) n_wk + beta in index order: mass_k over w, rowsum_w over k, total over all V * K cells (w outer, k inner).  Every
 * operation is rounded on its own in the Java order; log is the library's fdlibm log (StrictMath.log; Math.log on a JVM is
 * parity-unpinned, as everywhere here).  Bit-identical to those loops restated (tests/topic_summaries_restatement.py).
 * lambda is read by GGS_TOP_RELEVANCE only.  Nothing the sweep reads is written: a call between sweeps leaves the chain's bits.
 * GGS_ERR_BAD_ARG: null idx, n_words < 1 or > V (the Java IllegalArgumentException), an unknown kind, a lambda that is not
 * finite, beta == 0 with a kind other than GGS_TOP_WORDS (NaN scores, which IDSorter cannot order);
 * GGS_ERR_UNSUPPORTED: n_words > GGS_TOP_WORDS_MAX, or V * K >= 2^31 - 256; GGS_ERR_STATE before a corpus. */
#define GGS_TOP_WORDS 0
#define GGS_TOP_RELEVANCE 1
#define GGS_TOP_DISTINCTIVE 2
#define GGS_TOP_SALIENT 3
#define GGS_TOP_K1 4
#define GGS_TOP_WORDS_MAX 128
int ggs_top_words(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t *idx /*[K][n_words]*/, double *score /*[K][n_words] or NULL*/);
/* replaces: new TopicModelDiagnosticsPlain(model, numTopWords).topicsToCsv() (topics/TopicModelDiagnosticsPlain.java; the file
 * save_doc_topic_diagnostics makes tui/ParallelLDA.java:218-225 write), in two calls: the statistics over the documents (z), then
 * the scores from the corpus-wide counts and those statistics.  Notation: n = n_words; T_k[r], r < n: the top words of topic k,
 * exactly ggs_top_words(GGS_TOP_WORDS); c_dk: tokens of document d with z = k; n_wk, n_k: the corpus-wide counts;
 * wtc[w] = sum_k n_wk and numTokens = sum_k n_k (integers); P = {0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5}.  Every product, quotient
 * and sum is rounded on its own in the Java order; log is the library's fdlibm log (Math.log on a JVM is parity-unpinned).
 *
 * ggs_topic_doc_statistics (collectDocumentStatistics :108-220) covers THIS handle's documents; integers add across shards:
 *   doc_stats[k][0] nonzero   documents with c_dk > 0
 *   doc_stats[k][1] rank1     documents whose largest c_dk is at k (strict > walking k upwards: the lowest k among equal maxima)
 *   doc_stats[k][2 + i] at_prop[k][i]: for each document with c_dk > 0, prop = (alpha_k + c_dk) / (alphaSum + len_d), alphaSum the
 *                   running sum of alpha_k from 0.0 in index order; counters i = 0, 1, ... incremented until the first prop < P[i]
 *   codoc[k][i][j]  S_dk = { i : some token of d has type T_k[i] and z = k }; for each d with c_dk > 0 and each i in S_dk
 *                   codoc[k][i][i]++, for i < j both in S_dk [i][j]++ and [j][i]++ (a word under another topic does not count,
 *                   a word twice in a document counts once)
 *   clogc_out[k]    from 0.0 (or clogc_in[k], what the shards before this one left), over the documents in index order:
 *                   s = s + (double) c_dk * log((double) c_dk) for every d with c_dk > 0 -- one rounding chain per topic
 * idx [K][n_words] (host): the corpus-wide top words, or NULL for the handle's own ggs_top_words (then a collective call with an
 * exchange).  A doc-sharded run calls it rank after rank in document order with the same idx, clogc_out of one rank being the
 * next rank's clogc_in, and adds the integers: bit-identical to one handle over the whole corpus.
 *
 * ggs_topic_scores: topic_scores[row][k], the CSV's columns without word-length (host: it needs the alphabet), from the handle's
 * CURRENT corpus-wide counts (gathered as ggs_top_words gathers them: a collective call with an exchange) and the (summed)
 * statistics passed in.  Every division is in doubles, ints cast first.
 *   0 tokens            (double) n_k
 *   1 document_entropy  -clogc[k] / n_k + log(n_k)
 *   2 coherence         for row = 0..n-1, col < row: score = log((codoc[row][col] + beta) / (codoc[col][col] + beta)),
 *                       rowScore += score, min = score if score < min (from 0.0); topic += rowScore; word score of row = min
 *   3 uniform_dist      the words of k in IDSorter order (all V, falling count, ties by falling id):
 *                       score = (c / n_k) * log((c * V) / n_k), running sum from 0.0; word scores: the first n addends
 *   4 corpus_dist       same order: coef = (double) numTokens / n_k; score = (c / n_k) * log(coef * c / wtc[w]); running sum
 *   5 eff_num_words     same order: p = c / n_k; s += p * p; 1.0 / s
 *   6 token-doc-diff    over r < n: w_r = (double) n_{T_k[r],k}, d_r = codoc[r][r], running sums wordSum, docSum; per r:
 *                       p = w_r / wordSum, q = d_r / docSum, m = 0.5 * (p + q), score = 0.0, += 0.5 * p * log(p / m) if p > 0,
 *                       += 0.5 * q * log(q / m) if q > 0; word score; topic = running sum
 *   7 rank_1_docs       (double) rank1 / nonzero
 *   8 allocation_ratio  (double) at_prop[k][6] / at_prop[k][1]
 *   9 allocation_count  (double) at_prop[k][5] / nonzero
 * word_scores[4][K][n_words] (or NULL): coherence, uniform_dist, corpus_dist, token-doc-diff.  As in the Java, a zero cell's addend
 * of uniform_dist / corpus_dist is 0.0 * log(0.0) = NaN: those two topic scores are NaN unless the topic's column has no zero
 * cell, and a top word with count 0 has word score NaN; eff_num_words is unaffected (+ 0.0); n_k == 0 gives IEEE's NaNs and
 * infinities.  NaNs are NaN whatever their bits; everything else equals the Java loops restated
 * (tests/topic_diagnostics_restatement.py) bit for bit.  One deviation: the Java driver builds the diagnostics before it clamps
 * nr_top_words to V and then reads word id 0 for the missing positions; here n_words must be in [1, min(V, GGS_TOP_WORDS_MAX)].
 * Works under every scheme; nothing a sweep reads is written: a call between sweeps leaves the chain's bits.
 * GGS_ERR_STATE before a corpus; GGS_ERR_BAD_ARG: a null argument, n_words < 1 or > V, an idx entry outside [0, V);
 * GGS_ERR_UNSUPPORTED: n_words > GGS_TOP_WORDS_MAX, or (document statistics) K > GGS_TOPIC_DIAGNOSTICS_MAX_TOPICS: a document's
 * K-long histogram and masks no longer fit 60 KiB of LDS. */
#define GGS_TOPIC_DIAGNOSTICS_MAX_TOPICS 3072
#define GGS_TOPIC_SCORE_ROWS 10
#define GGS_TOPIC_WORD_SCORE_ROWS 4
int ggs_topic_doc_statistics(ggs_handle *h, int32_t n_words, const int32_t *idx /*[K][n_words] host, or NULL*/, const double *clogc_in /*[K] or NULL*/,
                             int32_t *codoc /*[K][n_words][n_words]*/, int32_t *doc_stats /*[K][9]*/, double *clogc_out /*[K]*/);
int ggs_topic_scores(ggs_handle *h, int32_t n_words, const int32_t *idx /*[K][n_words] host, or NULL*/, const int32_t *codoc, const int32_t *doc_stats,
                     const double *clogc, double *topic_scores /*[10][K]*/, double *word_scores /*[4][K][n_words] or NULL*/);
/* replaces: addTestInstances (UPLDA:340-343; the test set of the held-out estimator).  CSR like ggs_set_corpus; token
 * ids are indices of the TRAINING alphabet, ids >= num_types are out of vocabulary and skipped as at MPE:341-345.
 * doc_base = global index of the first test document (RNG element ids only; for a sharded test set).  Documents longer
 * than 2^25 tokens (the 24-bit block field of a particle's Philox stream, two uniforms per block): GGS_ERR_UNSUPPORTED. */
int ggs_set_test_corpus(ggs_handle *h, int64_t D, const int64_t *doc_ptr /*D+1*/, const int32_t *tokens, int64_t doc_base);
/* replaces: new MarginalProbEstimatorPlain(numTopics, alpha, alphaSum, beta, typeTopicCounts, tokensPerTopic)
 * .evaluateLeftToRight(testSet, numParticles, null) (MPE:51-121,123-519; call sites UPLDA:604-622,677-682,840-844 with
 * numParticles = 100, UPLDA:615) on the handle's CURRENT counts (corpus-wide after the sweep's exchange): the
 * left-to-right estimate of the test set's log likelihood, without the resampling pass (MPE:125).  doc_ll (D or NULL)
 * = the per-document values (what Java prints to docProbabilityStream); *total = their sum in document order.
 * Bit-identical to the oracle's restatement under the Philox stream GGS_PURPOSE_HELDOUT (the reference's Randoms is
 * clock-seeded).  The estimator's IllegalStateException ("Sampled invalid topic") -> GGS_ERR_INVALID_TOPIC.
 * The per-particle topic counts (1, 2 or 4 bytes each by the length of the test document) live in LDS where K * 64 of
 * them fit beside the tables -- up to 1704 topics with test documents of at most 255 tokens, 1024 with longer ones --
 * and in global memory otherwise (same arithmetic, slower).  GGS_ERR_UNSUPPORTED only when the estimator's tables
 * themselves do not fit LDS (about 6000 topics). */
int ggs_heldout_log_likelihood(ggs_handle *h, int32_t num_particles, double *doc_ll, double *total);
/* out[k] = x[0][k] + x[1][k] + ... in index order (exactly one of x / counts given; with counts the addends are
 * beta + counts[v][k]): the Phi normalisers' exact parallel column sum on its own, for adversarial inputs */
int ggs_debug_column_sum(int32_t device_id, int32_t V, int32_t K, const double *x /*V*K or NULL*/, const int32_t *counts /*V*K or NULL*/,
                         double beta, double *out /*K*/);
/* The same with the caller's GUESS of the running sums at every 64-row segment start (guess [V/64 rounded up + 1][K],
 * or NULL: the kernels make their own) -- what a sweep feeds from the previous sweep's exact values.  The guess must
 * never decide a result: the tests pass wrong, zero, NaN and exact ones.  pref_out (same shape, or NULL) = the exact
 * running sums the walk leaves behind; n_k_out (K, or NULL; counts only) = the integer column sums (tokensPerTopic). */
int ggs_debug_column_sum_guided(int32_t device_id, int32_t V, int32_t K, const double *x, const int32_t *counts, double beta,
                                const double *guess, double *out, double *pref_out, int32_t *n_k_out);
/* The distance kernels on their own, for arbitrary inputs: min_dist[i], i in [0, n) = min(1e+20, sqrt(min_sq[i])), min_sq[i]
 * (or NULL) = the smallest in-order sum of squared differences of row i of a over its partners, NaN sums ignored, +inf where
 * there is none.  element_major == 0: a is [n][len]; the partners are the m rows of b [m][len], or with b == NULL the other rows
 * of a (the diagonal skipped; m is not read) -- the document kernel.  element_major == 1: a is [len][n], b must be NULL -- the
 * topic kernel, which ggs_min_topic_distance follows with the minimum over i.  n, len (and m with b) must be positive. */
int ggs_debug_min_distances(int32_t device_id, const double *a, int64_t n, const double *b /*or NULL*/, int64_t m, int64_t len, int32_t element_major,
                            double *min_dist /*[n]*/, double *min_sq /*[n] or NULL*/);
/* The topic-summary kernels on their own, for an arbitrary count matrix [V][K] (host): idx / score as ggs_top_words, and (each
 * or NULL) the normalisers mass_k [K], rowsum_w [V], *total and every score all_scores [V][K].  Same error codes. */
int ggs_debug_topic_summaries(int32_t device_id, int32_t V, int32_t K, const int32_t *counts /*[V][K]*/, double beta, double lambda, int32_t kind,
                              int32_t n_words, int32_t *idx /*[K][n_words]*/, double *score /*[K][n_words] or NULL*/, double *mass_k /*[K] or NULL*/,
                              double *rowsum_w /*[V] or NULL*/, double *total /*or NULL*/, double *all_scores /*[V][K] or NULL*/);
/* Where a ggs_top_words call spends its device time (scripts/time_topic_summaries.py): the same launches on the handle's counts
 * with events between them; ms[4] = mass_k, total, the words' statistics (rowsum_w, p_w, log p_w), selection and merge.  The
 * first three are 0 for GGS_TOP_WORDS.  element_chain != 0: both column sums by the element-by-element chain kernel (one
 * lane per sum: what the total chain costs without ggs_exact_sum.hpp).  Nothing is copied back. */
int ggs_debug_top_words_phases(ggs_handle *h, int32_t kind, int32_t n_words, double lambda, int32_t element_chain, double *ms /*[4]*/);

/* The topic-diagnostics kernels on their own, for an arbitrary corpus with its z (doc_ptr [D + 1] from 0, tokens < V, z < K; host)
 * and an arbitrary count matrix [V][K] (host): outputs as ggs_topic_doc_statistics / ggs_topic_scores; sorted_ids [K][n_words] (or
 * NULL): the first n_words cells of every topic's sorted non-zero cells, -1 beyond them.  Same error codes. */
int ggs_debug_topic_doc_statistics(int32_t device_id, int64_t D, const int64_t *doc_ptr, const int32_t *tokens, const int32_t *z, int32_t V, int32_t K,
                                   const double *alpha /*[K]*/, int32_t n_words, const int32_t *idx, const double *clogc_in /*[K] or NULL*/, int32_t *codoc,
                                   int32_t *doc_stats, double *clogc_out);
int ggs_debug_topic_scores(int32_t device_id, int32_t V, int32_t K, const int32_t *counts /*[V][K]*/, double beta, int32_t n_words, const int32_t *idx,
                           const int32_t *codoc, const int32_t *doc_stats, const double *clogc, double *topic_scores, double *word_scores /*or NULL*/,
                           int32_t *sorted_ids /*or NULL*/);
/* Where ggs_topic_doc_statistics + ggs_topic_scores spend their device time (scripts/time_topic_diagnostics.py): both calls on the
 * handle's own top words with events between the launches; ms[7] = membership (host CSR and its upload), document pass (with the
 * mirror), column statistics and c log c addends, the clogc chain, n_k and wtc, compaction + sort + sorted chains, small scores. */
int ggs_debug_topic_diagnostics_phases(ggs_handle *h, int32_t n_words, double *ms /*[7]*/);
#ifdef __cplusplus
}
#endif
#endif /* GGS_HIP_H */
