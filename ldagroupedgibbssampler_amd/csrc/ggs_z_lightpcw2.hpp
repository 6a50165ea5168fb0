// ggs_z_lightpcw2.hpp -- the z loop of scheme=lightpcldaw2 (LightPCLDAtypeTopicProposal.java:101-274; ParallelLDA.createModel's
// "lightpcldaw2"): the LightLDA sampler of Yuan et al. over the partially collapsed model -- Phi is drawn, as under pcgs -- with
// scheme=lightcollapsed's word proposal: the word's alias table over its type-topic counts plus a beta * K smoothing branch.
// Per token two Metropolis-Hastings proposals, each accepted on a quotient of two short products: O(1) per token, whatever K.
//
// The tables are the ones the class declares.  LightPCLDAtypeTopicProposal.java:72-77 declares a
// TypeTopicTableBuilderFactory and installs it nowhere (`tbFactory` exists only in CollapsedLightLDA), so a JVM run inherits
// spalias's alpha * phi tables of K entries and uses the drawn TOPIC as a POSITION in nonZeroTypeTopics[type][.] (:153), which
// beyond nnz_w holds what insert-at-end and swap-remove left behind, by thread timing.  That cannot be restated and is not the
// proposal calculateWordAcceptanceProbability corrects for.  This build runs what the class and TypeTopicParallelTableBuilder
// declare: p_i = n_w,L[i] / topicCountBetaHat[L[i]] over the word's ascending list L -- count_alias_build_kernel
// (ggs_alias.hpp), unchanged, at the head of every z step on the sweep-start counts.
//
// Per non-empty document: n[k] = the topic histogram of the document's z; ni[k] is n[k] without the token in flight.  G[w][k] are
// the sweep-start type-topic counts and bhat[k] = (double)n_k + betaSum of the sweep start: unlike lightcollapsed nothing moves
// them for the token in flight (the reference's typeTopicCounts change in updateCounts only).  For each position in order, w the
// word, z0 = s = z[pos], (U1, U2, U3, U4) the token's uniforms:
//   word proposal   u_w = U1 * (tokensPerType[w] + beta * K).  u_w < tokensPerType[w]: t = L_w[generateSample(u_w /
//                   tokensPerType[w])] on the word's table of nnz_w entries; otherwise t = (int)(((u_w - tokensPerType[w]) /
//                   (beta * K)) * K) (:148-156).  If t != s (:270-272):
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (beta + G[w][s]) * bhat[t]
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (beta + G[w][t]) * bhat[s],   pi_w = nom / den
//                   (left to right, fp64, counts converted first); accepted if pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--,
//                   n[t]++, s = t.
//   doc proposal    LightPCLDA's, word for word (ggs_z_lightpc.hpp): ui = U3 * (len + alphaSum), z[doc][(int)ui] -- this sweep's
//                   topics before pos, the old ones from pos on, pos itself still z0 -- or the alpha branch; if t != s
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (alpha[s] + n[s])
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (alpha[s] + n[t]),   new = t if nom / den > 1, else if U4 < it, else s.
//                   If t == s, new = z0 (`newTopic` keeps its initial value, :130): that undoes an accepted word proposal.
//   n[s]--, z[pos] = new, n[new]++.
// IEEE as it falls: 0/0 is NaN and accepts nothing, x/0 is inf and accepts.  It is alpha[s] everywhere, and the word proposal
// weighs tokensPerType against beta * K while its acceptance assumes n_wk / bhat: the chain is approximate as written and nothing
// of it is repaired here.
//
// Ours: the uniforms are lightpclda's (U1, U2 from Philox block 0, U3, U4 from block 1 of the token's Z stream, taken whether or
// not the branch that uses them runs).  A table draw with i == nnz_w, and a beta- or alpha-branch topic == K, are
// GGS_ERR_INVALID_TOPIC, the topic clamped to the last valid one.  The three counters (ggs_get_mh_stats) are lightpclda's classes.
//
// The kernel is light_wave_body<Light::w2> (ggs_z_light.hpp: the chunk machinery, the uniforms' layout, the counters), its word
// proposal light_draw_count_table.  Computed a chunk ahead besides lightpclda's: beta + G and bhat at z0 and at the word proposal;
// the serial part per token is two quotients of three- and four-factor products.
#pragma once
#include "ggs_z_light.hpp"

namespace ggs {

__global__ __launch_bounds__(64) void lightpcw2_wave_kernel(LightCountParams lp) { light_wave_body<Light::w2>(lp); }

}  // namespace ggs
