// ggs_z_lightcollapsed.hpp -- scheme=lightcollapsed (CollapsedLightLDA.java; ParallelLDA.java:429-433): the LightLDA sampler of
// Yuan et al. over the COLLAPSED model.  No theta, no Phi: the state is z, the type-topic counts and tokensPerTopic.  Per
// token two Metropolis-Hastings proposals, one from the word's alias table over the counts and one from the document's own
// indicator array, each accepted on a product of a handful of quotients: O(1) per token, whatever K.
//
// The schedule is scheme=collapsed's parallel one: AD-LDA with one worker per document.  The reference gives
// every document batch a private copy of typeTopicCounts / tokensPerTopic (CollapsedLightLDA.java:795-802) and moves it with
// balanceGlobalCounts (:1130-1135); with one document per worker and the rule of the collapsed schedule -- a document is
// sampled against the counts as they stood at the start of the sweep, minus the token being resampled -- that copy shrinks
// to the sweep-start counts with the token in flight moved.  While a token of word w is processed, z0 its old topic and s its
// current one (z0, or an accepted word proposal):
//     G(k) = n_wk[start][w][k] - [k == z0] + [k == s]      stands for globalTypeTopicCounts[type][k]
//     T(k) = n_k[start][k]     - [k == z0] + [k == s]      stands for globalTokensPerTopic[k]
// Earlier tokens of the same document do not move G or T.  n[k] is the document's histogram with the token in flight (at s)
// and ni[k] = n[k] - [k == s]; both run along the document as in the reference (localTopicCounts, localTopicCounts_i).
//
// Per token, (U1, U2, U3, U4) its uniforms, b = beta, bS = betaSum = beta * V, counts converted to double first, the quotients
// multiplied left to right as calculateWordAcceptanceProbability (:1094-1128) and calculateDocumentAcceptanceProbability
// (:1050-1091) multiply them:
//   word proposal  u_w = U1 * (tokensPerType[w] + beta * K).  u_w < tokensPerType[w]: t = list_w[generateSample(u_w /
//                  tokensPerType[w])] on the word's table of nnz_w entries (ups = u * nnz, i = (int)ups, (ups - i) > ps[i] ?
//                  a[i] : i); otherwise t = (int)(((u_w - tokensPerType[w]) / (beta * K)) * K) (:946-954).  If t != z0, with
//                  s = z0 and a = alpha[z0]:
//                    pi_w = (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1)) * (bS + (T(s) - 1)) / (bS + T(t))
//                                                     * (b + G(s)) / (b + G(t))       * (bS + T(t)) / (bS + T(s))
//                  accepted if pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--, n[t]++, s = t (G and T follow by definition).
//   doc proposal   t exactly as in LightPCLDA (ggs_z_lightpc.hpp: ui = U3 * (len + alphaSum), z[doc][(int)ui] -- this sweep's
//                  topics before the position, the old ones from it on -- or the alpha branch).  If t != s, a = alpha[s]:
//                    pi_d = (a + ni[t]) / (a + ni[s]) * (b + G(t)) / (b + (G(s) - 1)) * (bS + (T(s) - 1)) / (bS + T(t))
//                                                     * (a + n[s]) / (a + n[t])
//                  new = t if pi_d > 1, else if U4 < pi_d, else s.  If t == s, new = z0 (`newTopic` keeps its initial value,
//                  :928, :1008): that undoes an accepted word proposal.
//   n[s]--, z[pos] = new, n[new]++.
// It is alpha[oldTopic] everywhere, and the word proposal weighs tokensPerType against beta * K while its acceptance assumes
// (n_wk + beta) / (n_k + betaSum): the chain is approximate as written and nothing of it is repaired here.
//
// Ours: the uniforms are lightpclda's (U1, U2 from Philox block 0, U3, U4 from block 1 of the token's Z stream, taken whether or
// not the branch that uses them runs).  A word's list is in ascending topic order; topicCountBetaHat[k] = (double)n_k + betaSum,
// afresh each sweep; tokensPerType[w] = the integer sum of the word's sweep-start row.  A table draw with i == nnz, and a
// beta- or alpha-branch topic == K, are GGS_ERR_INVALID_TOPIC, the topic clamped to the last valid one.  The three counters
// (ggs_get_mh_stats) are lightpclda's three classes.
//
// The kernel is light_wave_body<Light::collapsed> (ggs_z_light.hpp: the chunk machinery, the uniforms' layout, the counters), its
// word proposal light_draw_count_table on the tables of count_alias_build_kernel (ggs_alias.hpp).  Computed a chunk ahead: the
// count cells n_wk and n_k at z0 and at the word proposal, the four quotients of pi_w that do not involve the document and,
// where the document proposal is known ahead, its count cells and the two count quotients of pi_d for both outcomes of the word
// proposal (n_k is read from global memory: K cells that stay in cache).  The serial part per token is two divisions and seven
// multiplies; a token whose (int)ui is an earlier position of the SAME chunk loads its two count cells and divides twice more.
#pragma once
#include "ggs_z_light.hpp"

namespace ggs {

__global__ __launch_bounds__(64) void lightcollapsed_wave_kernel(LightCountParams lp) { light_wave_body<Light::collapsed>(lp); }

}  // namespace ggs
