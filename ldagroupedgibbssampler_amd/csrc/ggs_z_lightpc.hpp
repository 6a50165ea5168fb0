// ggs_z_lightpc.hpp -- the z loop of scheme=lightpclda (LightPCLDA.java:86-221; ParallelLDA.java:469-473): the LightLDA
// sampler of Yuan et al. over the partially collapsed model.  Per token two Metropolis-Hastings proposals, one from the
// word's alias table and one from the document's own indicator array, each accepted on a ratio of a handful of numbers:
// O(1) per token, whatever K.
//
// The tables are spalias's.  LightPCLDA.java:50-83 declares a PhiTableBuilderFactory, but nothing installs it (`tbFactory`
// exists only in CollapsedLightLDA); the inherited doPreIterationTableBuling (SpaliasUncollapsedParallelLDA.java:83-115)
// builds PhiAlphaParallelTableBuilder tables, so a running LightPCLDA draws its word proposal from
// pi[k] = phi[k][w] * alpha[k] -- alias_build_kernel (ggs_alias.hpp), unchanged.
//
// The reference as it runs, per non-empty document: n[k] = the topic histogram of the document's z; ni[k] is n[k] without
// the token in flight (the reference keeps it as a second array of doubles; here it is n[k] - (k == s), no array).  For
// each position in order, w the word, z0 = s = z[pos], (U1, U2, U3, U4) the token's uniforms:
//   word proposal   t = the alias draw of w at U1.  If t != s: pi_w = (alpha[s] + ni[t]) / (alpha[s] + ni[s]); accepted if
//                   pi_w > 1, else if U2 < pi_w.  Accepted: n[s]--, n[t]++, s = t.
//   doc proposal    ui = U3 * (len + alphaSum).  ui < len: t = z[doc][(int)ui] -- the array holds this sweep's new topics
//                   before pos and the old ones from pos on, position pos itself still z0, not s.  Otherwise
//                   t = (int)(((ui - len) / alphaSum) * K).  If t != s:
//                     nom = phi[t][w] * (alpha[s] + ni[t]) * (alpha[s] + n[s])
//                     den = phi[s][w] * (alpha[s] + ni[s]) * (alpha[s] + n[t]),   ratio = nom / den
//                   (left to right, fp64, counts converted first); new = t if ratio > 1, else if U4 < ratio, else s.
//                   If t == s the reference assigns nothing and `newTopic` still holds its initial value (LightPCLDA.java:115):
//                   new = z0, which undoes an accepted word proposal.  IEEE as it falls: 0/0 is NaN and accepts nothing,
//                   x/0 is inf and accepts.
//   n[s]--, z[pos] = new, n[new]++.
// It is alpha[s] everywhere (right for symmetric alpha only), the document proposal is treated as state independent and
// reads z0 after an accepted word proposal: the chain is approximate by design and nothing of it is repaired here.
//
// Ours: U1, U2 are the two doubles of Philox block 0 and U3, U4 those of block 1 of the token's Z stream (purpose Z,
// element = global token index), taken at these positions whether or not the branch that uses them runs; U1 is the
// uniform every other scheme's token draws.  alphaSum is the k-order sum of alpha.  An alias draw with i == K, and an
// alpha-branch topic == K (ui rounded up to len + alphaSum; Java would index out of bounds), are GGS_ERR_INVALID_TOPIC, the
// topic clamped to K - 1.  The three counters (ggs_get_mh_stats) classify a token by where its new topic came from: the
// document proposal accepted; else the word proposal accepted and kept; else left on z0.
//
//
// The kernel is light_wave_body<Light::pc> (ggs_z_light.hpp: the chunk machinery, the uniforms' layout, the counters), its word
// proposal light_draw_alias_cell, pi_w and pi_d the two quotients above.
#pragma once
#include "ggs_z_light.hpp"

namespace ggs {

__global__ __launch_bounds__(64) void lightpc_wave_kernel(LightpcParams lp) { light_wave_body<Light::pc>(lp); }

}  // namespace ggs
