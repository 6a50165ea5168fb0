"""The exact posterior p(z | w) of an LDA corpus small enough to enumerate, the statistics that compare a chain with it, and
a plain NumPy Gibbs sampler written from the model (not from oracle/).  A test helper, not collected.

The model: theta_d ~ Dir(alpha), phi_k ~ Dir(beta), z_i ~ theta_d(i), w_i ~ phi_z(i).  With theta and phi integrated out,

    log p(z, w) = sum_d sum_k lgamma(n_dk + alpha_k) + sum_k [sum_w lgamma(n_kw + beta) - lgamma(n_k + V beta)] + const,

which is normalised here over all K^N assignments.  The uncollapsed (ggs), the partially collapsed (pcgs, spalias) and the
serial collapsed chain all leave that distribution of z invariant; the AD-LDA schedule of the collapsed scheme and
polyaurn do not (tests/test_posterior_model.py measures how far they are).

State index convention: z[0] is the MOST significant digit, index = sum_i z[i] * K^(N-1-i) (np.ravel_multi_index).

The mutants of ReferenceSampler exist only to show that the statistics have power: each is a slip that a restatement and
its kernel could share without a parity test noticing.

scheme=spalias_priors leaves another law invariant, with the row masses of its masked Phi as a parameter: the second half of
this file ("the constrained posterior") enumerates it and has a sampler and mutants of its own.
"""
import collections
import itertools
import math

import numpy as np
from scipy import special, stats

MAX_STATES = 4096

Fixture = collections.namedtuple("Fixture", "K V alpha beta doc_ptr tokens")

# Fixture A: three documents, the last of one token; alpha asymmetric so that a wrong alpha index shows; 3^6 = 729 states.
FIXTURE_A = Fixture(K=3, V=3, alpha=(0.3, 0.9, 1.7), beta=0.4, doc_ptr=(0, 3, 5, 6), tokens=(0, 0, 1, 1, 2, 2))
PAD_ALPHA = 1e-12


def fixture_b(Kpad):
    """Fixture A's corpus with the topics padded to Kpad by alpha = 1e-12: the padded topics are (as good as) never drawn, and
    the state projected on the first three topics has fixture A's posterior to about 1e-9."""
    a = FIXTURE_A
    return a._replace(K=int(Kpad), alpha=tuple(a.alpha) + (PAD_ALPHA,) * (int(Kpad) - a.K))


Posterior = collections.namedtuple("Posterior", "K N states p e_theta e_phi")


def state_index(z, K):
    """index of one assignment z [N] (or of each row of z [T][N]); z[0] is the most significant digit"""
    z = np.asarray(z, np.int64)
    w = K ** np.arange(z.shape[-1] - 1, -1, -1, dtype=np.int64)
    return (z * w).sum(axis=-1)


def counts_of(doc_ptr, tokens, z, K, V):
    """(n_dk [D][K], n_kw [K][V]) of one assignment"""
    doc_ptr = np.asarray(doc_ptr, np.int64)
    D = doc_ptr.size - 1
    doc = np.repeat(np.arange(D), np.diff(doc_ptr))
    n_dk = np.zeros((D, K), np.int64)
    n_kw = np.zeros((K, V), np.int64)
    np.add.at(n_dk, (doc, np.asarray(z, np.int64)), 1)
    np.add.at(n_kw, (np.asarray(z, np.int64), np.asarray(tokens, np.int64)), 1)
    return n_dk, n_kw


def enumerate_posterior(doc_ptr, tokens, K, V, alpha, beta):
    """Posterior(K, N, states [K^N][N], p [K^N], E[theta | w] [D][K], E[phi | w] [K][V]); states[i] has index i."""
    N = len(tokens)
    if K ** N > MAX_STATES:
        raise ValueError("K**N = %d states: too many to enumerate (limit %d)" % (K ** N, MAX_STATES))
    alpha = np.broadcast_to(np.asarray(alpha, np.float64), (K,))
    beta = float(beta)
    lens = np.diff(np.asarray(doc_ptr, np.int64)).astype(np.float64)
    states = np.array(list(itertools.product(range(K), repeat=N)), np.int64).reshape(K ** N, N)
    logp = np.empty(len(states), np.float64)
    th = np.empty((len(states), len(lens), K), np.float64)
    ph = np.empty((len(states), K, V), np.float64)
    for i, z in enumerate(states):
        n_dk, n_kw = counts_of(doc_ptr, tokens, z, K, V)
        n_k = n_kw.sum(axis=1)
        logp[i] = special.gammaln(n_dk + alpha).sum() + special.gammaln(n_kw + beta).sum() - special.gammaln(n_k + V * beta).sum()
        th[i] = (n_dk + alpha) / (lens + alpha.sum())[:, None]
        ph[i] = (n_kw + beta) / (n_k + V * beta)[:, None]
    p = np.exp(logp - special.logsumexp(logp))
    assert (state_index(states, K) == np.arange(len(states))).all()
    return Posterior(K, N, states, p, np.tensordot(p, th, 1), np.tensordot(p, ph, 1))


Verdict = collections.namedtuple("Verdict", "chi2 dof pvalue cells tv n")


def histogram(indices, num_states):
    return np.bincount(np.asarray(indices, np.int64), minlength=num_states)


def verdict(indices, p, min_expected=5.0):
    """Pearson chi-square of the visited state indices against the probabilities p.  Every cell whose expected count is
    below min_expected goes into ONE pooled cell, which is kept: no observation is dropped.  Also the total variation
    distance between the empirical distribution and p (over the unpooled states)."""
    p = np.asarray(p, np.float64)
    obs = histogram(indices, p.size).astype(np.float64)
    n = obs.sum()
    exp = n * p
    small = exp < min_expected
    o, e = obs[~small], exp[~small]
    if small.any():
        o, e = np.append(o, obs[small].sum()), np.append(e, exp[small].sum())
    chi2 = float(((o - e) ** 2 / e).sum())
    dof = o.size - 1
    return Verdict(chi2, dof, float(stats.chi2.sf(chi2, dof)), o.size, float(0.5 * np.abs(obs / n - p).sum()), int(n))


def batch_means_z(samples, expected, batches=40):
    """z scores of the chain mean of samples [T][...] against expected [...], the standard error from the spread of the
    means of `batches` consecutive batches (T a multiple of batches; T == batches: the rows are batch means already)."""
    x = np.asarray(samples, np.float64)
    T = x.shape[0]
    if T % batches:
        raise ValueError("%d samples do not split into %d batches" % (T, batches))
    bm = x.reshape((batches, T // batches) + x.shape[1:]).mean(axis=1)
    se = bm.std(axis=0, ddof=1) / np.sqrt(batches)
    return (bm.mean(axis=0) - np.asarray(expected, np.float64)) / se


def run_chain(step, get_z, K, n, thin, burn_in=50, max_topic=None):
    """The recipe every chain is measured by: burn_in sweeps, then n samples of the whole z vector, one every thin sweeps.
    step(m) advances the chain by m sweeps.  Returns the state indices [n] in base K; with max_topic every sampled z must
    stay at or below it (fixture B: a padded topic was drawn otherwise)."""
    out = np.empty(n, np.int64)
    step(burn_in)
    for i in range(n):
        step(thin)
        z = np.asarray(get_z(), np.int64)
        if max_topic is not None and z.max() > max_topic:
            raise AssertionError("sample %d: topic %d drawn, above %d" % (i, z.max(), max_topic))
        out[i] = state_index(z, K)
    return out


N_SAMPLES = 4000
# the longer pcgs chain: the pcgs chain forgets a perturbed draw about twice as fast as the ggs chain, so the late-walk slip
# moves its stationary distribution half as far -- measured with the NumPy sampler (seed 1, thin 4): p = 0.29 at n = 4000,
# 0.006 at 8000, 6e-8 at 12000
N_LONG = 12000
BURN_IN = 50
# sweeps between two samples: the lag at which a scheme's samples of z are as good as independent on fixture A (at thin 4 the
# ggs chain's lag autocorrelation of a state indicator is still 0.065, and a correct chain is rejected)
THIN = {"ggs": 8, "pcgs": 4, "spalias": 4, "collapsed": 2, "collapsed_parallel": 2, "polyaurn": 4, "spalias_priors": 4}


def oracle_chain(O, fixture, scheme, seed, n=N_SAMPLES):
    """State indices (base 3) of n samples of a chain of the CPU oracle O (the module oracle.oracle), started the way the
    parity tests start a sampler: seeded z0, initial Phi."""
    o = O.OracleSampler(fixture.K, fixture.V, np.asarray(fixture.alpha), fixture.beta, seed)
    if scheme == "pcgs":
        o.set_scheme("pcgs")
    o.set_corpus(fixture.doc_ptr, np.asarray(fixture.tokens, np.int32))
    o.init_z_java_lcg(seed)
    o.init_phi()
    step = {"ggs": o.sweep, "pcgs": o.sweep, "collapsed": lambda m: o.collapsed_sweep(seed, m),
            "collapsed_parallel": o.collapsed_parallel_sweep}[scheme]
    idx = run_chain(step, o.get_z, 3, n, THIN[scheme], BURN_IN, max_topic=2)
    o.close()
    return idx


def spalias_chain(O, fixture, seed, n=N_SAMPLES):
    """The same for tests/spalias_restatement.Model, from the z0 that init_z_java_lcg(seed) gives"""
    from tests import spalias_restatement as R
    z0 = O.jrandom_ints(seed, fixture.K, len(fixture.tokens))
    m = R.Model(fixture.K, fixture.V, np.asarray(fixture.alpha), fixture.beta, seed, fixture.doc_ptr, fixture.tokens, z0)
    m.init_phi()
    return run_chain(m.sweep, lambda: m.z, 3, n, THIN["spalias"], BURN_IN, max_topic=2)


MUTANTS = (None, "beta_double", "no_exclude", "alpha_reversed", "walk_late")
# the scheme whose sampler a slip imitates: the Phi draw, the theta draw and the CDF walk of the uncollapsed sweep (GGS:57-198),
# the count-form conditional of pcgs (UPLDA:1466-1544)
MUTANT_SCHEME = {"beta_double": "ggs", "no_exclude": "pcgs", "alpha_reversed": "ggs", "walk_late": "ggs"}


class ReferenceSampler:
    """Gibbs samplers for p(z | w) from the model's own conditionals, in NumPy.

    scheme "ggs":   theta_d | z ~ Dir(alpha + n_d.),  phi_k | z ~ Dir(beta + n_k.),  then every z_i | theta, phi
                    independently, p(z_i = k) ~ theta_dk phi_kw.
    scheme "pcgs":  phi_k | z ~ Dir(beta + n_k.), then z_i | z_-i, phi token after token,
                    p(z_i = k) ~ (n_dk^-i + alpha_k) phi_kw  (theta integrated out; the current token excluded).

    A topic is drawn the way the samplers under test draw it: u ~ U[0, 1), walk the cumulative scores until they pass
    u * total.

    mutant: None, or one slip --
      "beta_double"     the Phi draw uses 2 beta
      "no_exclude"      the pcgs conditional counts the current token (n_dk instead of n_dk^-i)
      "alpha_reversed"  alpha is read back to front
      "walk_late"       with probability 0.03 the walk lands one topic late (clamped to K - 1, as a kernel would)
    """

    def __init__(self, fixture, scheme, seed, mutant=None):
        if scheme not in ("ggs", "pcgs") or mutant not in MUTANTS:
            raise ValueError("scheme %r / mutant %r" % (scheme, mutant))
        if mutant == "no_exclude" and scheme != "pcgs":
            raise ValueError("no_exclude is a slip of the pcgs conditional")
        self.K, self.V, self.scheme, self.mutant = fixture.K, fixture.V, scheme, mutant
        self.alpha = np.broadcast_to(np.asarray(fixture.alpha, np.float64), (self.K,)).copy()
        if mutant == "alpha_reversed":
            self.alpha = self.alpha[::-1].copy()
        self.beta_phi = fixture.beta * (2.0 if mutant == "beta_double" else 1.0)
        self.doc_ptr = np.asarray(fixture.doc_ptr, np.int64)
        self.tokens = np.asarray(fixture.tokens, np.int64)
        self.doc = np.repeat(np.arange(self.doc_ptr.size - 1), np.diff(self.doc_ptr))
        self.rng = np.random.default_rng(seed)
        self.z = self.rng.integers(0, self.K, self.tokens.size)
        self.theta = self.phi = None

    def _walk(self, scores):
        """scores [..., K] -> topics [...]"""
        cum = np.cumsum(scores, axis=-1)
        u = self.rng.random(cum.shape[:-1])
        k = (cum < (u * cum[..., -1])[..., None]).sum(axis=-1)     # the first k whose cumulative score reaches u * total
        if self.mutant == "walk_late":
            k = k + (self.rng.random(k.shape) < 0.03)
        return np.minimum(k, self.K - 1)

    def _dirichlet(self, shape):
        g = self.rng.standard_gamma(shape)
        return g / g.sum(axis=-1, keepdims=True)

    def sweep(self, n=1):
        for _ in range(n):
            n_dk, n_kw = counts_of(self.doc_ptr, self.tokens, self.z, self.K, self.V)
            self.phi = self._dirichlet(n_kw + self.beta_phi)
            if self.scheme == "ggs":
                self.theta = self._dirichlet(n_dk + self.alpha)
                self.z = self._walk(self.theta[self.doc] * self.phi[:, self.tokens].T)
            else:
                for i in range(self.tokens.size):
                    d = self.doc[i]
                    if self.mutant != "no_exclude":
                        n_dk[d, self.z[i]] -= 1
                    new = int(self._walk((n_dk[d] + self.alpha) * self.phi[:, self.tokens[i]]))
                    if self.mutant == "no_exclude":
                        n_dk[d, self.z[i]] -= 1
                    n_dk[d, new] += 1
                    self.z[i] = new

    def get_z(self):
        return self.z


# ---- scheme=spalias_priors: the constrained posterior -----------------------------------------------------------------
# Topic priors P [K][V] in {0, 1}; A_k the words topic k is allowed.  The initial Phi is the unconstrained draw times P, rows
# not renormalised, and every sweep rescales row k to the mass it had: m_k = sum_v P_kv phi0_kv is a constant of the chain.
# With phi_k = m_k psi_k, psi_k on the simplex over A_k, a sweep is
#     psi_k | z ~ Dir(beta + n_k.) over A_k          (the draw's ((beta + n) / mag) * mag shape is beta + n to an ulp)
#     p(z_i = k | z_-i, psi) ~ (n_dk^-i + alpha_k) m_k psi_k[w_i]
# the two Gibbs conditionals of
#     p(z | w, m) ~ prod_d prod_k Gamma(n_dk + alpha_k)
#                   * prod_k [ m_k^n_k * prod_{v in A_k} Gamma(n_kv + beta) / Gamma(n_k + |A_k| beta) ],
# zero for a z that puts a token on a masked (topic, word) cell.
#
# The fixture: fixture A with two cells masked.  Word 2 is the one-token document's, so that document's alias-only draw meets
# a zero weight.  For a padded K every padded topic k is masked at word k mod 3 (mask bits 3 ... K - 1 set, across the 32-bit
# words of the device's bit mask); every topic keeps two allowed words and every word an allowed topic.
PRIOR_CELLS = ((0, 2), (1, 2))                                      # (topics, words): cells (0, 1) and (2, 2)
PRIOR_CELLS_RB = ((0, 2), (1, 0))                                   # the Rao-Blackwell check's mask: cells (0, 1) and (2, 0)


def prior_cells(K, base=PRIOR_CELLS):
    """(topics, words) int32: base, plus (k, k mod 3) for every padded topic k >= 3"""
    t, w = list(base[0]) + list(range(3, K)), list(base[1]) + [k % 3 for k in range(3, K)]
    return np.asarray(t, np.int32), np.asarray(w, np.int32)


def prior_matrix(K, V, cells):
    """[K][V] float64, 0.0 at the cells and 1.0 elsewhere (written here, not taken from the code under test)"""
    P = np.ones((K, V), np.float64)
    for k, v in zip(*cells):
        P[int(k), int(v)] = 0.0
    return P


def enumerate_constrained_posterior(fixture, P, m):
    """The law above on fixture's corpus: Posterior with p = 0 off the support, e_theta = E[(n_dk + alpha_k) / (N_d + sum alpha)]
    and e_phi = E[m_k P_kv (n_kv + beta) / (n_k + |A_k| beta)]."""
    K, V, N = fixture.K, fixture.V, len(fixture.tokens)
    if K ** N > MAX_STATES:
        raise ValueError("K**N = %d states: too many to enumerate (limit %d)" % (K ** N, MAX_STATES))
    P = np.asarray(P, np.float64)
    m = np.broadcast_to(np.asarray(m, np.float64), (K,))
    if P.shape != (K, V) or not np.isin(P, (0.0, 1.0)).all() or not (m > 0).all():
        raise ValueError("P must be [K][V] in {0, 1} and m positive")
    alpha = np.broadcast_to(np.asarray(fixture.alpha, np.float64), (K,))
    beta = float(fixture.beta)
    allowed = P != 0.0
    n_allowed = allowed.sum(axis=1).astype(np.float64)
    lens = np.diff(np.asarray(fixture.doc_ptr, np.int64)).astype(np.float64)
    states = np.array(list(itertools.product(range(K), repeat=N)), np.int64).reshape(K ** N, N)
    logp = np.full(len(states), -np.inf, np.float64)
    th = np.zeros((len(states), len(lens), K), np.float64)
    ph = np.zeros((len(states), K, V), np.float64)
    for i, z in enumerate(states):
        n_dk, n_kw = counts_of(fixture.doc_ptr, fixture.tokens, z, K, V)
        if n_kw[~allowed].any():
            continue
        n_k = n_kw.sum(axis=1)
        logp[i] = (special.gammaln(n_dk + alpha).sum() + special.gammaln(n_kw + beta)[allowed].sum()
                   - special.gammaln(n_k + n_allowed * beta).sum() + (n_k * np.log(m)).sum())
        th[i] = (n_dk + alpha) / (lens + alpha.sum())[:, None]
        ph[i] = m[:, None] * P * (n_kw + beta) / (n_k + n_allowed * beta)[:, None]
    p = np.exp(logp - special.logsumexp(logp))
    return Posterior(K, N, states, p, np.tensordot(p, th, 1), np.tensordot(p, ph, 1))


def off_support(indices, p):
    """how many of the visited states have probability 0"""
    return int((np.asarray(p)[np.asarray(indices, np.int64)] == 0.0).sum())


CONSTRAINED_MUTANTS = (None, "renormalised", "beta_double", "mask_transposed")


class ConstrainedSampler:
    """A Gibbs sampler of the constrained law from its two conditionals, in NumPy; it starts from a z inside the support.

    mutant: None, or one slip --
      "renormalised"     the rows of Phi are normalised to 1: the mass m_k is dropped from the z step
      "beta_double"      the Phi draw uses 2 beta
      "mask_transposed"  P is read as [V][K] (K == V)
    """

    def __init__(self, fixture, P, m, seed, mutant=None):
        if mutant not in CONSTRAINED_MUTANTS:
            raise ValueError("mutant %r" % (mutant,))
        self.K, self.V, self.mutant = fixture.K, fixture.V, mutant
        P = np.asarray(P, np.float64)
        self.P = np.ascontiguousarray(P.T) if mutant == "mask_transposed" else P.copy()
        self.m = np.broadcast_to(np.asarray(m, np.float64), (self.K,)).copy()
        self.alpha = np.broadcast_to(np.asarray(fixture.alpha, np.float64), (self.K,)).copy()
        self.beta_phi = fixture.beta * (2.0 if mutant == "beta_double" else 1.0)
        self.doc_ptr = np.asarray(fixture.doc_ptr, np.int64)
        self.tokens = np.asarray(fixture.tokens, np.int64)
        self.doc = np.repeat(np.arange(self.doc_ptr.size - 1), np.diff(self.doc_ptr))
        self.rng = np.random.default_rng(seed)
        self.z = np.array([self.rng.choice(np.flatnonzero(self.P[:, w] != 0.0)) for w in self.tokens], np.int64)
        self.phi = None

    def sweep(self, n=1):
        for _ in range(n):
            n_dk, n_kw = counts_of(self.doc_ptr, self.tokens, self.z, self.K, self.V)
            g = self.rng.standard_gamma(n_kw + self.beta_phi) * self.P
            self.phi = g / g.sum(axis=1, keepdims=True)
            if self.mutant != "renormalised":
                self.phi = self.phi * self.m[:, None]
            for i in range(self.tokens.size):
                d = self.doc[i]
                n_dk[d, self.z[i]] -= 1
                cum = np.cumsum((n_dk[d] + self.alpha) * self.phi[:, self.tokens[i]])
                new = min(int((cum < self.rng.random() * cum[-1]).sum()), self.K - 1)
                n_dk[d, new] += 1
                self.z[i] = new

    def get_z(self):
        return self.z


def exact_row_sums(phi):
    """row sums without a rounding of their own (math.fsum): nothing of the measurement in the figure"""
    return np.asarray([math.fsum(row) for row in np.asarray(phi, np.float64).tolist()])


def oracle_row_masses(O, fixture, cells, seed):
    """(m [K], phi0 * P [K][V]): the CPU oracle's unmasked initial Phi of a sampler seeded like the parity tests seed one, times
    the prior matrix, and its row sums -- the reference for the chain's constant, not the code under test."""
    o = O.OracleSampler(fixture.K, fixture.V, np.asarray(fixture.alpha), fixture.beta, seed)
    o.set_corpus(fixture.doc_ptr, np.asarray(fixture.tokens, np.int32))
    o.init_z_java_lcg(seed)
    o.init_phi()
    phi0 = o.get_phi() * prior_matrix(fixture.K, fixture.V, cells)
    o.close()
    return exact_row_sums(phi0), phi0


def mass_bound(sweeps, V):
    """relative drift of a row's mass after `sweeps` sweeps: a sweep sums the V cells of the old row (one rounding per summand)
    and rescales the new row to that sum (a division and a multiplication per cell); at worst the roundings add up linearly"""
    return sweeps * (V + 2) * 2.0 ** -53


def spalias_priors_chain(O, fixture, cells, seed, n=N_SAMPLES, masses=None):
    """(state indices base 3 [n], m [K]) of tests/spalias_priors_restatement.Model under the prior cells, from the z0 that
    init_z_java_lcg(seed) gives; m from oracle_row_masses.  masses, a list, receives the model's exact row sums after the
    initial draw, after the burn-in and at the end."""
    from tests import spalias_priors_restatement as PR
    m, _ = oracle_row_masses(O, fixture, cells, seed)
    z0 = O.jrandom_ints(seed, fixture.K, len(fixture.tokens))
    mdl = PR.Model(fixture.K, fixture.V, np.asarray(fixture.alpha), fixture.beta, seed, fixture.doc_ptr, fixture.tokens, z0, cells=cells)
    mdl.init_phi()
    note = (lambda: masses.append(exact_row_sums(mdl.phi))) if masses is not None else (lambda: None)
    note()
    mdl.sweep(BURN_IN)
    note()
    idx = run_chain(mdl.sweep, lambda: mdl.z, 3, n, THIN["spalias_priors"], 0, max_topic=2)
    note()
    return idx, m
