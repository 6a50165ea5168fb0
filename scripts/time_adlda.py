#!/usr/bin/env python3
"""scheme=adlda against scheme=collapsed's parallel schedule and scheme=lightcollapsed, in one process, on the legs DESIGN.md
("6i. Scheme adlda") quotes: one JSON line per (leg, state, scheme) with ms_per_sweep and the per-sweep phases of
ggs_get_timings, each as median / min / max over --windows timed windows of --steps sweeps that ALTERNATE between the three
schemes' handles, so that a drift of the clocks hits all of them; the kernel that ran; for adlda the share of the tokens
drawn from each bucket (Q: the word's, R: the document's, S: smoothing) and the token-weighted mean numbers of candidates
over the sweeps timed; and one line per (leg, state) with the spread of the per-window ratios of the sweeps.  Legs as
scripts/time_lightcollapsed.py:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
States: "warm" = after the warm-up sweeps from the random start; "burned" = after --burn further sweeps -- both of the
collapsed parallel chain, so the schemes are timed from the SAME z (ggs_set_z) and see the same sparsity of the counts.
The sweep head (adlda_head_kernel and the words' lists) runs at the head of the z step and is counted in z_ms.
mean_candidates is ggs_get_sparse_stats' out[3] over the tokens sampled: nnz_w + nnz_d per token.  mean_nnz_w is the
token-weighted mean of the lists' lengths (ggs_get_word_topic_lists), averaged over the counts before and after the timed
windows; mean_nnz_d is the difference of the two.
usage: python scripts/time_adlda.py [--legs config2,k1024] [--steps N] [--windows R] [--warmup W] [--burn B] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import synthetic_lda_corpus  # noqa: E402

SEED, ALPHA, BETA = 2019, 0.1, 0.01
SCHEMES = ("adlda", "collapsed", "lightcollapsed")
FLAGS = {s: native.SCHEME_FLAGS[s] for s in SCHEMES}


def timed(h, steps):
    h.synchronize()
    h.reset_timings()
    t0 = time.perf_counter()
    h.sweep(steps)
    h.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tm = h.get_timings()
    return round(dt * 1e3, 4), {k: round(tm[k] / steps, 4) for k in ("theta_ms", "z_ms", "merge_ms", "phi_ms", "exchange_ms")}


def handle(scheme, corpus, K):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    return h


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def token_weighted_nnz_w(h, word_freq):
    nw = np.empty(h.V, np.int32)                                    # the lists' lengths are all that is copied back
    h._chk(h._L.ggs_get_word_topic_lists(h._h, nw.ctypes.data_as(C.POINTER(C.c_int32)), None))
    return float((nw.astype(np.float64) * word_freq).sum() / word_freq.sum())


def leg(name, corpus, K, steps, warmup, burn, windows, emit):
    base = {"leg": name, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens, "steps_per_window": steps,
            "windows": windows}
    word_freq = np.bincount(corpus.tokens, minlength=corpus.num_types).astype(np.float64)
    states = {}
    h = handle("collapsed", corpus, K)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    states["warm"] = h.get_z()
    h.sweep(burn)
    states["burned"] = h.get_z()
    h.close()
    for state in ("warm", "burned"):
        hs, rows = {}, {s: dict(ms=[], z=[], merge=[], phi=[]) for s in SCHEMES}
        for scheme in SCHEMES:                                      # all handles live, the windows alternate between them
            hs[scheme] = handle(scheme, corpus, K)
            hs[scheme].set_z(states[state], redraw_phi=True)
            hs[scheme].sweep(1)                                     # the first z step of a corpus is not the steady one
        before = hs["adlda"].sparse_stats()
        nnz_w = token_weighted_nnz_w(hs["adlda"], word_freq)
        for _ in range(windows):
            for scheme in SCHEMES:
                ms, ph = timed(hs[scheme], steps)
                r = rows[scheme]
                r["ms"].append(ms); r["z"].append(ph["z_ms"]); r["merge"].append(ph["merge_ms"]); r["phi"].append(ph["phi_ms"])
        d = (hs["adlda"].sparse_stats() - before).astype(np.float64)
        nnz_w = 0.5 * (nnz_w + token_weighted_nnz_w(hs["adlda"], word_freq))
        sampled = float(windows * steps * corpus.num_tokens)
        for scheme in SCHEMES:
            r = rows[scheme]
            out = dict(base, state=state, sweeps_before={"warm": warmup, "burned": warmup + burn}[state], scheme=scheme, ms_per_sweep=spread(r["ms"]),
                       z_ms=spread(r["z"]), merge_ms=spread(r["merge"]), phi_ms=spread(r["phi"]), z_kernel=hs[scheme].launch_info()["z_kernel"])
            if scheme == "adlda":
                out["bucket_shares"] = dict(Q=round(d[0] / sampled, 4), R=round(d[1] / sampled, 4), S=round(d[2] / sampled, 4))
                out["mean_candidates"] = round(d[3] / sampled, 2)
                out["mean_nnz_w"] = round(nnz_w, 2)
                out["mean_nnz_d"] = round(d[3] / sampled - nnz_w, 2)
                out["lds_bytes_z"] = hs[scheme].launch_info()["lds_bytes_z"]
            emit(out)
        emit(dict(base, state=state,
                  ratio_collapsed_over_adlda=spread([c / a for c, a in zip(rows["collapsed"]["ms"], rows["adlda"]["ms"])]),
                  ratio_lightcollapsed_over_adlda=spread([c / a for c, a in zip(rows["lightcollapsed"]["ms"], rows["adlda"]["ms"])])))
        for scheme in SCHEMES:
            hs[scheme].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--steps", type=int, default=20, help="sweeps per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per scheme and state, alternating between the schemes")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn", type=int, default=200)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    corpus = synthetic_lda_corpus(100000, 50000, 200, true_topics=100, seed=SEED)
    for name in args.legs.split(","):
        if name == "config2":
            leg(name, corpus, 100, args.steps, args.warmup, args.burn, args.windows, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, max(3, args.steps // 2), args.warmup, args.burn, args.windows, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
