#!/usr/bin/env python3
"""scheme=spalias against scheme=pcgs, in one process, on the legs DESIGN.md ("6c. Scheme spalias") quotes: one JSON line
per (leg, state, scheme) with ms_per_sweep, the per-sweep phases of ggs_get_timings, the kernel that ran and the mean
number of non-zero topics per document (nnz_d) of the state timed.  One handle at a time.  Legs as scripts/time_polyaurn.py:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
States: "warm" = after the warm-up sweeps from the random start; "burned" = after --burn spalias sweeps.  pcgs is timed from
the SAME z (ggs_set_z, Phi redrawn), so both schemes see the same sparsity.  The table build has no phase of its own in
ggs_get_timings (it is counted in phi_ms): alias_build_ms is the spalias leg's phi_ms less the pcgs leg's of the same
state, the two Phi phases being otherwise the same kernels on the same counts.
usage: python scripts/time_spalias.py [--legs config2,k1024] [--steps N] [--warmup W] [--burn B] [--out FILE]"""
import argparse
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


def mean_nnz(corpus, z, K):
    doc = np.repeat(np.arange(corpus.num_docs, dtype=np.int64), np.diff(corpus.doc_ptr))
    return float(np.unique(doc * K + z).size) / max(1, int((np.diff(corpus.doc_ptr) > 0).sum()))


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
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    return h


def leg(name, corpus, K, steps, warmup, burn, emit):
    base = {"leg": name, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens, "steps": steps}
    states = {}
    h = handle("spalias", corpus, K)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    states["warm"] = h.get_z()
    rows = {}
    ms, ph = timed(h, steps)
    rows[("warm", "spalias")] = dict(ms_per_sweep=ms, phase_ms=ph, z_kernel=h.launch_info()["z_kernel"])
    h.set_z(states["warm"], redraw_phi=True)
    h.sweep(burn)
    states["burned"] = h.get_z()
    ms, ph = timed(h, steps)
    rows[("burned", "spalias")] = dict(ms_per_sweep=ms, phase_ms=ph, z_kernel=h.launch_info()["z_kernel"])
    h.close()
    for state in ("warm", "burned"):
        h = handle("pcgs", corpus, K)
        h.set_z(states[state], redraw_phi=True)
        ms, ph = timed(h, steps)
        rows[(state, "pcgs")] = dict(ms_per_sweep=ms, phase_ms=ph, z_kernel=h.launch_info()["z_kernel"])
        h.close()
    for state in ("warm", "burned"):
        nnz = round(mean_nnz(corpus, states[state], K), 2)
        build = round(rows[(state, "spalias")]["phase_ms"]["phi_ms"] - rows[(state, "pcgs")]["phase_ms"]["phi_ms"], 4)
        for scheme in ("spalias", "pcgs"):
            r = dict(base, state=state, sweeps_before={"warm": warmup, "burned": burn}[state], scheme=scheme, mean_nnz_d=nnz, **rows[(state, scheme)])
            if scheme == "spalias":
                r["alias_build_ms"] = build
            emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--steps", type=int, default=10)
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
            leg(name, corpus, 100, args.steps, args.warmup, args.burn, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, max(3, args.steps // 2), args.warmup, args.burn, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
