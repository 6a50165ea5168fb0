#!/usr/bin/env python3
"""scheme=nzvsspalias against scheme=spalias and scheme=polyaurn_sparse, in one process, on the legs DESIGN.md ("6h. Scheme
nzvsspalias") quotes: one JSON line per (leg, state, scheme) with the medians over --windows windows of --steps sweeps of
ms_per_sweep and of the per-sweep phases of ggs_get_timings, and the kernel that ran.  The nzvsspalias lines also carry the
rounds of the indicator chain (the largest per topic of the last draw, ggs_get_vs_stats), the share of undrawn and of zero
cells, and the share of tokens per list kind and the mean number of candidates (ggs_get_sparse_stats over the timed sweeps).
One handle at a time; the schemes take turns window by window (a fresh handle from the same z each turn), so that a drift of
the machine falls on all three alike.  Legs as scripts/time_polyaurn_sparse.py:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
States: "warm" = after the warm-up sweeps from the random start; "burned" = after --burn nzvsspalias sweeps.
ggs_get_timings has one phase for the whole Phi step.  What the script can separate is
  phi_ms (nzvsspalias) - phi_ms (spalias) = the indicator chain + the list build + (the masked draw - pcgs's draw),
spalias's phi_ms being pcgs's draw + the alias tables, which nzvsspalias builds with the same kernel: phi_over_spalias_ms.
usage: python scripts/time_nzvs.py [--legs config2,k1024] [--steps N] [--windows W] [--warmup W] [--burn B] [--out FILE]"""
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
FLAGS = {s: native.SCHEME_FLAGS[s] for s in ("nzvsspalias", "spalias", "polyaurn_sparse")}
PHASES = ("theta_ms", "z_ms", "merge_ms", "phi_ms", "exchange_ms")
DEFAULT_OUT = os.path.join(ROOT, "profiles", "nzvs_bench.jsonl")


def window(h, steps):
    h.synchronize()
    h.reset_timings()
    t0 = time.perf_counter()
    h.sweep(steps)
    h.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tm = h.get_timings()
    return dict(ms_per_sweep=dt * 1e3, **{k: tm[k] / steps for k in PHASES})


def handle(scheme, corpus, K, z):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.set_z(z, redraw_phi=True)
    return h


def turn(scheme, corpus, K, z, steps):
    """one window of one scheme from z: a sweep to get past the initial Phi (nzvsspalias's lists are empty before it), then
    the timed sweeps"""
    h = handle(scheme, corpus, K, z)
    h.sweep(1)
    extra = {}
    before = h.sparse_stats() if scheme != "spalias" else None
    row = window(h, steps)
    if before is not None:
        d = (h.sparse_stats() - before).astype(np.float64)
        tokens = max(1.0, float(d[:3].sum()))
        extra.update(share_word_list=d[0] / tokens, share_doc_list=d[1] / tokens, share_no_candidate=d[2] / tokens, mean_n=d[3] / tokens)
    if scheme == "nzvsspalias":
        vs = h.vs_stats()
        cells = float(K) * corpus.num_types
        extra.update(rounds_max=int(vs[2]), share_undrawn=vs[0] / cells, share_zero=vs[1] / cells)
    row.update(extra, z_kernel=h.launch_info()["z_kernel"])
    h.close()
    return row


def median_row(rows):
    out = {}
    for k, v in rows[0].items():
        out[k] = v if isinstance(v, str) else round(float(np.median([r[k] for r in rows])), 5)
    return out


def leg(name, corpus, K, steps, windows, warmup, burn, emit):
    base = {"leg": name, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens, "steps": steps, "windows": windows}
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=FLAGS["nzvsspalias"])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    states = {"warm": h.get_z()}
    h.sweep(max(0, burn - warmup))
    states["burned"] = h.get_z()
    h.close()
    for state in ("warm", "burned"):
        rows = {s: [] for s in FLAGS}
        for _ in range(windows):                                    # the schemes take turns
            for scheme in FLAGS:
                rows[scheme].append(turn(scheme, corpus, K, states[state], steps))
        med = {s: median_row(rows[s]) for s in FLAGS}
        for scheme in FLAGS:
            r = dict(base, state=state, sweeps_before={"warm": warmup, "burned": burn}[state], scheme=scheme, **med[scheme])
            if scheme == "nzvsspalias":
                r["phi_over_spalias_ms"] = round(med["nzvsspalias"]["phi_ms"] - med["spalias"]["phi_ms"], 5)
            emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn", type=int, default=200)
    ap.add_argument("--out", default=DEFAULT_OUT, help="the lines are appended to this file")
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
            leg(name, corpus, 100, args.steps, args.windows, args.warmup, args.burn, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, max(3, args.steps // 2), args.windows, args.warmup, args.burn, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
