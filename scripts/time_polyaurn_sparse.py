#!/usr/bin/env python3
"""scheme=polyaurn_sparse against scheme=polyaurn and scheme=spalias, in one process, on the legs DESIGN.md ("6e. Scheme
polyaurn_sparse") quotes: one JSON line per (leg, state, scheme) with ms_per_sweep, the per-sweep phases of
ggs_get_timings and the kernel that ran; the polyaurn_sparse lines also carry the share of tokens per list kind and the
mean number of candidates n (ggs_get_sparse_stats over the timed sweeps), beside the mean number of non-zero topics per
document (nnz_d) of the state timed.  One handle at a time.  Legs as scripts/time_spalias.py:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
States: "warm" = after the warm-up sweeps from the random start; "burned" = after --burn polyaurn_sparse sweeps (Phi's
sparsity grows with burn-in).  polyaurn and spalias are timed from the SAME z (ggs_set_z, Phi redrawn).  The table and
list build has no phase of its own in ggs_get_timings (it is counted in phi_ms): build_ms is the polyaurn_sparse leg's
phi_ms less the polyaurn leg's of the same state, the two Phi phases being otherwise the same kernels on the same counts.
usage: python scripts/time_polyaurn_sparse.py [--legs config2,k1024] [--steps N] [--warmup W] [--burn B] [--out FILE]"""
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
FLAGS = {s: native.SCHEME_FLAGS[s] for s in ("polyaurn_sparse", "polyaurn", "spalias")}
DEFAULT_OUT = os.path.join(ROOT, "profiles", "polyaurn_sparse_bench.jsonl")


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
    return dict(ms_per_sweep=round(dt * 1e3, 4), phase_ms={k: round(tm[k] / steps, 4) for k in ("theta_ms", "z_ms", "merge_ms", "phi_ms", "exchange_ms")},
                z_kernel=h.launch_info()["z_kernel"])


def handle(scheme, corpus, K):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    return h


def timed_sparse(h, steps):
    before = h.sparse_stats()
    row = timed(h, steps)
    d = (h.sparse_stats() - before).astype(np.float64)
    tokens = max(1.0, float(d[:3].sum()))
    row.update(share_word_list=round(d[0] / tokens, 4), share_doc_list=round(d[1] / tokens, 4), share_uniform=round(d[2] / tokens, 6),
               mean_n=round(d[3] / tokens, 2), mean_nw=round(float(h.word_topic_lists()[0].mean()), 2))
    return row


def leg(name, corpus, K, steps, warmup, burn, emit):
    base = {"leg": name, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens, "steps": steps}
    states, rows = {}, {}
    h = handle("polyaurn_sparse", corpus, K)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    states["warm"] = h.get_z()
    rows[("warm", "polyaurn_sparse")] = timed_sparse(h, steps)
    h.set_z(states["warm"], redraw_phi=True)
    h.sweep(burn)
    states["burned"] = h.get_z()
    rows[("burned", "polyaurn_sparse")] = timed_sparse(h, steps)
    h.close()
    for scheme in ("polyaurn", "spalias"):
        for state in ("warm", "burned"):
            h = handle(scheme, corpus, K)
            h.set_z(states[state], redraw_phi=True)
            rows[(state, scheme)] = timed(h, steps)
            h.close()
    for state in ("warm", "burned"):
        nnz = round(mean_nnz(corpus, states[state], K), 2)
        build = round(rows[(state, "polyaurn_sparse")]["phase_ms"]["phi_ms"] - rows[(state, "polyaurn")]["phase_ms"]["phi_ms"], 4)
        for scheme in FLAGS:
            r = dict(base, state=state, sweeps_before={"warm": warmup, "burned": burn}[state], scheme=scheme, mean_nnz_d=nnz, **rows[(state, scheme)])
            if scheme == "polyaurn_sparse":
                r["build_ms"] = build
            emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--steps", type=int, default=10)
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
            leg(name, corpus, 100, args.steps, args.warmup, args.burn, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, max(3, args.steps // 2), args.warmup, args.burn, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
