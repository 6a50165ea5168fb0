#!/usr/bin/env python3
"""The Phi phase of scheme=spalias with and without topic priors, on the legs DESIGN.md ("6f. Scheme spalias_priors") quotes:
one JSON line per (leg, variant) with phi_ms per sweep (ggs_get_timings: the Phi draw and the alias table build), the other
phases and ms_per_sweep.  Legs as scripts/time_spalias.py:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
Variants: "plain" = a spalias handle without ggs_set_topic_priors; "priors" = the --anchors most frequent words anchored to one
topic each (word i to topic i mod K).  Both start from the same seeded z and are timed after --warmup sweeps.
To compare the plain variant between two builds of the library, run this script once per build with GGS_HIP_LIB pointing at
the other libggs_hip.so, alternating, with --variants plain and --tag naming the build.  --corpus-cache FILE keeps the
generated corpus between such runs.
usage: python scripts/time_spalias_priors.py [--legs config2,k1024] [--variants plain,priors] [--steps N] [--warmup W]
                                             [--anchors A] [--repeat R] [--tag T] [--corpus-cache FILE] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import Corpus, synthetic_lda_corpus  # noqa: E402

SEED, ALPHA, BETA = 2019, 0.1, 0.01


def timed(h, steps):
    h.synchronize()
    h.reset_timings()
    t0 = time.perf_counter()
    h.sweep(steps)
    h.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tm = h.get_timings()
    return round(dt * 1e3, 4), {k: round(tm[k] / steps, 4) for k in ("theta_ms", "z_ms", "merge_ms", "phi_ms")}


def anchor_cells(corpus, K, anchors):
    words = np.argsort(-np.bincount(corpus.tokens, minlength=corpus.num_types), kind="stable")[:anchors]
    topics, cells_w = [], []
    for i, w in enumerate(words):
        others = np.delete(np.arange(K, dtype=np.int32), i % K)
        topics.append(others)
        cells_w.append(np.full(others.size, w, np.int32))
    return np.concatenate(topics), np.concatenate(cells_w)


def load_corpus(cache):
    if cache and os.path.exists(cache):
        d = np.load(cache)
        return Corpus(d["doc_ptr"], d["tokens"], int(d["num_types"]))
    c = synthetic_lda_corpus(100000, 50000, 200, true_topics=100, seed=SEED)
    if cache:
        np.savez(cache, doc_ptr=c.doc_ptr, tokens=c.tokens, num_types=c.num_types)
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--variants", default="plain,priors")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--anchors", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=3, help="timed windows per handle")
    ap.add_argument("--tag", default="")
    ap.add_argument("--corpus-cache", default=None)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None
    corpus = load_corpus(args.corpus_cache)
    for leg in args.legs.split(","):
        K = {"config2": 100, "k1024": 1024}[leg]
        steps = args.steps if K == 100 else max(3, args.steps // 4)
        for variant in args.variants.split(","):
            h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=native.FLAG_SPALIAS)
            h.set_corpus(corpus.doc_ptr, corpus.tokens)
            cells = 0
            if variant == "priors":
                t, w = anchor_cells(corpus, K, args.anchors)
                h.set_topic_priors(t, w)
                cells = int(t.size)
            h.init_z_java_lcg(SEED)
            h.init_phi()
            h.sweep(args.warmup)
            for r in range(args.repeat):
                ms, ph = timed(h, steps)
                line = json.dumps(dict(leg=leg, K=K, variant=variant, tag=args.tag, window=r, steps=steps, zero_cells=cells, ms_per_sweep=ms, phase_ms=ph))
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
            h.close()


if __name__ == "__main__":
    main()
