#!/usr/bin/env python3
"""ggs_min_doc_distances and ggs_min_topic_distance on the legs DESIGN.md ("distances of the diagnostics loop") quotes: one
JSON line per (leg, entry) with ms_per_call as median / min / max over --windows timed windows of --calls calls that
ALTERNATE between the two entries, so that a drift of the clocks hits both.  A call is timed by the host clock around the
entry, which ends in the device-to-host copy of its result and a stream synchronise: the time a driver waits.
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
Both under scheme ggs, after --burn sweeps from the seeded start (theta is then the last z step's; Phi the last draw).
Beside each time, what the hardware could do: pair_steps = the subtract-square-add steps the loops need (D (D - 1) / 2 * K for
the documents, each unordered pair once; K (K - 1) / 2 * V for the topics); fp64_per_pair_step = 3, read from the kernels'
ISA (v_add_f64 for the difference, v_mul_f64, v_add_f64; no v_fma_f64); issue_bound_ms = pair_steps * 3 wave-lanes over
CUs * 64 lanes per clock at 2.4 GHz -- one wave64 fp64 instruction per 4 cycles per SIMD, the rate the 78.6 TFLOP/s fp64 vector
peak implies for a non-fused instruction, NOT measured here -- and fraction_of_issue_bound = issue_bound_ms / median.
usage: python scripts/time_min_distances.py [--legs config2,k1024] [--calls N] [--windows R] [--burn B] [--docs D] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import synthetic_lda_corpus  # noqa: E402

SEED, ALPHA, BETA = 2019, 0.1, 0.01
CLOCK_HZ, FP64_PER_PAIR_STEP = 2.4e9, 3


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def timed(call, h, calls):
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        call()
    return (time.perf_counter() - t0) / calls * 1e3


def leg(name, corpus, K, calls, windows, burn, cus, emit):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED)
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(burn)
    entries = {"min_doc_distances": h.min_doc_distances, "min_topic_distance": h.min_topic_distance}
    D, V = corpus.num_docs, corpus.num_types
    steps = {"min_doc_distances": D * (D - 1) // 2 * K, "min_topic_distance": K * (K - 1) // 2 * V}
    for call in entries.values():                                   # first launches load the code objects and size the scratch
        call()
    ms = {e: [] for e in entries}
    for _ in range(windows):
        for e, call in entries.items():
            ms[e].append(timed(call, h, calls))
    for e in entries:
        s = spread(ms[e])
        bound = steps[e] * FP64_PER_PAIR_STEP / (cus * 64 * CLOCK_HZ) * 1e3
        emit(dict(leg=name, entry=e, scheme="ggs", K=K, docs=D, types=V, sweeps_before=burn, calls_per_window=calls, windows=windows, ms_per_call=s,
                  pair_steps=steps[e], fp64_per_pair_step=FP64_PER_PAIR_STEP, compute_units=cus, clock_ghz=CLOCK_HZ / 1e9,
                  issue_bound_ms=round(bound, 4), fraction_of_issue_bound=round(bound / s["median"], 4)))
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--calls", type=int, default=5, help="calls per timed window")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per entry, alternating between the two")
    ap.add_argument("--burn", type=int, default=20, help="sweeps before the entries are timed")
    ap.add_argument("--docs", type=int, default=100000, help="documents of the corpus (a rehearsal takes fewer)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    out = open(args.out, "a") if args.out else None

    def emit(r):
        line = json.dumps(r)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is timed without one")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    corpus = synthetic_lda_corpus(args.docs, 50000, 200, true_topics=100, seed=SEED)
    for name in args.legs.split(","):
        if name == "config2":
            leg(name, corpus, 100, args.calls, args.windows, args.burn, cus, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, args.calls, args.windows, args.burn, cus, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
