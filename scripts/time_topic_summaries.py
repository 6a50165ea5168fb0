#!/usr/bin/env python3
"""ggs_top_words on the legs DESIGN.md ("top words per topic") quotes, beside the route the library offered before it: one
JSON line per (leg, kind) with ms_per_call as median / min / max over --windows timed windows that ALTERNATE between the two
routes, so that a drift of the clocks hits both.
  device   h.top_words(kind, 20): timed by the host clock around the entry, which ends in the device-to-host copy of the
           K x 20 ids and a stream synchronise -- the time a driver waits
  host     h.get_type_topic_counts() (the V x K copy) followed by the vectorised numpy restatement of the ranking
           (tests/topic_summaries_restatement.py: cumsum chains, the oracle's fdlibm log, one lexsort per topic)
  config2  bench.py's default corpus and seed (D = 100 000, V = 50 000, mean length 200), K = 100:  V * K = 5 * 10^6 cells
  k1024    the same corpus at K = 1024:  5.1 * 10^7 cells
Both under scheme ggs after --burn sweeps.  device_phases_ms: the device time of one call by phase, from events between the
launches (ggs_debug_top_words_phases) -- mass_k, the total chain, the words' statistics, selection + merge -- and
total_chain_share = total / their sum.  plain_walk_total_ms: the total chain as ONE lane walking the V * K cells (the
element-by-element chain kernel), what the exact parallel sum of ggs_exact_sum.hpp replaces.
usage: python scripts/time_topic_summaries.py [--legs config2,k1024] [--windows R] [--burn B] [--docs D] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import synthetic_lda_corpus  # noqa: E402
from tests import topic_summaries_restatement as R  # noqa: E402

SEED, ALPHA, BETA, N_WORDS, LAMBDA = 2019, 0.1, 0.01, 20, 0.6


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def leg(name, corpus, K, windows, host_windows, burn, emit):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED)
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(burn)
    V = corpus.num_types

    def host(kind):
        return R.top_words(h.get_type_topic_counts(), BETA, kind, N_WORDS, LAMBDA)[0]

    for kind in ("top", "relevance"):
        same = bool((h.top_words(kind, N_WORDS, LAMBDA) == host(kind)).all())      # also: the code objects are loaded, the scratch is sized
        dev_ms, host_ms = [], []
        for i in range(windows):
            h.synchronize()
            t0 = time.perf_counter()
            h.top_words(kind, N_WORDS, LAMBDA)
            dev_ms.append((time.perf_counter() - t0) * 1e3)
            if i < host_windows:
                t0 = time.perf_counter()
                host(kind)
                host_ms.append((time.perf_counter() - t0) * 1e3)
        phases = [h.top_words_phases(kind, N_WORDS, LAMBDA) for _ in range(5)]
        med = {p: round(sorted(x[p] for x in phases)[2], 4) for p in phases[0]}
        rec = dict(leg=name, kind=kind, scheme="ggs", K=K, types=V, cells=V * K, n_words=N_WORDS, sweeps_before=burn, windows=windows,
                   host_windows=host_windows, equal_to_host_route=same, device_ms_per_call=spread(dev_ms), host_ms_per_call=spread(host_ms),
                   device_phases_ms=med, total_chain_share=round(med["total"] / max(sum(med.values()), 1e-9), 4))
        if kind == "relevance":
            walks = sorted(h.top_words_phases(kind, N_WORDS, LAMBDA, element_chain=True)["total"] for _ in range(3))
            rec["plain_walk_total_ms"] = round(walks[1], 4)
        emit(rec)
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--windows", type=int, default=15, help="timed device calls per kind")
    ap.add_argument("--host-windows", type=int, default=3, help="timed runs of the host route per kind (it takes seconds at K = 1024)")
    ap.add_argument("--burn", type=int, default=10, help="sweeps before the entries are timed")
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
    corpus = synthetic_lda_corpus(args.docs, 50000, 200, true_topics=100, seed=SEED)
    for name in args.legs.split(","):
        if name == "config2":
            leg(name, corpus, 100, args.windows, args.host_windows, args.burn, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, args.windows, args.host_windows, args.burn, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
