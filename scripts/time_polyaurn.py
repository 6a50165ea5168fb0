#!/usr/bin/env python3
"""scheme=polyaurn against scheme=pcgs, in one process, on the legs DESIGN.md ("Scheme polyaurn") quotes: one JSON line per
(leg, scheme) with ms_per_sweep and the per-sweep phases of ggs_get_timings.  Each handle is destroyed before the next is
built.  Legs:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
  config4_standin  bench.py's config-4 stand-in (D=18 846, V=60 000, mean length 150), K = 200
  rank3_of_8       one rank of 8 of config2 through ggs_attach_null_exchange, as bench.py --simulate-world 8 runs it
usage: python scripts/time_polyaurn.py [--legs config2,k1024,...] [--steps N] [--warmup W] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import even_split, synthetic_lda_corpus  # noqa: E402

SEED, ALPHA, BETA = 2019, 0.1, 0.01


def run(leg, scheme, corpus, K, steps, warmup, world=1, rank=0, tok_base=0, doc_base=0, total_tokens=None):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=native.SCHEME_FLAGS[scheme])
    if world > 1:
        h.attach_null_exchange(rank, world)
    h.set_corpus(corpus.doc_ptr, corpus.tokens, doc_base, tok_base)
    if world > 1:
        h.set_global_token_count(total_tokens)
        from ldagroupedgibbssampler_amd.sharded import java_lcg_initial_z_slice
        h.set_z(java_lcg_initial_z_slice(tok_base, corpus.num_tokens, K, SEED), redraw_phi=True)
    else:
        h.init_z_java_lcg(SEED)
        h.init_phi()
    h.sweep(warmup)
    h.synchronize()
    h.reset_timings()
    t0 = time.perf_counter()
    h.sweep(steps)
    h.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tm = h.get_timings()
    info = h.launch_info()
    h.close()
    return {"leg": leg, "scheme": scheme, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens,
            "world": world, "rank": rank, "steps": steps, "warmup": warmup, "ms_per_sweep": round(dt * 1e3, 4),
            "phase_ms": {k: round(tm[k] / steps, 4) for k in ("theta_ms", "z_ms", "merge_ms", "phi_ms", "exchange_ms")},
            "z_kernel": info["z_kernel"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024,config4_standin,rank3_of_8")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    legs = args.legs.split(",")
    out = open(args.out, "a") if args.out else None
    corpus2 = None
    for leg in legs:
        if leg in ("config2", "k1024", "rank3_of_8") and corpus2 is None:
            corpus2 = synthetic_lda_corpus(100000, 50000, 200, true_topics=100, seed=SEED)
        for scheme in ("polyaurn", "pcgs"):
            if leg == "config2":
                r = run(leg, scheme, corpus2, 100, args.steps, args.warmup)
            elif leg == "k1024":
                r = run(leg, scheme, corpus2, 1024, max(3, args.steps // 4), 1)
            elif leg == "config4_standin":
                c4 = synthetic_lda_corpus(18846, 60000, 150, true_topics=100, seed=SEED)
                r = run(leg, scheme, c4, 200, args.steps, args.warmup)
            elif leg == "rank3_of_8":
                b = even_split(corpus2.num_docs, 8)
                sub, doc_base, tok_base = corpus2.shard(b[3], b[4])
                r = run(leg, scheme, sub, 100, args.steps, args.warmup, world=8, rank=3, tok_base=tok_base, doc_base=doc_base,
                        total_tokens=corpus2.num_tokens)
            else:
                raise SystemExit("unknown leg %r" % leg)
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
