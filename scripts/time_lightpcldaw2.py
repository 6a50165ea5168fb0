#!/usr/bin/env python3
"""scheme=lightpcldaw2 against scheme=lightpclda, scheme=lightcollapsed and scheme=pcgs, in one process, on the legs DESIGN.md
("6m. Scheme lightpcldaw2") quotes, in the manner of scripts/time_lightcollapsed.py: one JSON line per (leg, state, scheme)
with ms_per_sweep and the per-sweep phases of ggs_get_timings, each as median / min / max over --windows timed windows of
--steps sweeps that ALTERNATE between the four schemes' handles, so that a drift of the clocks hits all of them; the kernel
that ran; for the three Metropolis-Hastings schemes the three rates of the sweeps timed; for the two schemes that build their
tables over the counts the build call apart from the z step; and one line per (leg, state) with the spread of the per-window
ratios of the pcgs and the lightpclda sweep to the lightpcldaw2 sweep.  Legs:
  config2          bench.py's default corpus and seed (D=100 000, V=50 000, mean length 200), K = 100
  k1024            the same corpus at K = 1024
States: "warm" = after the warm-up sweeps from the random start; "burned" = after --burn further sweeps -- both of the pcgs
chain, so the four schemes are timed from the SAME z (ggs_set_z) and see the same sparsity of the counts.
The table build (count_alias_build_kernel) runs at the head of the z step and is counted in z_ms; it is timed on its own as
the host wall clock of ggs_get_word_topic_lists(h, nw, NULL): that call launches the build, copies V integers back and
synchronises, so build_call_ms is an UPPER bound of the kernel's time by a launch, a 200 KB copy and a synchronisation, and
z_step_ms = z_ms - build_call_ms a lower bound of the z kernel's.
usage: python scripts/time_lightpcldaw2.py [--legs config2,k1024] [--steps N] [--windows R] [--warmup W] [--burn B] [--out FILE]"""
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
FLAGS = {"lightpcldaw2": native.FLAG_LIGHTPCLDAW2, "lightpclda": native.FLAG_LIGHTPCLDA, "lightcollapsed": native.FLAG_LIGHTCOLLAPSED, "pcgs": native.FLAG_PCGS}
SCHEMES = tuple(FLAGS)
MH = ("lightpcldaw2", "lightpclda", "lightcollapsed")
COUNT_TABLES = ("lightpcldaw2", "lightcollapsed")


def timed(h, steps):
    h.synchronize()
    h.reset_timings()
    t0 = time.perf_counter()
    h.sweep(steps)
    h.synchronize()
    dt = (time.perf_counter() - t0) / steps
    tm = h.get_timings()
    return round(dt * 1e3, 4), {k: round(tm[k] / steps, 4) for k in ("theta_ms", "z_ms", "merge_ms", "phi_ms", "exchange_ms")}


def build_ms(h, steps):
    """the table build alone: the lists' lengths are all that is copied back"""
    nw = np.empty(h.V, np.int32)
    ptr = nw.ctypes.data_as(C.POINTER(C.c_int32))
    h._chk(h._L.ggs_get_word_topic_lists(h._h, ptr, None))          # untimed: code upload
    h.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        h._chk(h._L.ggs_get_word_topic_lists(h._h, ptr, None))
    return round((time.perf_counter() - t0) / steps * 1e3, 4), float(nw[nw > 0].mean()) if (nw > 0).any() else 0.0


def handle(scheme, corpus, K):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED, flags=FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    return h


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def leg(name, corpus, K, steps, warmup, burn, windows, emit):
    base = {"leg": name, "K": K, "docs": corpus.num_docs, "types": corpus.num_types, "tokens": corpus.num_tokens, "steps_per_window": steps,
            "windows": windows}
    states = {}
    h = handle("pcgs", corpus, K)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    states["warm"] = h.get_z()
    h.sweep(burn)
    states["burned"] = h.get_z()
    h.close()
    for state in ("warm", "burned"):
        hs, rows = {}, {s: dict(ms=[], z=[], merge=[], phi=[], build=[]) for s in SCHEMES}
        for scheme in SCHEMES:                                      # all handles live, the windows alternate between them
            hs[scheme] = handle(scheme, corpus, K)
            hs[scheme].set_z(states[state], redraw_phi=True)
            hs[scheme].sweep(1)                                     # the first z step of a corpus is not the steady one
        before = {s: hs[s].mh_stats() for s in MH}
        nnz = {}
        for _ in range(windows):
            for scheme in SCHEMES:
                ms, ph = timed(hs[scheme], steps)
                r = rows[scheme]
                r["ms"].append(ms); r["z"].append(ph["z_ms"]); r["merge"].append(ph["merge_ms"]); r["phi"].append(ph["phi_ms"])
                if scheme in COUNT_TABLES:
                    b, nnz[scheme] = build_ms(hs[scheme], steps)
                    r["build"].append(b)
        for scheme in SCHEMES:
            r = rows[scheme]
            out = dict(base, state=state, sweeps_before={"warm": warmup, "burned": warmup + burn}[state], scheme=scheme, ms_per_sweep=spread(r["ms"]),
                       z_ms=spread(r["z"]), merge_ms=spread(r["merge"]), phi_ms=spread(r["phi"]), z_kernel=hs[scheme].launch_info()["z_kernel"])
            if scheme in MH:
                d = (hs[scheme].mh_stats() - before[scheme]).astype(np.float64) / (windows * steps * corpus.num_tokens)
                out["mh_rates"] = dict(word_kept=round(float(d[0]), 4), doc_accepted=round(float(d[1]), 4), left_on_old=round(float(d[2]), 4))
            if scheme in COUNT_TABLES:
                out["build_call_ms"] = spread(r["build"])
                out["z_step_ms"] = spread([z - b for z, b in zip(r["z"], r["build"])])
                out["mean_nnz_w"] = round(nnz[scheme], 2)
            emit(out)
        w2 = rows["lightpcldaw2"]["ms"]
        emit(dict(base, state=state, ratio_pcgs_over_lightpcldaw2=spread([p / w for p, w in zip(rows["pcgs"]["ms"], w2)]),
                  ratio_lightpclda_over_lightpcldaw2=spread([p / w for p, w in zip(rows["lightpclda"]["ms"], w2)]),
                  ratio_lightcollapsed_over_lightpcldaw2=spread([p / w for p, w in zip(rows["lightcollapsed"]["ms"], w2)])))
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
