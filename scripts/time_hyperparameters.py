#!/usr/bin/env python3
"""The hyperparameter step (DESIGN.md "6n") on the benchmark corpus, in one process: one JSON line per (leg, what) with the
median / min / max in ms over --windows timed windows that ALTERNATE between everything timed, so that a drift of the clocks hits
all of it alike (as scripts/time_adlda.py does):
  doc_hist_sym / doc_hist_asym   ggs_doc_topic_histogram (kernel, copy-back of the bins, bin 0 on the host), with docLengthCounts
  cell_hist                      ggs_type_topic_count_histogram
  learn_alpha_sym / learn_alpha_asym / learn_beta   the estimators on the host (ggs_learn_*), from those histograms
  setter                         ggs_set_hyperparameters (the values it already has: the state is not moved)
  host_doc / host_cell           the route they replace: get_doc_topic_counts / get_type_topic_counts and numpy bincount
  sweep                          one sweep of the same handle, for scale
and one line per leg with the byte floors (N * 4 B of z, V * K * 4 B of counts) beside the histogram calls' medians.
Legs: config2 = bench.py's default corpus (D = 100 000, V = 50 000, mean length 200, 20 M tokens) at K = 100; k1024 = the same at K = 1024.
usage: python scripts/time_hyperparameters.py [--legs config2,k1024] [--windows R] [--warmup W] [--scheme ggs] [--out FILE]"""
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


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def ms_of(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def leg(name, corpus, K, scheme, warmup, windows, emit):
    V, D = corpus.num_types, corpus.num_docs
    h = native.GGSHandle(K, V, ALPHA, BETA, SEED, flags=native.SCHEME_FLAGS[scheme])
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(warmup)
    lens = np.diff(corpus.doc_ptr)
    n_bins = int(lens.max()) + 1
    max_type = int(np.bincount(corpus.tokens, minlength=V).max())
    alpha, beta, beta_sum = h.hyperparameters()

    def host_doc():
        n_dk = h.get_doc_topic_counts()
        return np.stack([np.bincount(n_dk[:, k], minlength=n_bins) for k in range(K)])

    def host_cell():
        return np.bincount(h.get_type_topic_counts().ravel(), minlength=max_type + 1)

    def sweep():
        h.sweep(1)
        h.synchronize()

    sym, lengths = h.doc_topic_histogram(True, n_bins)
    asym, _ = h.doc_topic_histogram(False, n_bins)
    cell = h.type_topic_count_histogram(max_type + 1)
    assert np.array_equal(asym, host_doc()) and np.array_equal(cell, host_cell()) and np.array_equal(sym[0, 1:], asym[:, 1:].sum(0))
    n_k = h.get_topic_totals()
    sizes = np.bincount(n_k, minlength=int(n_k.max()) + 1).astype(np.int32)
    what = {
        "doc_hist_sym": lambda: h.doc_topic_histogram(True, n_bins),
        "doc_hist_asym": lambda: h.doc_topic_histogram(False, n_bins),
        "cell_hist": lambda: h.type_topic_count_histogram(max_type + 1),
        "learn_alpha_sym": lambda: native.learn_symmetric_concentration(sym[0], lengths, K, float(alpha.sum())),
        "learn_alpha_asym": lambda: native.learn_parameters(alpha.copy(), asym, lengths, 1.001, 1.0, 1),
        "learn_beta": lambda: native.learn_symmetric_concentration(cell, sizes, V, beta_sum),
        "setter": lambda: h.set_hyperparameters(alpha, beta, beta_sum),
        "host_doc": host_doc,
        "host_cell": host_cell,
        "sweep": sweep,
    }
    rows = {k: [] for k in what}
    for _ in range(windows):
        for k, fn in what.items():
            h.synchronize()
            rows[k].append(ms_of(fn)[0])
    base = {"leg": name, "scheme": scheme, "K": K, "docs": D, "types": V, "tokens": corpus.num_tokens, "windows": windows, "n_bins_doc": n_bins, "n_bins_cell": max_type + 1}
    for k in what:
        emit(dict(base, what=k, ms=spread(rows[k])))
    z_bytes, cell_bytes = corpus.num_tokens * 4, V * K * 4
    emit(dict(base, what="floors", z_bytes=z_bytes, cell_bytes=cell_bytes,
              doc_hist_sym_GBps=round(z_bytes / spread(rows["doc_hist_sym"])["median"] / 1e6, 1),
              cell_hist_GBps=round(cell_bytes / spread(rows["cell_hist"])["median"] / 1e6, 1),
              step_over_sweep=round((spread(rows["doc_hist_asym"])["median"] + spread(rows["cell_hist"])["median"] + spread(rows["learn_alpha_asym"])["median"] +
                                     spread(rows["learn_beta"])["median"] + spread(rows["setter"])["median"]) / spread(rows["sweep"])["median"], 3),
              host_route_over_device=round((spread(rows["host_doc"])["median"] + spread(rows["host_cell"])["median"]) /
                                           (spread(rows["doc_hist_asym"])["median"] + spread(rows["cell_hist"])["median"]), 1)))
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--windows", type=int, default=7, help="timed windows, alternating between everything timed")
    ap.add_argument("--warmup", type=int, default=5, help="sweeps from the random start before anything is timed")
    ap.add_argument("--scheme", default="ggs", choices=list(native.SCHEME_FLAGS))
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
            leg(name, corpus, 100, args.scheme, args.warmup, args.windows, emit)
        elif name == "k1024":
            leg(name, corpus, 1024, args.scheme, args.warmup, args.windows, emit)
        else:
            raise SystemExit("unknown leg %r" % name)


if __name__ == "__main__":
    main()
