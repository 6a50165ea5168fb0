#!/usr/bin/env python3
"""The topic diagnostics (ggs_topic_doc_statistics + ggs_topic_scores) on the legs DESIGN.md ("topic diagnostics") quotes,
beside the route the library offered before them: one JSON line per leg.
  device   h.topic_diagnostics(20): timed by the host clock around the call -- top words, document statistics, scores, each
           ending in its device-to-host copy and a stream synchronise: the time a driver waits; median / min / max of --windows
  host     h.get_z() (N ints) + h.get_type_topic_counts() (V x K ints) + the vectorised numpy restatement
           (tests/topic_diagnostics_restatement.py); median of --host-windows
  config2  bench.py's default corpus and seed (D = 100 000, V = 50 000, mean length 200), K = 100
  k1024    the same corpus at K = 1024
Both under scheme ggs after --burn sweeps, n = 20.  equal_to_host_route: integers equal, doubles bit for bit (NaN as NaN).
device_phases_ms: the device time of one call by phase, from events between the launches
(ggs_debug_topic_diagnostics_phases), median of 5: membership (host CSR and its upload), document pass, column statistics
(with the c log c addends), the clogc chain, n_k and wtc, compaction + sort + sorted chains, small scores.
usage: python scripts/time_topic_diagnostics.py [--legs config2,k1024] [--windows R] [--host-windows H] [--burn B] [--docs D] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import synthetic_lda_corpus  # noqa: E402
from tests import topic_diagnostics_restatement as R  # noqa: E402

SEED, ALPHA, BETA, N_WORDS = 2019, 0.1, 0.01, 20


def spread(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def leg(name, corpus, K, windows, host_windows, burn, emit):
    h = native.GGSHandle(K, corpus.num_types, ALPHA, BETA, SEED)
    h.set_corpus(corpus.doc_ptr, corpus.tokens)
    h.init_z_java_lcg(SEED)
    h.init_phi()
    h.sweep(burn)

    def host():
        return R.diagnostics(corpus.doc_ptr, corpus.tokens, h.get_z(), h.get_type_topic_counts(), ALPHA, BETA, N_WORDS)

    d = h.topic_diagnostics(N_WORDS)                                  # also: the code objects are loaded, the scratch is sized
    host_ms = []
    want = None
    for _ in range(host_windows):
        t0 = time.perf_counter()
        want = host()
        host_ms.append((time.perf_counter() - t0) * 1e3)
    same = bool((d.idx == want["idx"]).all() and (d.codoc == want["codoc"]).all() and (d.doc_stats == want["doc_stats"]).all() and
                R.same_doubles(d.clogc, want["clogc"]) and
                all(R.same_doubles(d.scores[x], want["topic_scores"][i]) for i, x in enumerate(R.SCORE_ROWS)) and
                all(R.same_doubles(d.word_scores[x], want["word_scores"][i]) for i, x in enumerate(R.WORD_ROWS)))
    dev_ms = []
    for _ in range(windows):
        h.synchronize()
        t0 = time.perf_counter()
        h.topic_diagnostics(N_WORDS)
        dev_ms.append((time.perf_counter() - t0) * 1e3)
    phases = [h.topic_diagnostics_phases(N_WORDS) for _ in range(5)]
    med = {p: round(sorted(x[p] for x in phases)[2], 4) for p in phases[0]}
    emit(dict(leg=name, scheme="ggs", K=K, types=corpus.num_types, docs=corpus.num_docs, tokens=corpus.num_tokens, n_words=N_WORDS, sweeps_before=burn,
              windows=windows, host_windows=host_windows, equal_to_host_route=same, device_ms_per_call=spread(dev_ms), host_ms_per_call=spread(host_ms),
              device_phases_ms=med, largest_phase=max(med, key=med.get)))
    h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="config2,k1024")
    ap.add_argument("--windows", type=int, default=15, help="timed device calls")
    ap.add_argument("--host-windows", type=int, default=3, help="timed runs of the host route")
    ap.add_argument("--burn", type=int, default=10, help="sweeps before the calls are timed")
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
