#!/usr/bin/env python3
"""Which kernels a handle launches, with how much LDS, for every kernel family: one line per (K, scheme) with what
ggs_get_z_form, ggs_get_launch_info, ggs_get_z_parts, ggs_get_warm_tiers and ggs_get_num_hot_words answer after one
seeded corpus is set (or the error code where the combination is unsupported).  A row describes the z step the handle
launches: for the pcgs family lds_bytes_z is the dynamic LDS of the lane-per-document, wave-per-document, spalias,
lightpclda or polyaurn_sparse kernel and num_chunks the entries of the document order it strides (groups of 64 for the lane-per-document
kernel).  Two builds of the library that make the same launches print the same text: run it before and after a change of the host code (GGS_HIP_LIB selects the library)
and compare.  usage: python scripts/dump_launch_plans.py [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ldagroupedgibbssampler_amd import native  # noqa: E402
from ldagroupedgibbssampler_amd.corpus import zipf_unigram_corpus  # noqa: E402

TOPICS = (8, 20, 100, 160, 161, 176, 192, 200, 256, 512, 1024, 2048, 4096)
SCHEMES = native.SCHEME_FLAGS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    # more documents than twice the vocabulary (the z step of the streaming kernel goes in parts), enough tokens per
    # frequent word for warm tiers
    corpus = zipf_unigram_corpus(20000, 5000, 100, seed=2019)
    lines = []
    for K in TOPICS:
        for scheme, flags in SCHEMES.items():
            row = {"K": K, "scheme": scheme}
            try:
                h = native.GGSHandle(K, corpus.num_types, 0.1, 0.01, 2019, flags=flags)
                try:
                    row["before_corpus"] = h.launch_info()
                    h.set_corpus(corpus.doc_ptr, corpus.tokens)
                    row["with_corpus"] = h.launch_info()
                finally:
                    h.close()
            except native.GGSError as e:
                row["error"] = e.code
            lines.append(json.dumps(row, sort_keys=True))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
