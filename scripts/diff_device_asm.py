#!/usr/bin/env python3
"""Is the device code of two builds the same?  usage: diff_device_asm.py A.s B.s

A.s, B.s: the gfx950 assembly `make -C ldagroupedgibbssampler_amd/csrc asm` writes (ggs_gfx950.s).  A host-only change
reorders template instantiations, the compiler numbers local labels by function ordinal (.LBB237_4, .Lfunc_end237) and
the padding in front of its comments moves with that number's width, so the files differ bytewise although no
instruction does.  The comparison is therefore per function: the span from `; -- Begin function NAME` to
`; -- End function` (instructions and the .amdhsa_kernel descriptor: registers, LDS, scratch), ordinals stripped from
the labels, comments and runs of blanks dropped.  Both files must hold the same names and, name by name, the same text.
Prints the counts and the names that differ; exit status 0 if none does, 1 otherwise."""
import hashlib
import re
import sys


def functions(path):
    out, name, buf = {}, None, []
    with open(path) as f:
        for ln in f:
            m = re.search(r"; -- Begin function (\S+)", ln)
            if m:
                name, buf = m.group(1), []
            if name is None:
                continue
            t = re.sub(r"(\.?L?BB)\d+_", r"\1_", re.sub(r"\.Lfunc_end\d+", ".Lfunc_end", ln))
            buf.append(" ".join(t.split(";")[0].split()) + "\n")
            if "; -- End function" in ln:
                out[name] = hashlib.sha256("".join(buf).encode()).hexdigest()
                name = None
    return out


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    a, b = functions(argv[1]), functions(argv[2])
    bad = sorted(set(a) ^ set(b)) + sorted(k for k in a if k in b and a[k] != b[k])
    print("%d functions, %d functions, %d differ" % (len(a), len(b), len(bad)))
    for name in bad:
        print(name)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
