"""The gamma draws in shape-class order, what needs no GPU: the cell list and the table must not cost the two kernels their
waves per SIMD (the draws are VALU-bound and hide their latencies behind each other's waves) nor send a register to
scratch -- read from the summary the build writes."""
import os


def test_the_gamma_kernels_keep_their_occupancy_and_use_no_scratch():
    from ldagroupedgibbssampler_amd import _lib
    path = os.path.join(_lib.CSRC, "ggs_resource_summary.txt")
    assert os.path.exists(path), "the build writes %s beside the library" % path
    rows = {}
    for line in open(path):
        if line.startswith("#") or not line.strip():
            continue
        f = line.split()
        rows[" ".join(f[:-6])] = [int(x) for x in f[-6:]]       # VGPRs, AGPRs, SGPRs, scratch, waves per SIMD, static LDS
    for name, waves in (("ggs::theta_kernel<256>", 7), ("ggs::phi_gamma_kernel<false>", 5), ("ggs::phi_gamma_kernel<true>", 5),
                        ("ggs::phi_gamma_vs_kernel", 5)):
        assert name in rows, "kernel %s is not in the build" % name
        assert rows[name][3] == 0, "%s spills %d bytes per lane" % (name, rows[name][3])
        assert rows[name][4] >= waves, "%s: %d waves per SIMD by registers, %d before the cell list" % (name, rows[name][4], waves)
