"""What the scheme table (csrc/ggs_host_state.hpp, kSchemes) must leave as it was: how ggs_create classes every combination of the
scheme flags, and what every scheme's handle answers to the getters that only some schemes have.  The two functions here
observe a library; the goldens beside them (tests/golden/scheme_flag_codes.json, scheme_capabilities.json) were recorded
with them from the library of the commit before the table."""
import ctypes as C
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCHEME_BITS = tuple(1 << b for b in range(2, 11))           # GGS_FLAG_PCGS ... GGS_FLAG_ADLDA
TOPICS = (5, 4097)                                           # 4097: one more than the wave-per-document kernels take
THRESHOLDS = (0, -1, 513)                                    # alias_poisson_threshold: the default, below and above 1 .. 512


def golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def flag_classes(native):
    """{"K/threshold": [class of flags = sum of SCHEME_BITS[i] for the set bits i of the index, 512 of them]}: BAD_ARG,
    UNSUPPORTED or accepted (GGS_OK, or GGS_ERR_HIP where no device is: ggs_create answers the argument check before it asks
    for one).  The golden was recorded without a device, so its UNSUPPORTED rows are the argument check's own."""
    out = {}
    for K in TOPICS:
        for L in THRESHOLDS:
            row = []
            for i in range(1 << len(SCHEME_BITS)):
                flags = sum(b for j, b in enumerate(SCHEME_BITS) if i >> j & 1)
                try:
                    native.GGSHandle(K, 10, 0.1, 0.01, 1, flags=flags, alias_poisson_threshold=L).close()
                    code = native.OK
                except native.GGSError as e:
                    code = e.code
                row.append({native.ERR_BAD_ARG: "BAD_ARG", native.ERR_UNSUPPORTED: "UNSUPPORTED", native.OK: "accepted",
                            native.ERR_HIP: "accepted"}.get(code, "code %d" % code))
            out["%d/%d" % (K, L)] = row
    return out


def same_class(K, recorded, seen):
    """K = 5: the class itself.  K = 4097: an accepted combination is anything but BAD_ARG (with a device the planner may refuse
    what the argument check let through); the other two classes are themselves."""
    if K == 5 or recorded != "accepted":
        return recorded == seen
    return seen != "BAD_ARG"


def capabilities(native):
    """{scheme: {call: return code, "z_kernel": number}} after set_corpus, init_z, init_phi and one sweep at K = 3, V = 4 over
    three documents: one empty, one of one token, one of five.  Every call is an ordinary call that answers a code."""
    K, V = 3, 4
    doc_ptr, tokens = np.array([0, 0, 1, 6], np.int64), np.array([2, 0, 1, 3, 1, 0], np.int32)
    out = {}
    for scheme, flags in (("ggs", 0), ("pcgs", native.FLAG_PCGS), ("collapsed", native.FLAG_COLLAPSED), ("polyaurn", native.FLAG_POLYAURN),
                          ("spalias", native.FLAG_SPALIAS), ("lightpclda", native.FLAG_LIGHTPCLDA), ("polyaurn_sparse", native.FLAG_POLYAURN_SPARSE),
                          ("lightcollapsed", native.FLAG_LIGHTCOLLAPSED), ("nzvsspalias", native.FLAG_NZVSSPALIAS), ("adlda", native.FLAG_ADLDA)):
        h = native.GGSHandle(K, V, 0.1, 0.01, 7, flags=flags)
        try:
            h.set_corpus(doc_ptr, tokens)
            h.init_z_java_lcg(7)
            h.init_phi()
            h.sweep(1)
            L, p = h._L, h._h
            ps, a, tn = np.empty((V, K)), np.empty((V, K), np.int32), np.empty(V)
            nw, lists = np.empty(V, np.int32), np.empty((V, K), np.int32)
            i3, i4, phi, theta = np.zeros(3, np.int64), np.zeros(4, np.int64), np.empty((K, V)), np.empty((3, K))
            none = np.empty(0, np.int32)
            zk = C.c_int32(-1)
            row = {
                "ggs_get_alias_tables": L.ggs_get_alias_tables(p, native._dp(ps), native._ip(a), native._dp(tn)),
                "ggs_get_mh_stats": L.ggs_get_mh_stats(p, native._lp(i3)),
                "ggs_get_word_topic_lists": L.ggs_get_word_topic_lists(p, native._ip(nw), native._ip(lists)),
                "ggs_get_sparse_stats": L.ggs_get_sparse_stats(p, native._lp(i4)),
                "ggs_get_vs_stats": L.ggs_get_vs_stats(p, native._lp(i3)),
                "ggs_set_topic_priors": L.ggs_set_topic_priors(p, 0, native._ip(none), native._ip(none)),
                "ggs_get_phi": L.ggs_get_phi(p, native._dp(phi)),
                "ggs_get_theta": L.ggs_get_theta(p, 0, 3, native._dp(theta)),
            }
            assert L.ggs_get_z_form(p, C.byref(zk), None, None) == native.OK
            row["z_kernel"] = zk.value
            out[scheme] = row
        finally:
            h.close()
    return out
