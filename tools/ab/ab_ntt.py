#!/usr/bin/env python3
"""A/B of the NTT kernels between library variants (tools/ab/build_variants.sh with UNIT=ntt): per-kernel time of the inverse and the
expanding forward transform at the sizes a 2^20-row segment uses and at 2^13 .. 2^15 (FRI rounds, small circuits), and a digest of the outputs so that two variants can be compared
word for word (the default build is the one the parity tests cover).  usage: [R0HIP_AB_LIB=tools/ab/lib/libr0hip_X.so] ab_ntt.py [cols]"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

import hyperfridge_r0_amd as r0

if os.environ.get("R0HIP_AB_LIB"):
    r0.LIB_PATH = os.path.abspath(os.environ["R0HIP_AB_LIB"])


def main():
    cols = int(sys.argv[1]) if len(sys.argv) > 1 else 184
    hal = r0.Hal(0)
    rng = np.random.default_rng(0)
    digest = hashlib.sha256()
    # every kernel shape: the small kernel, one pass, the pass over the top four bits, two passes, the wide tiles
    for po2, width in ((5, 3), (8, 3), (13, 5), (14, 3), (15, 3), (16, 3), (18, 3), (20, 2)):
        n = 1 << po2
        src = hal.copy_from(rng.integers(0, r0.P, width * n, dtype=np.uint32))
        ev = hal.alloc(width * 4 * n)
        hal.batch_interpolate_ntt(src, width, po2)
        hal.batch_expand_into_evaluate_ntt(ev, src, width, po2, 2)
        digest.update(src.to_host().tobytes())
        digest.update(ev.to_host().tobytes())
        src.free(); ev.free()

    def timed(label, fn):
        fn()
        hal.sync()
        hal.kernel_timing(True)
        for _ in range(5):
            fn()
        st = hal.kernel_stats()
        hal.kernel_timing(False)
        ms = {k: v["total_ms"] / 5 for k, v in st.items() if v["launches"]}
        print("%-34s " % label + "  ".join("%s=%.4f ms" % kv for kv in ms.items()) + "  sum=%.4f ms" % sum(ms.values()), flush=True)

    # a segment's group transform (plain inverse, then x4), and the sizes of its late FRI rounds and of small circuits: the inverse
    # with the coset shift at 2^out, the x4 transform into 2^out
    for c, inv_po2, shift, in_po2 in ((cols, 20, False, 20), (64, 13, True, 11), (64, 14, True, 12), (64, 15, True, 13)):
        src = hal.copy_from(rng.integers(0, r0.P, c << max(inv_po2, in_po2), dtype=np.uint32))
        ev = hal.alloc(c << (in_po2 + 2))
        intt = hal.batch_interpolate_ntt_zk_shift if shift else hal.batch_interpolate_ntt
        timed("intt%s %d columns of 2^%d:" % ("+shift" if shift else "", c, inv_po2), lambda: intt(src, c, inv_po2))
        timed("ntt x4 %d columns of 2^%d:" % (c, in_po2), lambda: hal.batch_expand_into_evaluate_ntt(ev, src, c, in_po2, 2))
        src.free(); ev.free()
    print("lib", os.path.basename(r0.LIB_PATH), "outputs sha256", digest.hexdigest())
    hal.close()


if __name__ == "__main__":
    main()
