#!/usr/bin/env python3
"""One-shot timing of the log-derivative steps away from the headline's shape: r0h_logup_multiplicities, r0h_logup_totals and
r0h_accum_public on a generated circuit with one table (tests/logup_circuits.py) at the sizes given (default 16 and 24, the ends of the
range), every call synchronous, `--reps` calls each (min and max printed).  `R0HIP_AB_LIB=<variant .so>` for A/B runs, as bench_ops.py;
`--cache DIR` keeps the witness between the runs of an A/B (2^24 rows take a while to draw).
usage: bench_logup.py [--reps N] [--cache DIR] [po2 ...]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import hyperfridge_r0_amd as r0

if os.environ.get("R0HIP_AB_LIB"):
    r0.LIB_PATH = os.path.abspath(os.environ["R0HIP_AB_LIB"])


def main():
    args, opts = sys.argv[1:], {"--reps": "5", "--cache": ""}
    for o in opts:
        if o in args:
            opts[o] = args[args.index(o) + 1]
            del args[args.index(o):args.index(o) + 2]
    sizes = [int(a) for a in args] or [16, 24]
    import logup_circuits as lc
    c = lc.generate(0, tables=[1], n_chain=1, n_public=1, lean=True)
    hal = r0.Hal(0)
    gc = hal.load_circuit(c.words)
    out = {"lib": r0.LIB_PATH, "reps": int(opts["--reps"]), "lookups_per_row": sum(1 for _ in c.lookups)}
    for po2 in sizes:
        path = os.path.join(opts["--cache"], "logup_witness_%d.npz" % po2) if opts["--cache"] else ""
        if path and os.path.exists(path):
            z = np.load(path)
            data, glob, mix = z["data"], z["glob"], z["mix"]
        else:
            data, glob, mix = c.witness(po2, seed=1)
            if path:
                np.savez(path, data=data, glob=glob, mix=mix)
        code, spare, _ = hal.witgen(gc, po2, seed=0)
        spare.free()
        db = hal.copy_from(data)

        def timed(fn):
            ms = []
            for _ in range(int(opts["--reps"]) + 1):
                hal.sync()
                t0 = time.perf_counter()
                r = fn()
                hal.sync()
                ms.append(1e3 * (time.perf_counter() - t0))
                if hasattr(r, "free"):
                    r.free()
            ms = ms[1:]  # the first call pays for the pool's allocations
            return {"min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}
        out["po2_%d" % po2] = {
            "multiplicities": timed(lambda: hal.logup_multiplicities(gc, po2, db, glob)),
            "totals": timed(lambda: hal.logup_totals(gc, po2, code, db, glob)),
            "accum_public": timed(lambda: hal.accum_public(gc, po2, code, db, glob, mix)),
        }
        for b in (code, db):
            b.free()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
