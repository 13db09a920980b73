#!/usr/bin/env python3
"""The log-derivative steps of one trace-circuit segment with their challenges from the host (r0h_logup_totals, r0h_accum_public) and
from device buffers (r0h_logup_totals_device, r0h_accum_public_device), taking turns (profiles/r23/session_enqueue.md).  One process on
one GPU; the segment is the first one of the store-loop guest at 2^--po2 rows, expanded on the device.  Per round and form: wall time of
the two calls up to a stream sync, the times the library waited for the stream inside them; then, in a pass of its own,
r0h_kernel_timing of both forms.  The ACCUM columns and the totals of the two forms must be equal.
usage: ab_logup_device.py [--po2 20] [--rounds 5] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import hyperfridge_r0_amd as r0
    from bench_session import elf_of
    from test_rv32im import _guest
    entry.ensure_built()
    blob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32)
    hal = r0.Hal(0)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    vm = r0.Vm()
    vm.load_elf(elf_of(_guest((7 << a.po2) // 56), 0x400))    # a segment that is seven eighths cycles
    vm.set_input([7, 0x01020304])
    assert vm.run(segment_po2=a.po2, keep_trace=True, boundary_rows=True) == (0, 0)
    rows, bounds = vm.preflight_arrays(0)
    seg = vm.segments()[0]
    data, glob = hal.trace_witgen(rows, bounds, a.po2, claim_globals=vm.claims()[0].globals(), number=1, closing=bool(seg.closing), idle_pc=seg.pre.pc, circuit=gc)
    code, synthetic, _ = hal.witgen(gc, a.po2, 0)
    synthetic.free()
    rng = np.random.default_rng(23)
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = rng.integers(1, r0.P, size=16)
    mix = rng.integers(0, r0.P, size=gc.n_mix).astype(np.uint32)
    mbuf = hal.copy_from(mix)

    def host_form():
        full = hal.logup_totals(gc, a.po2, code, data, glob)
        return full, hal.accum_public(gc, a.po2, code, data, full, mix)

    def device_form():
        gbuf = hal.copy_from(glob)
        hal.logup_totals_device(gc, a.po2, code, data, gbuf)
        accum = hal.accum_public_device(gc, a.po2, code, data, gbuf, mbuf)
        return gbuf, accum

    forms = {"host": host_form, "device": device_form}
    out = {"po2": a.po2, "rows_in_use": int(rows.shape[0] + bounds.shape[0]), "wall_ms": {k: [] for k in forms}, "blocking_waits": {}}
    want = None
    for r in range(a.rounds + 1):  # (round 0 warms up)
        for name, fn in (list(forms.items()) if r % 2 == 0 else list(forms.items())[::-1]):
            hal.sync()
            w0, t0 = hal.blocking_waits(), time.perf_counter()
            g, accum = fn()
            inside = hal.blocking_waits() - w0
            hal.sync()
            ms = 1e3 * (time.perf_counter() - t0)
            if r:
                out["wall_ms"][name].append(round(ms, 3))
            out["blocking_waits"][name] = inside
            got = (np.asarray(g.to_host() if name == "device" else g), accum.to_host())
            if want is None:
                want = got
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
            accum.free()
            if name == "device":
                g.free()
    for name, fn in forms.items():  # events around every launch: a pass of its own
        hal.kernel_timing(True)
        g, accum = fn()
        hal.sync()
        out.setdefault("kernel_ms", {})[name] = {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 4)} for k, v in hal.kernel_stats().items() if v["launches"]}
        hal.kernel_timing(False)
        accum.free()
        if name == "device":
            g.free()
    text = json.dumps(out)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
