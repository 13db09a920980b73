#!/usr/bin/env python3
"""The witness checker timed on the workload it is for: the first 2^20-row segment of the camt53 session, trace circuit, all terms.
Three things on the same witness, alternating, --rounds times in one process:
  device   r0h_check_witness with the accumulation (every term, every row): wall time of the call -- launch, kernels, the read-back of
           the table -- and the kernels alone (r0h_kernel_timing)
  numpy    tools/gen_circuit.py check_trace_rows, the host tool that named constraints before (DATA / CODE terms and the fractions)
  scale    the eval_check phase of the proof of that segment (r0h_last_profile): the same arithmetic on the 4N coset
The witness is honest (both checkers must say so); one JSON line.
usage: python tools/bench_check_witness.py [--po2 20] [--rounds 3] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-numpy", action="store_true", help="leave check_trace_rows out (it takes about a minute per round at 2^20 rows)")
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.ensure_built()
    import hyperfridge_r0_amd as r0
    import guest_camt53
    from gen_circuit import check_trace_rows
    from trace_corners import canonical, canonical_globals
    elf, stream, what = guest_camt53.elf_and_input()
    vm = r0.Vm()
    vm.load_elf(elf)
    vm.set_input(stream)
    finished, _, _ = vm.run_segment(segment_po2=args.po2, keep_trace=True, boundary_rows=True)
    rows, bounds = vm.preflight_arrays(0)
    hal = r0.Hal(0)
    blob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    gc.load_check(entry.check_code_object_path("trace"))
    po2 = args.po2
    data, glob = hal.trace_witgen(rows, bounds, po2, number=1, closing=finished, circuit=gc)
    code, unused, _ = hal.witgen(gc, po2, 0)
    unused.free()
    rng = np.random.default_rng(1)
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = rng.integers(0, r0.P, 16).astype(np.uint32)
    full = hal.logup_totals(gc, po2, code, data, glob)
    mix = rng.integers(0, r0.P, gc.n_mix).astype(np.uint32)
    accum = hal.accum_public(gc, po2, code, data, full, mix)
    cc = hal.code_commit(gc, po2, code)
    assert hal.check_witness(gc, po2, code, data, full, accum, mix) == []  # (warm: module loaded, pools filled)
    hal.prove_segment(gc, po2, cc, data, full)
    m = g = None
    if not args.no_numpy:
        m, g = canonical(data.to_host(), po2), canonical_globals(full)
    device_ms, kernel_ms, numpy_s, eval_ms, early_ms = [], [], [], [], []
    for _ in range(args.rounds):
        hal.kernel_timing(True)
        t0 = time.perf_counter()
        bad = hal.check_witness(gc, po2, code, data, full, accum, mix)
        device_ms.append(1e3 * (time.perf_counter() - t0))
        stats = hal.kernel_stats()
        hal.kernel_timing(False)
        assert bad == []
        kernel_ms.append(stats["check_witness"]["total_ms"] - sum(kernel_ms))  # (the timers of a context add up over its life)
        t0 = time.perf_counter()
        assert hal.check_witness(gc, po2, code, data, full) == []
        early_ms.append(1e3 * (time.perf_counter() - t0))
        if m is not None:
            t0 = time.perf_counter()
            assert check_trace_rows(m, g) == []
            numpy_s.append(time.perf_counter() - t0)
        hal.prove_segment(gc, po2, cc, data, full)
        eval_ms.append(dict(hal.last_profile())["eval_check"])
    print(json.dumps({"segment": "first segment of the camt53 session (%s), %d cycles + %d boundary rows in 2^%d rows" % (what[:60], len(rows), len(bounds), po2),
                      "terms": gc.n_terms, "rounds": args.rounds,
                      "check_witness_all_terms_wall_ms": [round(v, 3) for v in device_ms],
                      "check_witness_kernels_ms": [round(v, 3) for v in kernel_ms],
                      "check_witness_before_the_mix_wall_ms": [round(v, 3) for v in early_ms],
                      "check_trace_rows_numpy_s": [round(v, 2) for v in numpy_s],
                      "eval_check_phase_ms": [round(float(v), 3) for v in eval_ms]}))
    cc.free()
    gc.free()
    hal.close()


if __name__ == "__main__":
    main()
