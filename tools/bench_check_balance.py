#!/usr/bin/env python3
"""The balance check timed on the workload it is for: the first 2^20-row segment of the camt53 session, trace circuit.
Four legs on the same witness, alternating, --rounds times in one process:
  balance   r0h_logup_check_balance: wall time of the call -- count, table from the pool, insert, scan, read-backs -- and its kernels
            alone (r0h_kernel_timing); with it the tuples, the table's slots and the share of inserts the LDS stage absorbed
  mult      r0h_logup_multiplicities on the same DATA group (the other walk over the lookups)
  checker   r0h_check_witness with the accumulation (every term, every row)
  proof     that segment's whole proof, the sum of r0h_last_profile's phases
and tools/trace_circuit.check_fractions (numpy) on the same witness once.  The witness is honest (every checker must say so); one JSON
line.
usage: python tools/bench_check_balance.py [--po2 20] [--rounds 3] [--no-numpy]"""
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
    ap.add_argument("--no-numpy", action="store_true", help="leave check_fractions out")
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.ensure_built()
    import hyperfridge_r0_amd as r0
    import guest_camt53
    from trace_circuit import check_fractions
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
    assert hal.logup_check_balance(gc, po2, code, data, full) == []  # (warm: pools filled)
    assert hal.check_witness(gc, po2, code, data, full, accum, mix) == []
    hal.prove_segment(gc, po2, cc, data, full)
    balance_ms, kernel_ms, mult_ms, checker_ms, proof_ms = [], [], [], [], []
    for _ in range(args.rounds):
        hal.kernel_timing(True)
        t0 = time.perf_counter()
        bad = hal.logup_check_balance(gc, po2, code, data, full)
        balance_ms.append(1e3 * (time.perf_counter() - t0))
        stats = hal.kernel_stats()
        hal.kernel_timing(False)
        assert bad == []
        kernel_ms.append(stats["logup_check_balance"]["total_ms"] - sum(kernel_ms))  # (the timers of a context add up over its life)
        t0 = time.perf_counter()
        hal.logup_multiplicities(gc, po2, data, full)
        mult_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        assert hal.check_witness(gc, po2, code, data, full, accum, mix) == []
        checker_ms.append(1e3 * (time.perf_counter() - t0))
        hal.prove_segment(gc, po2, cc, data, full)
        proof_ms.append(sum(ms for _, ms in hal.last_profile()))
    tuples, sent, slots = hal.logup_check_balance_stats()
    numpy_s = None
    if not args.no_numpy:
        m, g = canonical(data.to_host(), po2).astype(np.int64), canonical_globals(full)
        t0 = time.perf_counter()
        assert [b for b in check_fractions(m, g) if not b[0].startswith("session:")] == []
        numpy_s = round(time.perf_counter() - t0, 2)
    print(json.dumps({"segment": "first segment of the camt53 session (%s), %d cycles + %d boundary rows in 2^%d rows" % (what[:60], len(rows), len(bounds), po2),
                      "chain_fractions": gc.n_chain_fractions, "rounds": args.rounds,
                      "tuples": tuples, "table_slots": slots, "table_bytes": 32 * slots, "inserts_reaching_the_global_table": sent,
                      "share_absorbed_in_lds": round(1.0 - sent / max(tuples, 1), 4),
                      "check_balance_wall_ms": [round(v, 3) for v in balance_ms],
                      "check_balance_kernels_and_readbacks_ms": [round(v, 3) for v in kernel_ms],
                      "logup_multiplicities_wall_ms": [round(v, 3) for v in mult_ms],
                      "check_witness_all_terms_wall_ms": [round(v, 3) for v in checker_ms],
                      "segment_proof_phases_ms": [round(float(v), 3) for v in proof_ms],
                      "check_fractions_numpy_s": numpy_s}))
    cc.free()
    gc.free()
    hal.close()


if __name__ == "__main__":
    main()
