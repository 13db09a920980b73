#!/usr/bin/env python3
"""The session balance timed on the workload it is for: every segment of the camt53 session, trace circuit, as r0h_session_finish
feeds them under r0h_ctx_set_check_session -- a device handle, one r0h_session_balance_add per segment in index order, the verifier's
side from the ELF and the journal, one report.  --rounds times in one process on the same resident witnesses:
  add       wall time of each segment's addition (tape, count kernel, growth with its rehash, insert kernel, the closing read-back)
  verifier  r0h_session_balance_add_verifier_side: the ELF's image words and the journal's words through the list kernel
  report    scan, read-back (and compaction, had there been anything to report)
with the tuples each segment brings, the table's slots, how often it grew and the classes it holds, the closing segment's share of
the additions.  The session is honest (the report must be empty); one JSON line.
usage: python tools/bench_check_session.py [--po2 20] [--rounds 3]"""
import argparse
import json
import math
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
    ap.add_argument("--guest", default="camt53", choices=["camt53", "rsa"])
    args = ap.parse_args()
    import __graft_entry__ as entry
    entry.ensure_built()
    import hyperfridge_r0_amd as r0
    elf, stream, what = __import__("guest_" + args.guest).elf_and_input()
    vm = r0.Vm()
    vm.load_elf(elf)
    vm.set_input(stream)
    assert vm.run(segment_po2=args.po2, keep_trace=True, boundary_rows=True) == (0, 0)
    segs, claims = vm.segments(), vm.claims()
    hal = r0.Hal(0)
    blob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    code, witness = {}, []
    for k, seg in enumerate(segs):
        rows, bounds = vm.preflight_arrays(k)
        size = max(r0.TRACE_MIN_PO2, int(math.ceil(math.log2(max(2, len(rows) + len(bounds))))))
        data, glob = hal.trace_witgen(rows, bounds, size, claim_globals=claims[k].globals(), number=k + 1, closing=bool(seg.closing), idle_pc=seg.pre.pc, circuit=gc)
        if size not in code:
            code[size], unused, _ = hal.witgen(gc, size, 0)
            unused.free()
        witness.append((size, data, glob, len(rows), len(bounds)))
    journal = bytes(vm.journal)
    add_ms, verifier_ms, report_ms, stats, per_segment = [], [], [], None, None
    for rnd in range(args.rounds + 1):   # the first round fills the pools and is not reported
        sb = r0.SessionBalance(blob, hal)
        adds, tuples, before = [], [], 0
        for k, (size, data, glob, _, _) in enumerate(witness):
            t0 = time.perf_counter()
            sb.add(k, size, code[size], data, glob, circuit=gc)
            adds.append(1e3 * (time.perf_counter() - t0))
            tuples.append(sb.stats()[0] - before)
            before += tuples[-1]
        t0 = time.perf_counter()
        sb.add_verifier_side(elf, journal)
        t1 = time.perf_counter()
        report = sb.report()
        t2 = time.perf_counter()
        assert report == [], report[:4]
        stats = sb.stats()
        sb.free()
        if rnd == 0:
            continue
        add_ms.append(adds)
        verifier_ms.append(1e3 * (t1 - t0))
        report_ms.append(1e3 * (t2 - t1))
        per_segment = tuples
    best = [min(r[k] for r in add_ms) for k in range(len(witness))]
    print(json.dumps({"session": "%s (%s), %d segments of at most 2^%d rows" % (args.guest, what[:60], len(witness), args.po2), "rounds": args.rounds,
                      "segments": [{"po2": w[0], "cycles": w[3], "boundary_rows": w[4], "closing": bool(segs[k].closing), "session_tuples": per_segment[k], "add_ms_best": round(best[k], 3)}
                                   for k, w in enumerate(witness)],
                      "tuples": stats[0], "table_slots": stats[1], "table_bytes": 64 * stats[1], "grows": stats[2], "classes": stats[3],
                      "add_ms_per_round_all_segments": [round(sum(r), 3) for r in add_ms],
                      "closing_segment_share_of_additions": round(best[-1] / sum(best), 4),
                      "verifier_side_ms": [round(v, 3) for v in verifier_ms], "report_ms": [round(v, 3) for v in report_ms],
                      "session_ms_per_round": [round(sum(r) + v + w, 3) for r, v, w in zip(add_ms, verifier_ms, report_ms)]}))
    for c in code.values():
        c.free()
    gc.free()
    hal.close()


if __name__ == "__main__":
    main()
