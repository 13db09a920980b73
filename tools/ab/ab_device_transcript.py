#!/usr/bin/env python3
"""One segment proved with the transcript's tail on the host and on the device, taking turns (profiles/r21/device_transcript.md).
One process on one GPU: a synthetic witness of --circuit at 2^--po2 rows, CODE committed once, then per round r0h_prove_segment_committed
with r0h_ctx_set_device_transcript off and on: wall time of the call, the device time of its `fri_commit` and `queries` phases
(r0h_last_profile), the times the library waited for the stream (r0h_ctx_blocking_waits); the seals must be equal.  Then, in a pass
of its own (events around every launch slow the host), r0h_kernel_timing of the kernels the switch brings in.
usage: ab_device_transcript.py [--circuit bench] [--po2 20] [--rounds 5] [--hashfn poseidon2] [--out file.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", default="bench")
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--hashfn", default="poseidon2")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import hyperfridge_r0_amd as r0
    entry.ensure_built()
    blob = np.fromfile(entry.circuit_blob_path(a.circuit), dtype=np.uint32)
    hal = r0.Hal(0)
    hal.set_hashfn(a.hashfn)
    co = entry.code_object_path(a.circuit)
    gc = hal.load_circuit(blob, co if os.path.exists(co) else None)
    code, data, glob = hal.witgen(gc, a.po2, 1)
    cc = hal.code_commit(gc, a.po2)
    seals = {}
    rows = {False: [], True: []}

    def prove(on):
        hal.set_device_transcript(on)
        hal.sync()
        w0, t0 = hal.blocking_waits(), time.perf_counter()
        seal = hal.prove_segment(gc, a.po2, cc, data, glob)
        wall = (time.perf_counter() - t0) * 1e3
        waits = hal.blocking_waits() - w0
        phases = dict(hal.last_profile())
        return seal, {"wall_ms": round(wall, 3), "fri_commit_ms": round(phases["fri_commit"], 4), "queries_ms": round(phases["queries"], 4),
                      "all_phases_ms": round(sum(phases.values()), 3), "blocking_waits": waits}

    for on in (False, True):  # warm-up: code objects, pools
        seals[on], _ = prove(on)
    assert np.array_equal(seals[False], seals[True]), "the seals differ"
    for _ in range(a.rounds):
        for on in (False, True):
            seal, row = prove(on)
            assert np.array_equal(seal, seals[False])
            rows[on].append(row)
    kernels = {}
    for on in (False, True):
        hal.set_device_transcript(on)
        hal.kernel_timing(True)
        for _ in range(a.rounds):
            hal.prove_segment(gc, a.po2, cc, data, glob)
        stats = hal.kernel_stats()
        hal.kernel_timing(False)
        kernels["on" if on else "off"] = {k: {"launches_per_proof": v["launches"] / a.rounds, "ms_per_proof": round(v["total_ms"] / a.rounds, 4)}
                                          for k, v in stats.items() if v["launches"] and ("iop_" in k or "fri_fold" in k or "merkle_open" in k or "hash_fold" in k)}
    hal.set_device_transcript(False)
    line = {"circuit": a.circuit, "po2": a.po2, "hashfn": a.hashfn, "rounds": a.rounds, "seal_words": int(seals[False].size), "host_transcript": rows[False],
            "device_transcript": rows[True], "kernels": kernels}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    cc.free()
    for b in (code, data):
        b.free()
    gc.free()
    hal.close()


if __name__ == "__main__":
    main()
