#!/usr/bin/env python3
"""One segment proved with the transcript on the host, with its tail on the device (r0h_ctx_set_device_transcript) and with all of a
proof's second half on the device (r0h_ctx_set_device_finish), taking turns (profiles/r22/device_finish.md).  One process on one GPU, a
synthetic witness of --circuit at 2^--po2 rows, CODE committed once.
  pass 1  per round r0h_prove_segment_committed under the three settings: wall time of the call, device ms per phase
          (r0h_last_profile), the times the library waited for the stream (r0h_ctx_blocking_waits); the seals must be equal.
  pass 2  (events around every launch slow the host, so on its own) r0h_kernel_timing of the kernels the switches bring in.
  pass 3  what the split is for, --segments segments each: (a) one thread, one context, blocking finish; (b) two threads, a context
          each, blocking finish; (c) one thread, two contexts, r0h_proof_finish_enqueue / r0h_proof_finish_collect interleaved.
          Witness resident, CODE committed, the accumulation inside the timed loop.  Segments per second of each.
usage: ab_device_finish.py [--circuit bench] [--po2 20] [--rounds 5] [--segments 8] [--hashfn poseidon2] [--out file.json]"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SETTINGS = ("host", "device_transcript", "device_finish")
NEW = ("iop_", "fri_fold", "ext_powers", "deep_points", "interpolate_regs", "deep_head", "divide_jobs", "divide_report")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--circuit", default="bench")
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--segments", type=int, default=8)
    ap.add_argument("--hashfn", default="poseidon2")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import hyperfridge_r0_amd as r0
    entry.ensure_built()
    blob = np.fromfile(entry.circuit_blob_path(a.circuit), dtype=np.uint32)
    co = entry.code_object_path(a.circuit)

    class Lane:
        """a context with the circuit, a resident witness and the committed CODE group"""

        def __init__(self):
            self.hal = r0.Hal(0)
            self.hal.set_hashfn(a.hashfn)
            self.gc = self.hal.load_circuit(blob, co if os.path.exists(co) else None)
            self.code, self.data, self.glob = self.hal.witgen(self.gc, a.po2, 1)
            self.cc = self.hal.code_commit(self.gc, a.po2)

        def set(self, setting):
            self.hal.set_device_transcript(setting == "device_transcript")
            self.hal.set_device_finish(setting == "device_finish")

        def begin(self):
            proof, mix = self.hal.proof_begin(self.gc, a.po2, self.cc, self.data, self.glob)
            return proof, self.hal.accum(self.gc, a.po2, self.code, self.data, mix)

        def close(self):
            self.cc.free()
            for b in (self.code, self.data):
                b.free()
            self.gc.free()
            self.hal.close()

    lanes = [Lane(), Lane()]
    one = lanes[0]
    hal = one.hal

    def prove(setting):
        one.set(setting)
        hal.sync()
        w0, t0 = hal.blocking_waits(), time.perf_counter()
        seal = hal.prove_segment(one.gc, a.po2, one.cc, one.data, one.glob)
        wall = (time.perf_counter() - t0) * 1e3
        waits = hal.blocking_waits() - w0
        phases = {k: round(v, 4) for k, v in hal.last_profile()}
        return seal, {"wall_ms": round(wall, 3), "phases_ms": phases, "all_phases_ms": round(sum(phases.values()), 3), "blocking_waits": waits}

    seals = {s: prove(s)[0] for s in SETTINGS}  # warm-up: code objects, pools
    assert all(np.array_equal(seals[s], seals["host"]) for s in SETTINGS), "the seals differ"
    rows = {s: [] for s in SETTINGS}
    for _ in range(a.rounds):
        for s in SETTINGS:
            seal, row = prove(s)
            assert np.array_equal(seal, seals["host"])
            rows[s].append(row)

    kernels = {}
    for s in SETTINGS:
        one.set(s)
        hal.kernel_timing(True)
        for _ in range(a.rounds):
            hal.prove_segment(one.gc, a.po2, one.cc, one.data, one.glob)
        stats = hal.kernel_stats()
        hal.kernel_timing(False)
        kernels[s] = {k: {"launches_per_proof": v["launches"] / a.rounds, "ms_per_proof": round(v["total_ms"] / a.rounds, 4)} for k, v in stats.items()
                      if v["launches"] and any(n in k for n in NEW)}

    # ---- pass 3
    def blocking(lane, count, out):
        for _ in range(count):
            proof, accum = lane.begin()
            out.append(lane.hal.proof_finish(proof, accum))
            accum.free()

    def form_a():
        out = []
        blocking(one, a.segments, out)
        return out

    def form_b():
        outs = [[], []]
        threads = [threading.Thread(target=blocking, args=(lanes[k], a.segments // 2, outs[k])) for k in range(2)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        return outs[0] + outs[1]

    def form_c():
        out, flying = [], [None, None]
        for i in range(a.segments + 2):
            lane = lanes[i % 2]
            if flying[i % 2] is not None:  # the proof enqueued on this context two steps ago: collect it, then put the next behind it
                proof, accum = flying[i % 2]
                out.append(lane.hal.proof_finish_collect(proof))
                accum.free()
                flying[i % 2] = None
            if i < a.segments:
                proof, accum = lane.begin()
                lane.hal.proof_finish_enqueue(proof, accum)
                flying[i % 2] = (proof, accum)
        return out

    split = {}
    for lane in lanes:
        lane.set("device_finish")
    for name, form in (("a_one_thread_one_context", form_a), ("b_two_threads_two_contexts", form_b), ("c_one_thread_two_contexts_enqueue_collect", form_c)):
        form()  # warm-up of both contexts' pools
        rates = []
        for _ in range(3):
            for lane in lanes:
                lane.hal.sync()
            t0 = time.perf_counter()
            got = form()
            rates.append(round(len(got) / (time.perf_counter() - t0), 3))
            assert all(np.array_equal(s, seals["host"]) for s in got)
        split[name] = rates
    for lane in lanes:
        lane.set("host")

    line = {"circuit": a.circuit, "po2": a.po2, "hashfn": a.hashfn, "rounds": a.rounds, "seal_words": int(seals["host"].size), "settings": rows, "kernels": kernels,
            "segments_per_s": split, "segments_per_form": a.segments}
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    for lane in lanes:
        lane.close()


if __name__ == "__main__":
    main()
