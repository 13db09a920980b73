#!/usr/bin/env python3
"""What verifying seals costs the host, with and without the device hashing their Merkle openings (profiles/r16/verify_on_device.md).
One process on one GPU: a camt53 session is proved once (2^20-row trace-circuit seals), then, taking turns,
  * r0h_verify_seal_roots of one seal (the immediate verifier: every opening hashed on host threads), as it runs and with the
    process held to one processor,
  * r0h_verify_seals_on with ctx == NULL for one seal (the collecting walk, the batch hashed on the calling thread),
  * r0h_verify_seals_on on the device for n = 1 and for all seals of the receipt,
each with wall time, process CPU time (user + sys), merkle_climb_kernel's device time and the upload size; and r0h_compress of the
receipt on --lanes lanes with r0h_recursor_set_verify_on_device off and on, wall and process CPU time.
usage: ab_verify_on_device.py [--po2 20] [--rounds 5] [--lanes 4] [--recursion-po2 18] [--out file.json]"""
import argparse
import json
import os
import resource
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def cpu_s():
    u = resource.getrusage(resource.RUSAGE_SELF)
    return u.ru_utime + u.ru_stime


def timed(fn):
    c0, t0 = cpu_s(), time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3, (cpu_s() - c0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=4)
    ap.add_argument("--recursion-po2", type=int, default=18)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import guest_camt53
    import hyperfridge_r0_amd as r0
    from hyperfridge_r0_amd import recursion
    from verify_mutations import regions
    blob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32)
    hal = r0.Hal(0)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    image, stream, _ = guest_camt53.elf_and_input(form=1)
    receipt, image_id, cycles = hal.prove_elf(gc, image, stream, segment_po2=a.po2)
    seals = [s for _, s in receipt.seals()]
    sizes = [r0.verify_seal(blob, s)[2] for s in seals]
    roots = {size: hal.code_root(gc, size) for size in sorted(set(sizes))}
    per_seal = [roots[size] for size in sizes]
    first = next(i for i, size in enumerate(sizes) if size == a.po2)
    seal, root = seals[first], roots[a.po2]
    layout = regions(blob, seal)
    openings = layout["opening"]
    span_words = openings[(layout["fri"][-1], 49)][2] - openings[("accum", 0)][0]
    n_jobs = len(openings)
    res = {"segments": len(seals), "cycles": int(cycles), "seal_words": int(seal.size), "seal_po2": a.po2, "jobs_per_seal": n_jobs,
           "upload_bytes_per_seal": int(span_words * 4 + n_jobs * 16), "rounds": a.rounds}
    verdict, po2 = r0._c.c_int(-1), r0._u32(0)
    data_root = np.zeros(8, dtype=np.uint32)

    def immediate():
        r0._check(r0.lib().r0h_verify_seal_roots(blob.ctypes.data, blob.size, seal.ctypes.data, seal.size, root.ctypes.data, r0.ctypes.byref(verdict), r0.ctypes.byref(po2),
                                                 data_root.ctypes.data))
        assert verdict.value == 0

    def launches_ms():
        st = hal.kernel_stats().get("merkle_climb_kernel", {"launches": 0, "total_ms": 0.0})
        return st["launches"], st["total_ms"]

    hal.kernel_timing(True)
    runs = {"immediate_1": [], "immediate_1_one_cpu": [], "collecting_host_1": [], "device_1": [], "device_all": []}
    for rnd in range(a.rounds + 1):  # round 0 warms up
        row = {}
        _, w, c = timed(immediate)
        row["immediate_1"] = {"wall_ms": w, "cpu_ms": c}
        allowed = os.sched_getaffinity(0)  # the same call with the process held to ONE processor: its threads take turns on it
        os.sched_setaffinity(0, {min(allowed)})
        try:
            _, w, c = timed(immediate)
        finally:
            os.sched_setaffinity(0, allowed)
        row["immediate_1_one_cpu"] = {"wall_ms": w, "cpu_ms": c}
        got, w, c = timed(lambda: r0.verify_seals(blob, [seal], [root]))
        assert got[0][0] == 0 and np.array_equal(got[0][3], data_root)
        row["collecting_host_1"] = {"wall_ms": w, "cpu_ms": c}
        for name, ss, rr in (("device_1", [seal], [root]), ("device_all", seals, per_seal)):
            l0, k0 = launches_ms()
            got, w, c = timed(lambda: hal.verify_seals(blob, ss, rr))
            l1, k1 = launches_ms()
            assert all(g[0] == 0 for g in got) and l1 - l0 == 1
            row[name] = {"wall_ms": w, "cpu_ms": c, "kernel_ms": k1 - k0}
        if rnd:
            for k, v in row.items():
                runs[k].append({x: round(y, 3) for x, y in v.items()})
    hal.kernel_timing(False)
    res["verify"] = runs
    rec_blob = np.fromfile(entry.circuit_blob_path("recursion"), dtype=np.uint32)
    rec = recursion.Recursor(hal, rec_blob, blob, entry.code_object_path("recursion"), po2=a.recursion_po2, segment_roots=roots)
    comp = {"off": [], "on": []}
    want = None
    for rnd in range(4):  # round 0 warms up
        for mode in ("off", "on"):
            rec.set_verify_on_device(mode == "on")
            node, w, c = timed(lambda: rec.compress(receipt, lanes=a.lanes))
            if want is None:
                want = node.seal
            assert np.array_equal(node.seal, want)
            if rnd:
                comp[mode].append({"wall_s": round(w / 1e3, 4), "cpu_s": round(c / 1e3, 4)})
    rec.set_verify_on_device(False)
    res["compress"] = {"lanes": a.lanes, "recursion_po2": a.recursion_po2, "same_root_word_for_word": True, **comp}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    rec.close()


if __name__ == "__main__":
    main()
