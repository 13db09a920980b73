#!/usr/bin/env python3
"""One segment proof and one image proof in their blocking forms under r0h_ctx_set_device_finish (r0h_prove_segment_committed,
r0h_prove_image) and submitted and collected (r0h_prove_segment_committed_enqueue / r0h_prove_segment_collect, r0h_prove_image_enqueue /
r0h_prove_image_collect), taking turns (profiles/r27/begin_enqueue.md).  One process on one GPU.  Per round and form: wall time from the
first call to the seal, of it the time the calling thread spent before the collect (what it could have spent enqueueing elsewhere), and
the times the library waited for the stream.  The seals of the two forms must be equal.  The segment is --circuit at 2^--po2 rows; the
image is the ALU corner program's (tests/trace_corners.py).
usage: ab_begin_enqueue.py [--circuit bench] [--po2 16] [--rounds 5] [--out file.json]"""
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
    ap.add_argument("--circuit", default="bench")
    ap.add_argument("--po2", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import __graft_entry__ as entry
    import hyperfridge_r0_amd as r0
    from bench_session import elf_of
    import trace_corners as tcr
    entry.ensure_built()
    hal = r0.Hal(0)
    hal.set_device_finish(True)
    gc = hal.load_circuit(np.fromfile(entry.circuit_blob_path(a.circuit), dtype=np.uint32), None if a.circuit == "tiny" else entry.code_object_path(a.circuit))
    ic = hal.load_circuit(np.fromfile(entry.circuit_blob_path("image"), dtype=np.uint32), entry.code_object_path("image"))
    code, data, glob = hal.witgen(gc, a.po2, 1)
    cc = hal.code_commit(gc, a.po2)
    elf = elf_of(tcr.PROGRAMS["alu"](), tcr.BASE)  # (only its image matters)
    challenge = np.random.default_rng(27).integers(1, r0.P, size=16).astype(np.uint32)

    def timed(first, second=None):
        hal.sync()
        w0, t0 = hal.blocking_waits(), time.perf_counter()
        got = first()
        t1 = time.perf_counter()
        if second is not None:
            got = second(got)
        t2 = time.perf_counter()
        return got, 1e3 * (t2 - t0), 1e3 * (t1 - t0), hal.blocking_waits() - w0

    forms = {
        "segment_blocking": lambda: timed(lambda: hal.prove_segment(gc, a.po2, cc, data, glob)),
        "segment_enqueue": lambda: timed(lambda: hal.prove_segment_enqueue(gc, a.po2, cc, data, glob), hal.prove_segment_collect),
        "image_blocking": lambda: timed(lambda: hal.prove_image(ic, elf, challenge)),
        "image_enqueue": lambda: timed(lambda: hal.prove_image_enqueue(ic, elf, challenge), hal.prove_image_collect),
    }
    out = {"circuit": a.circuit, "po2": a.po2, "image_po2": r0.image_po2(elf), "wall_ms": {k: [] for k in forms}, "before_collect_ms": {k: [] for k in forms}, "blocking_waits": {}}
    want = {}
    for r in range(a.rounds + 1):  # (round 0 warms up, and commits the image circuit's CODE group)
        for name in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            seal, wall, before, waits = forms[name]()
            kind = name.split("_")[0]
            assert np.array_equal(seal, want.setdefault(kind, seal)), name
            if r:
                out["wall_ms"][name].append(round(wall, 3))
                out["before_collect_ms"][name].append(round(before, 3))
            out["blocking_waits"][name] = waits
    text = json.dumps(out)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
