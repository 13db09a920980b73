#!/usr/bin/env python3
"""r0h_hash_fold_top / r0h_ctx_set_merkle_fused_tops against the launch per level, taking turns on one GPU
(profiles/r24/merkle_fused_tops.md).  Three modes, one JSON line each:

  top       in this process, per hash suite: the levels of 8192 .. 1 parents as the loop of fourteen r0h_hash_fold calls and as one
            r0h_hash_fold_top, in turn, below trees of 2^14 .. 2^22 leaves (the top is the same work under every tree; what differs
            is what the larger tree's lower levels left in the caches) -- host wall time from an idle stream to an idle stream, and
            in a pass of its own the HIP events of r0h_kernel_timing; then r0h_merkle_build as a whole, switch off and on.  With
            R0HIP_AB_LIB a variant build of the library is measured (tools/ab/build_variants.sh with -DR0H_MERKLE_FUSED_SPLIT=a
            or -DR0H_MERKLE_FUSED_WG=n): the nodes are compared with the loop's in every case.
  sessions  in this process: prove(env, elf) over the trace circuit at 2^--po2 rows per segment with the switch off and on, in turn:
            one segment on one lane, four segments on four lanes, one segment with the image proof.  Receipts must be equal.
  turns     fresh child processes, in turn, in the order A B B A ..: `--cmd LABEL=ENV,..:command` as often as wanted, e.g.
            --cmd off=R0H_MERKLE_FUSED_TOPS=0:"python bench.py --gpus 1 --steps 8 --warmup 2"; --cwd LABEL=DIR runs a label's command
            in another checkout (the parent commit's, built there).  From each child's last JSON line the values at --key
            (dotted paths, several allowed) are collected per label.
usage: ab_merkle_fused.py top|sessions|turns [--rounds N] [--out file.json] ..."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    return {"min": round(min(values), 4), "max": round(max(values), 4), "all": [round(v, 4) for v in values]}


def mode_top(a):
    import hyperfridge_r0_amd as r0
    if os.environ.get("R0HIP_AB_LIB"):
        r0.LIB_PATH = os.path.abspath(os.environ["R0HIP_AB_LIB"])
    out = {"mode": "top", "lib": os.environ.get("R0HIP_AB_LIB", "the tree's"), "rounds": a.rounds, "suites": {}}
    for suite in ("poseidon2", "sha-256"):
        hal = r0.Hal(0)
        hal.set_hashfn(suite)
        hal.set_merkle_fused_tops(False)
        res = out["suites"][suite] = {}
        for k in a.leaves:
            rows, cols = 1 << k, 8
            rng = np.random.default_rng(k)
            matrix = hal.copy_from(rng.integers(0, r0.P, rows * cols, dtype=np.uint32))
            nodes, other = hal.alloc(2 * rows * 8), hal.alloc(2 * rows * 8)
            hal.merkle_build(nodes, matrix, rows, cols)
            want = nodes.to_host()

            def loop(buf):
                sz = min(rows // 2, 8192)
                while sz >= 1:
                    hal.hash_fold(buf, sz)
                    sz //= 2

            forms = {"loop": loop, "fused": lambda buf: hal.hash_fold_top(buf, min(rows // 2, 8192))}
            wall = {name: [] for name in forms}
            for r in range(a.rounds + 1):  # (round 0 warms up)
                for name in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
                    hal.sync()
                    t0 = time.perf_counter()
                    forms[name](nodes)
                    hal.sync()
                    if r:
                        wall[name].append(1e6 * (time.perf_counter() - t0))
                    assert np.array_equal(nodes.to_host(), want), (suite, k, name)
            events = {}
            for name in forms:  # events around every launch: a pass of its own
                hal.kernel_timing(True)
                for _ in range(a.rounds):
                    forms[name](nodes)
                events[name] = {kn: {"launches": v["launches"] // a.rounds, "us": round(1e3 * v["total_ms"] / a.rounds, 2)} for kn, v in hal.kernel_stats().items() if v["launches"]}
                hal.kernel_timing(False)
            build = {"off": [], "on": []}
            for r in range(a.rounds + 1):
                for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
                    hal.set_merkle_fused_tops(name == "on")
                    hal.sync()
                    t0 = time.perf_counter()
                    hal.merkle_build(other, matrix, rows, cols)
                    hal.sync()
                    if r:
                        build[name].append(1e6 * (time.perf_counter() - t0))
            hal.set_merkle_fused_tops(False)
            assert np.array_equal(other.to_host()[8:], want[8:]), (suite, k)
            res["2^%d" % k] = {"top_wall_us": {n: spread(v) for n, v in wall.items()}, "top_event_us": events, "merkle_build_wall_us": {n: spread(v) for n, v in build.items()}}
            matrix.free(), nodes.free(), other.free()
        hal.close()
    return out


def mode_sessions(a):
    import __graft_entry__ as entry
    import hyperfridge_r0_amd as r0
    from bench_session import elf_of
    from test_rv32im import _guest
    entry.ensure_built()
    blob, iblob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32), np.fromfile(entry.circuit_blob_path("image"), dtype=np.uint32)
    hal = r0.Hal(0)
    gc, ic = hal.load_circuit(blob, entry.code_object_path("trace")), hal.load_circuit(iblob, entry.code_object_path("image"))
    per_segment = (7 << a.po2) // 8                      # a segment that is seven eighths cycles
    configs = {"1 segment, 1 lane": (1, "1", False), "4 segments, 4 lanes": (4, "4", False), "1 segment and the image proof, 1 lane": (1, "1", True)}
    out = {"mode": "sessions", "po2": a.po2, "rounds": a.rounds, "configs": {}}
    for label, (segments, lanes, image) in configs.items():
        elf = elf_of(_guest((segments * per_segment - per_segment // 2) // 7), 0x400)
        os.environ["R0H_SESSION_LANES"] = lanes
        hal.set_image_circuit(ic if image else None)
        wall, prove_ms, want, n = {"off": [], "on": []}, {"off": [], "on": []}, None, 0
        for r in range(a.rounds + 1):  # (round 0 warms up)
            for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
                hal.set_merkle_fused_tops(name == "on")
                hal.sync()
                t0 = time.perf_counter()
                receipt, _, _ = hal.prove_elf(gc, elf, [7, 0x01020304], segment_po2=a.po2)
                hal.sync()
                if r:
                    wall[name].append(1e3 * (time.perf_counter() - t0))
                    prove_ms[name].append(hal.last_session_stats()["prove_ms"])
                text = receipt.to_json()
                want, n = want or text, len(receipt.seals())
                assert text == want, (label, name)
        hal.set_merkle_fused_tops(False)
        hal.set_image_circuit(None)
        del os.environ["R0H_SESSION_LANES"]
        out["configs"][label] = {"segments": n, "wall_ms": {k: spread(v) for k, v in wall.items()}, "device_prove_ms_per_session": {k: spread(v) for k, v in prove_ms.items()}}
    gc.free(), ic.free()
    hal.close()
    return out


def dig(obj, path):
    for part in path.split("."):
        obj = obj[int(part)] if isinstance(obj, list) else obj[part]
    return obj


def mode_turns(a):
    cmds, cwds = {}, dict(c.split("=", 1) for c in a.cwd)
    for spec in a.cmd:
        head, command = spec.split(":", 1)
        label, _, env = head.partition("=")
        cmds[label] = (dict(e.split("=", 1) for e in env.split(",") if e), command)
    labels = list(cmds)
    out = {"mode": "turns", "rounds": a.rounds, "order": [], "values": {label: {key: [] for key in a.key} for label in labels}}
    for r in range(a.rounds):
        for label in (labels if r % 2 == 0 else labels[::-1]):
            env, command = cmds[label]
            child = subprocess.run(command, shell=True, cwd=cwds.get(label, ROOT), env=dict(os.environ, **env), stdout=subprocess.PIPE, text=True, timeout=a.timeout)
            if child.returncode != 0:
                raise SystemExit("ab_merkle_fused.py: %s: `%s` ended with status %d" % (label, command, child.returncode))
            line = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("{")][-1])
            out["order"].append(label)
            for key in a.key:
                out["values"][label][key].append(dig(line, key))
            print("ab_merkle_fused.py: %s %s" % (label, {key: out["values"][label][key][-1] for key in a.key}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("top", "sessions", "turns"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leaves", type=int, nargs="*", default=[14, 16, 18, 20, 22], help="top: log2 of the trees' leaves")
    ap.add_argument("--po2", type=int, default=20, help="sessions: log2 of a segment's rows")
    ap.add_argument("--cmd", action="append", default=[], help="turns: LABEL[=ENV=value,..]:command")
    ap.add_argument("--cwd", action="append", default=[], help="turns: LABEL=directory the label's command runs in")
    ap.add_argument("--key", action="append", default=[], help="turns: dotted path into the child's JSON line")
    ap.add_argument("--timeout", type=float, default=300.0, help="turns: seconds a child may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    out = {"top": mode_top, "sessions": mode_sessions, "turns": mode_turns}[a.mode](a)
    text = json.dumps(out)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
