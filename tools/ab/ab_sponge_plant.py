#!/usr/bin/env python3
"""A/B timing of the sponge plant of one lift (sponge_plant: the rows of the in-circuit sponge over a consumed seal written into a
recursion witness) across library builds, in one process on one box: the builds take turns, several rounds.  Per call: the host time
until the call returns, the time until the stream is idle (call + r0h_sync), and -- where the build has it -- sponge_rows_kernel's
own time from the library's kernel timing.  sponge_plant is internal (C++ linkage), reached by its mangled name.
usage: ab_sponge_plant.py [--po2 18] [--words 61000] [--rounds 5] name=path/to/libr0hip.so ..."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
_vp, _u32, _sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
PLANT = "_ZN3r0h12sponge_plantEP7r0h_ctxPK11r0h_circuitjPKjmP7r0h_buf"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--po2", type=int, default=18)
    ap.add_argument("--words", type=int, default=61000, help="a 2^20-row trace-circuit seal is about 61k words")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("libs", nargs="+")
    a = ap.parse_args()
    blob = np.fromfile(os.path.join(ROOT, "circuits", "recursion.r0c"), dtype=np.uint32)
    co = os.path.join(ROOT, "circuits", "recursion.evalcheck.hsaco").encode()
    words = np.random.default_rng(7).integers(0, 2013265921, a.words).astype(np.uint32)
    built = {}
    for spec in a.libs:
        name, path = spec.split("=", 1)
        L = ctypes.CDLL(os.path.abspath(path))
        for f in ("r0h_ctx_create", "r0h_circuit_load", "r0h_buf_alloc", "r0h_sync", "r0h_kernel_timing", "r0h_kernel_stats", "r0h_buf_d2h", PLANT):
            getattr(L, f).restype = _vp
        L.r0h_circuit_group_size.restype = _u32
        ctx, circ, data = _vp(), _vp(), _vp()
        assert not L.r0h_ctx_create(0, ctypes.byref(ctx))
        assert not L.r0h_circuit_load(ctx, blob.ctypes.data_as(_vp), _sz(blob.size), co, ctypes.byref(circ))
        n_data = L.r0h_circuit_group_size(circ, _u32(2))
        assert not L.r0h_buf_alloc(ctx, _sz((n_data << a.po2) * 4), ctypes.byref(data))
        built[name] = (L, ctx, circ, data, n_data)
    res = {n: {"call_ms": [], "call_and_sync_ms": [], "kernel_ms": []} for n in built}
    rows = {}
    for rnd in range(a.rounds + 1):  # round 0 warms up
        for name, (L, ctx, circ, data, n_data) in built.items():
            plant = getattr(L, PLANT)
            assert not L.r0h_kernel_timing(ctx, 1)
            call = total = 0.0
            for _ in range(a.calls):
                assert not L.r0h_sync(ctx)
                t0 = time.perf_counter()
                err = plant(ctx, circ, _u32(a.po2), words.ctypes.data_as(_vp), _sz(words.size), data)
                t1 = time.perf_counter()
                assert not err, ctypes.cast(err, ctypes.c_char_p).value
                assert not L.r0h_sync(ctx)
                t2 = time.perf_counter()
                call += t1 - t0
                total += t2 - t0
            out = ctypes.create_string_buffer(1 << 16)
            assert not L.r0h_kernel_stats(ctx, out, _sz(len(out)))
            stats = json.loads(out.value.decode())
            assert not L.r0h_kernel_timing(ctx, 0)
            if rnd == 0:
                got = np.empty((n_data << a.po2), dtype=np.uint32)
                assert not L.r0h_buf_d2h(ctx, data, _sz(0), got.ctypes.data_as(_vp), _sz(got.nbytes))
                rows[name] = got
                continue
            res[name]["call_ms"].append(round(1e3 * call / a.calls, 4))
            res[name]["call_and_sync_ms"].append(round(1e3 * total / a.calls, 4))
            k = stats.get("sponge_rows_kernel")
            if k:
                res[name]["kernel_ms"].append(round(k["total_ms"] / k["launches"], 4))
    names = list(built)
    # the sponge's 65 columns (blob section SPONGE names the first) must be the same words in every build; nothing else was written here
    at, first = 3, None
    for _ in range(int(blob[2])):
        if int(blob[at]) == 12:
            first = int(blob[at + 3])
        at += 2 + int(blob[at + 1])
    cols = {n: rows[n].reshape(-1, 1 << a.po2)[first:first + 65] for n in names}
    same = all(np.array_equal(cols[names[0]], cols[n]) for n in names[1:])
    print(json.dumps({"po2": a.po2, "words": a.words, "calls_per_round": a.calls, "results": res, "sponge_columns_equal_across_builds": bool(same)}))


if __name__ == "__main__":
    sys.exit(main())
