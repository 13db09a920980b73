"""r0h_check_witness on the device against tests/check_ref.py (the numpy interpreter of the blob's constraint program): honest
witnesses of every kind of circuit are clean, seeded single-cell mutations give the reference's table term for term, the check
before the mix covers exactly the reference's early terms, the sequencer's switch turns a seal no verifier accepts into an error
that names the term, and with the switch off nothing moves (the frozen seal)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import check_ref  # noqa: E402
import gen_circuit  # noqa: E402
import trace_corners as tcr  # noqa: E402
from trace_corners import COL, P  # noqa: E402

pytestmark = pytest.mark.gpu
PO2 = r0.TRACE_MIN_PO2
R = (1 << 32) % P


def enc(v):
    return int(v) * R % P


def words(rng, n):
    """n random field elements as device words (any word below p is the Montgomery form of some element)"""
    return rng.integers(0, P, n).astype(np.uint32)


def table(hal, gc, po2, code, data, glob, accum=None, mix=None):
    return {t: (rows, first) for t, rows, first in hal.check_witness(gc, po2, code, data, glob, accum, mix)}


def reference(blob, po2, code, data, glob, accum=None, mix=None):
    return check_ref.check(blob, po2, code.to_host(), data.to_host(), glob, accum.to_host() if accum is not None else None, mix)


@pytest.fixture(scope="module")
def trace(hal):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    gc.load_check(entry.check_code_object_path("trace"))  # the code object of the build (tiny goes through hipRTC on first use)
    yield blob, gc
    gc.free()


def synthetic(hal, name, po2, seed, code_object=None):
    """a synthetic circuit with its honest witness and accumulation; tiny compiles both of its modules in-process (hipRTC), the
    others load the code objects of the build"""
    code_object = name in entry.PRECOMPILED if code_object is None else code_object
    blob = np.fromfile(circuit_path(name), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path(name) if code_object else None)
    if code_object:
        gc.load_check(entry.check_code_object_path(name))
    code, data, glob = hal.witgen(gc, po2, seed)
    mix = words(np.random.default_rng(seed), gc.n_mix)
    accum = hal.accum(gc, po2, code, data, mix)
    return blob, gc, code, data, glob, accum, mix


def trace_witness(hal, trace, prog, seed=3):
    """the device witness of a corner program at 2^16 rows, its multiplicities, totals under a random challenge and accumulation"""
    blob, gc = trace
    vm = tcr.run(tcr.PROGRAMS[prog](), expect=(0, 0x00050003) if prog == "ecall" else (0, 0))
    rows, bounds = vm.preflight_arrays(0)
    data, glob = hal.trace_witgen(rows, bounds, PO2, circuit=gc)
    code, unused, _ = hal.witgen(gc, PO2, 0)
    unused.free()
    rng = np.random.default_rng(seed)
    glob = glob.copy()
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = words(rng, 16)
    full = hal.logup_totals(gc, PO2, code, data, glob)
    mix = words(rng, gc.n_mix)
    accum = hal.accum_public(gc, PO2, code, data, full, mix)
    return code, data, full, accum, mix, len(rows)


# ---- 1. honest witnesses
@pytest.mark.parametrize("name,po2", [("tiny", 9), ("tiny", 16), ("small", 9), ("small", 12), ("small", 16)])
def test_honest_synthetic_witnesses_violate_nothing(hal, name, po2):
    blob, gc, code, data, glob, accum, mix = synthetic(hal, name, po2, seed=po2)
    assert gc.n_terms == check_ref.Program(blob).n_and_eqz
    assert hal.check_witness(gc, po2, code, data, glob, accum, mix) == []
    assert hal.check_witness(gc, po2, code, data, glob) == []
    gc.free()


@pytest.mark.parametrize("prog", sorted(tcr.PROGRAMS))
def test_honest_trace_witnesses_violate_nothing(hal, trace, prog):
    code, data, full, accum, mix, _ = trace_witness(hal, trace, prog)
    assert hal.check_witness(trace[1], PO2, code, data, full, accum, mix) == []
    assert hal.check_witness(trace[1], PO2, code, data, full) == []


def test_an_honest_image_witness_and_a_recursion_node_violate_nothing(hal):
    from bench_session import elf_of
    from test_rv32im import _guest
    elf = elf_of(_guest(40), 0x400)
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = hal.load_circuit(iblob, entry.code_object_path("image"))
    po2 = r0.image_po2(elf)
    idata, iglob = r0.image_witness(elf, po2)
    rng = np.random.default_rng(9)
    iglob[r0.IMAGE_GAMMA:r0.IMAGE_GAMMA + 16] = words(rng, 16)
    code, unused, _ = hal.witgen(ic, po2, 0)
    unused.free()
    data = hal.copy_from(idata)
    full = hal.logup_totals(ic, po2, code, data, iglob)
    mix = words(rng, ic.n_mix)
    accum = hal.accum_public(ic, po2, code, data, full, mix)
    assert hal.check_witness(ic, po2, code, data, full, accum, mix) == []
    assert reference(iblob, po2, code, data, full, accum, mix) == {}
    # a digest that is not the image's: the sponge's tie to the public inputs objects, by name
    wrong = full.copy()
    wrong[0] = (int(wrong[0]) + 1) % P
    got = table(hal, ic, po2, code, data, wrong, accum, mix)
    assert got and got == reference(iblob, po2, code, data, wrong, accum, mix)
    names = gen_circuit.term_names("image")
    assert all(names[t].startswith("sponge:") for t in got)
    ic.free()
    # a node of the recursion tree: the recursion circuit's columns with the in-circuit sponge planted, at a node's size or below
    blob, rc, code, data, glob, accum, mix = synthetic(hal, "recursion", 12, seed=5)
    assert hal.check_witness(rc, 12, code, data, glob, accum, mix) == []
    rc.free()


# ---- 2. seeded single-cell mutations: the device's table is the reference's, term for term
@pytest.mark.parametrize("name,po2", [("tiny", 9), ("small", 10)])
def test_single_cell_mutations_of_a_synthetic_witness(hal, name, po2):
    blob, gc, code, data, glob, accum, mix = synthetic(hal, name, po2, seed=7)
    sites = check_ref.mutations(blob, po2, seed=11, count=20)
    assert {r for _, r, _ in sites} >= {0, (1 << po2) - 1}
    silent = 0
    for col, row, word in sites:
        at = col * (1 << po2) + row
        old = data.to_host(at, 1)
        data.upload(np.array([word], dtype=np.uint32), at)
        want = reference(blob, po2, code, data, glob, accum, mix)
        got = table(hal, gc, po2, code, data, glob, accum, mix)
        print("mutation", name, (col, row), "reference", want, "device", got)
        assert got == want, (col, row)
        silent += not want
        data.upload(old, at)
    assert silent * 10 <= len(sites), "vacuous: the reference is silent on %d of %d mutations" % (silent, len(sites))
    assert hal.check_witness(gc, po2, code, data, glob, accum, mix) == []
    gc.free()


def test_single_cell_mutations_of_a_trace_witness(hal, trace):
    blob, gc = trace
    code, data, full, accum, mix, n_rows = trace_witness(hal, trace, "alu")
    sites = check_ref.mutations(blob, PO2, seed=13, count=10, columns=[COL[c] for c in check_ref.TRACE_MUTATION_COLUMNS], rows=n_rows)
    names = gen_circuit.term_names("trace")
    silent = 0
    for col, row, word in sites:
        at = col * (1 << PO2) + row
        old = data.to_host(at, 1)
        data.upload(np.array([word], dtype=np.uint32), at)
        want = reference(blob, PO2, code, data, full, accum, mix)
        got = table(hal, gc, PO2, code, data, full, accum, mix)
        print("mutation trace", (gen_circuit.TRACE_COLUMNS[col], row), "reference", {names[t]: v for t, v in want.items()})
        assert got == want, (col, row)
        silent += not want
        data.upload(old, at)
    assert silent * 10 <= len(sites), "vacuous: the reference is silent on %d of %d mutations" % (silent, len(sites))


# ---- 3. before the mix is drawn
def test_without_accum_exactly_the_early_terms_are_reported(hal):
    po2 = 10
    blob, gc, code, data, glob, accum, mix = synthetic(hal, "small", po2, seed=21)
    pr = check_ref.Program(blob)
    rng = np.random.default_rng(2)
    bad = accum.to_host()
    bad[rng.integers(0, bad.size, 5)] = words(rng, 5)  # ACCUM cells: late terms only
    accum.upload(bad)
    for col, row, word in check_ref.mutations(blob, po2, seed=3, count=4):
        data.upload(np.array([word], dtype=np.uint32), col * (1 << po2) + row)
    full = reference(blob, po2, code, data, glob, accum, mix)
    early = table(hal, gc, po2, code, data, glob)
    assert any(pr.late[t] for t in full) and any(not pr.late[t] for t in full)
    assert early == {t: v for t, v in full.items() if not pr.late[t]} == reference(blob, po2, code, data, glob)
    assert table(hal, gc, po2, code, data, glob, accum, mix) == full
    gc.free()


# ---- 4. the sequencer's switch
def test_a_violated_trace_segment_still_proves_unless_the_switch_is_on(hal, orc, trace):
    blob, gc = trace
    vm = tcr.run(tcr.PROGRAMS["alu"]())
    rows, bounds = vm.preflight_arrays(0)
    data, glob = hal.trace_witgen(rows, bounds, PO2, circuit=gc)
    code, unused, _ = hal.witgen(gc, PO2, 0)
    unused.free()
    mid = len(rows) // 2
    data.upload(np.array([enc(0x5000)], dtype=np.uint32), COL["next_pc"] * (1 << PO2) + mid)  # a row that goes where the next one does not start
    hal.logup_multiplicities(gc, PO2, data, glob)
    glob = glob.copy()
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = words(np.random.default_rng(4), 16)
    full = hal.logup_totals(gc, PO2, code, data, glob)
    cc = hal.code_commit(gc, PO2, code)
    names = gen_circuit.term_names("trace")
    try:
        seal = hal.prove_segment(gc, PO2, cc, data, full)  # the parent's behaviour: a seal comes out ...
        root = cc.root()
        assert orc.circuit(blob).verify(seal, code_root=root)[0] != 0 and r0.verify_seal(blob, seal, code_root=root)[0] != 0  # ... that nobody accepts
        early = table(hal, gc, PO2, code, data, full)
        assert "run:pc" in {names[t] for t in early} and early == reference(blob, PO2, code, data, full)
        hal.set_check_witness(True)
        with pytest.raises(r0.R0HipError) as e:
            hal.prove_segment(gc, PO2, cc, data, full)
        first = min(early)
        assert "term %d does not vanish on %d of 2^%d rows, first at row %d" % (first, early[first][0], PO2, early[first][1]) in str(e.value)
        # the split sequencer: begin, late inputs, the caller's accumulation, finish
        h, _ = hal.proof_begin(gc, PO2, cc, data, full)
        mix = np.zeros(gc.n_mix, dtype=np.uint32)
        r0._check(r0.lib().r0h_proof_late(h, full[r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS:].ctypes.data_as(r0._vp), mix.ctypes.data_as(r0._vp)))
        accum = hal.accum_public(gc, PO2, code, data, full, mix)
        with pytest.raises(r0.R0HipError, match="the witness violates"):
            hal.proof_finish(h, accum)
    finally:
        hal.set_check_witness(False)
        cc.free()


def test_the_switch_leaves_honest_seals_alone(hal):
    want = np.load(os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy"))
    gc = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
    code, data, glob = hal.witgen(gc, 9, 1)
    assert np.array_equal(hal.prove_segment(gc, 9, code, data, glob), want)  # off: the parent's seal, word for word
    assert "check_witness" not in [n for n, _ in hal.last_profile()]
    hal.set_check_witness(True)
    try:
        assert np.array_equal(hal.prove_segment(gc, 9, code, data, glob), want)  # on, honest: the same seal
        assert "check_witness" in [n for n, _ in hal.last_profile()]
        data.upload(np.array([5], dtype=np.uint32), check_ref.mutations(gc.blob, 9, 1, 1)[0][0] << 9)
        with pytest.raises(r0.R0HipError, match="prove_segment: the witness violates"):
            hal.prove_segment(gc, 9, code, data, glob)
    finally:
        hal.set_check_witness(False)
    gc.free()


# ---- 5. wrong everywhere
@pytest.mark.parametrize("name,po2", [("tiny", 12), ("small", 12)])
def test_a_witness_that_is_wrong_everywhere(hal, name, po2):
    blob, gc, code, data, glob, accum, mix = synthetic(hal, name, po2, seed=31)
    data.upload(words(np.random.default_rng(8), data.words))
    want = reference(blob, po2, code, data, glob, accum, mix)
    got = table(hal, gc, po2, code, data, glob, accum, mix)
    assert got == want and len(want) > gc.n_terms // 2 and max(v[0] for v in want.values()) > (1 << po2) * 9 // 10
    gc.free()


def test_a_trace_witness_that_is_wrong_everywhere(hal, trace):
    blob, gc = trace
    code, data, full, accum, mix, _ = trace_witness(hal, trace, "control")
    data.upload(words(np.random.default_rng(6), data.words))
    want = reference(blob, PO2, code, data, full, accum, mix)
    assert table(hal, gc, PO2, code, data, full, accum, mix) == want and len(want) > gc.n_terms // 2


# ---- 6. argument errors
def test_argument_errors(hal):
    po2 = 9
    blob, gc, code, data, glob, accum, mix = synthetic(hal, "tiny", po2, seed=1)
    L, n = r0.lib(), ctypes.c_size_t(0)
    out = (r0.Violation * 4)()
    g, m = glob.ctypes.data_as(r0._vp), mix.ctypes.data_as(r0._vp)

    def call(ctx=hal.ctx, c=gc.handle, p=po2, a=accum.handle, co=code.handle, d=data.handle, gl=g, mx=m, o=out, cap=4, nn=ctypes.byref(n)):
        r0._check(L.r0h_check_witness(ctx, c, p, a, co, d, gl, mx, o, cap, nn))

    call()
    for kw in (dict(ctx=None), dict(c=None), dict(co=None), dict(d=None), dict(nn=None), dict(o=None)):
        with pytest.raises(r0.R0HipError, match="r0h_check_witness: NULL argument"):
            call(**kw)
    call(o=None, cap=0)
    for kw in (dict(gl=None), dict(mx=None)):
        with pytest.raises(r0.R0HipError, match="r0h_check_witness: NULL globals"):
            call(**kw)
    call(a=None, mx=None)  # before the mix there is none to give
    for p in (5, 25):
        with pytest.raises(r0.R0HipError, match="r0h_check_witness: po2 %d outside" % p):
            call(p=p)
    with pytest.raises(r0.R0HipError, match="buffer too small"):
        call(p=po2 + 1)
    bad = glob.copy()
    bad[0] = P
    with pytest.raises(r0.R0HipError, match=r"global\[0\] not canonical"):
        call(gl=bad.ctypes.data_as(r0._vp))
    bad = mix.copy()
    bad[3] = 0xFFFFFFFF
    with pytest.raises(r0.R0HipError, match=r"mix\[3\] not canonical"):
        call(mx=bad.ctypes.data_as(r0._vp))
    # more violated terms than room: the first `capacity` in term order, the total in n_out
    data.upload(words(np.random.default_rng(1), data.words))
    full = hal.check_witness(gc, po2, code, data, glob, accum, mix)
    assert len(full) > 4
    call()
    assert n.value == len(full) and [(out[i].term, out[i].rows, out[i].first_row) for i in range(4)] == full[:4]
    with pytest.raises(r0.R0HipError, match="room for 2"):
        hal.check_witness(gc, po2, code, data, glob, accum, mix, capacity=2)
    with pytest.raises(r0.R0HipError, match="loaded already"):
        gc.load_check()
    with pytest.raises(r0.R0HipError, match="has no check_witness_0"):
        hal.load_circuit(blob).load_check(entry.code_object_path("small"))
    gc.free()


# ---- 7. the command line
def test_cli_round_trip(tmp_path):
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    runs = []
    for extra in ([], ["--check-witness", "1"], ["--check-witness", "1", "--check-code-object", entry.check_code_object_path("small")]):
        out = subprocess.run([prove, circuit_path("small"), "--code-object", entry.code_object_path("small"), "--po2", "10", "--seed", "3", "--verify", "1"] + extra,
                             capture_output=True, text=True)
        assert out.returncode == 0 and "seals verified" in out.stderr, out.stdout + out.stderr
        runs.append(json.loads(out.stdout.splitlines()[0])["seal_fnv1a"])
    assert runs[0] == runs[1] == runs[2]
    # prove(env, elf) with the trace circuit and its names beside the blob: every segment checked, the receipt verified as before
    from bench_session import elf_of
    from test_rv32im import _guest
    (tmp_path / "guest.elf").write_bytes(elf_of(_guest(300), 0x400))
    np.array([7, 0x01020304], dtype=np.uint32).tofile(str(tmp_path / "input.bin"))
    out = subprocess.run([prove, circuit_path("trace"), "--code-object", entry.code_object_path("trace"), "--elf", str(tmp_path / "guest.elf"), "--input", str(tmp_path / "input.bin"),
                          "--po2", "16", "--receipt-out", str(tmp_path / "receipt.json"), "--check-witness", "1", "--check-code-object", entry.check_code_object_path("trace")],
                         capture_output=True, text=True)
    assert out.returncode == 0 and json.loads(out.stdout.splitlines()[-1])["receipts_verified_with_the_elf"] == 1, out.stdout + out.stderr
    assert len(open(entry.term_names_path("trace")).read().split()) == 302
