"""The segment-proof sequencer (csrc/prover.hip) seen from outside: the phases it marks, what a proof in flight holds on the device
and gives back at r0h_proof_shrink, and what r0h_last_profile reports between proofs.  Circuit `small` at 2^10 rows: one FRI round
plus the final polynomial, every group and tree path.  A committed group of `count` columns of N rows holds N * (20 * count + 256)
bytes: 4 * count * N of coefficients, 16 * count * N of evaluations on the 4N coset, 2 * 4N * 32 of Merkle nodes."""
import ctypes
import math

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import circuit_path

pytestmark = pytest.mark.gpu
PO2, SEED = 10, 31
N = 1 << PO2
PHASES = ["transcript_seed", "commit_code", "commit_data", "accum", "commit_accum", "eval_check", "commit_check", "evaluate_at_z",
          "mix_combos", "deep_divide", "fri_commit", "queries"]
PHASES_SHRUNK = PHASES[:4] + ["evaluate_data_again"] + PHASES[4:]


def group_bytes(count):
    return N * (20 * count + 256)


@pytest.fixture(scope="module")
def blob():
    return np.fromfile(circuit_path("small"), dtype=np.uint32)


@pytest.fixture(scope="module")
def oracle_seal(orc, blob):
    oc = orc.circuit(blob)
    ocode, odata, oglob = oc.witgen(PO2, seed=SEED)
    return oc.prove(PO2, ocode, odata, oglob)


def check_profile(profile, names):
    assert [n for n, _ in profile] == names
    assert all(math.isfinite(ms) and ms >= 0 for _, ms in profile), profile


def test_phase_names_in_both_forms(hal, blob, oracle_seal):
    gc = hal.load_circuit(blob, entry.code_object_path("small"))
    code, data, glob_ = hal.witgen(gc, PO2, SEED)
    cc = hal.code_commit(gc, PO2)
    for form in (code, cc):
        assert np.array_equal(hal.prove_segment(gc, PO2, form, data, glob_), oracle_seal)
        check_profile(hal.last_profile(), PHASES)
    cc.free()
    for b in (code, data):
        b.free()
    gc.free()


@pytest.mark.parametrize("committed", [False, True], ids=["columns", "committed"])
def test_shrink_and_resident_bytes(hal, blob, oracle_seal, committed):
    L = r0.lib()
    gc = hal.load_circuit(blob, entry.code_object_path("small"))
    n_code, n_data = gc.group_size[r0.GROUP_CODE], gc.group_size[r0.GROUP_DATA]
    code, data, glob_ = hal.witgen(gc, PO2, SEED)
    cc = hal.code_commit(gc, PO2) if committed else None
    assert np.array_equal(hal.prove_segment(gc, PO2, cc if committed else code, data, glob_), oracle_seal)

    proof, mix = hal.proof_begin(gc, PO2, cc if committed else code, data, glob_)
    resident = group_bytes(n_data) + (0 if committed else group_bytes(n_code))
    assert L.r0h_proof_resident_bytes(proof) == resident
    freed = ctypes.c_size_t(0)
    r0._check(L.r0h_proof_shrink(proof, ctypes.byref(freed)))
    assert freed.value == 16 * n_data * N
    assert L.r0h_proof_resident_bytes(proof) == resident - 16 * n_data * N
    r0._check(L.r0h_proof_shrink(proof, ctypes.byref(freed)))
    assert freed.value == 0
    assert L.r0h_proof_resident_bytes(proof) == resident - 16 * n_data * N
    accum = hal.accum(gc, PO2, code, data, mix)
    assert np.array_equal(hal.proof_finish(proof, accum), oracle_seal)
    check_profile(hal.last_profile(), PHASES_SHRUNK)
    if committed:
        cc.free()
    for b in (code, data, accum):
        b.free()
    gc.free()


def test_profile_between_proofs(blob, oracle_seal):
    """r0h_last_profile reports the last profile that was closed: nothing on a fresh context, and a proof in flight or aborted leaves
    what it reports alone.  (Before the profile moved to ctx.cpp the names were those of the proof in flight and the times, sized only
    at a close, could be fewer -- on a fresh context none, behind a count of three.)"""
    fresh = r0.Hal(0)
    gc = fresh.load_circuit(blob, entry.code_object_path("small"))
    code, data, glob_ = fresh.witgen(gc, PO2, SEED)
    assert fresh.last_profile() == []
    proof, _ = fresh.proof_begin(gc, PO2, code, data, glob_)
    assert fresh.last_profile() == []
    fresh.proof_abort(proof)
    assert np.array_equal(fresh.prove_segment(gc, PO2, code, data, glob_), oracle_seal)
    closed = fresh.last_profile()
    check_profile(closed, PHASES)
    proof, _ = fresh.proof_begin(gc, PO2, code, data, glob_)
    assert fresh.last_profile() == closed
    fresh.proof_abort(proof)
    assert fresh.last_profile() == closed
    for b in (code, data):
        b.free()
    gc.free()
    fresh.close()
