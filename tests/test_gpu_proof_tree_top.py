"""A proof begun from the top of its DATA tree (r0h_proof_data_top, r0h_proof_begin_committed_top): DATA is interpolated and evaluated,
no tree is built, and the seal is word for word the one of the hashing path.  Circuit `tiny` at 2^9 rows: a 2^11-row domain, six path
digests, so levels 1 .. 6 fit and 6 -- one wave per query -- is the most."""
import ctypes
import os

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

pytestmark = pytest.mark.gpu
PO2 = 9
DOMAIN = 4 << PO2
GOLDEN = os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy")


@pytest.fixture(scope="module")
def blob():
    return np.fromfile(circuit_path("tiny"), dtype=np.uint32)


@pytest.fixture(scope="module")
def sha():
    h = r0.Hal(0)
    h.set_hashfn("sha-256")
    yield h
    h.close()


def through_the_top(h, gc, seed, levels, shrink=False, witness_seed=None):
    """begin, take the top, abort; begin again from the top (the witness of `witness_seed`, if another), accumulate, finish"""
    code, data, glob = h.witgen(gc, PO2, seed)
    cc = h.code_commit(gc, PO2)
    bufs = [code, data]
    try:
        proof, _ = h.proof_begin(gc, PO2, cc, data, glob)
        plain_bytes = r0.lib().r0h_proof_resident_bytes(proof)
        top = h.proof_data_top(proof, PO2, levels)
        bufs.append(top)
        h.proof_abort(proof)
        assert top.words == 8 * ((2 * DOMAIN) >> levels)
        if witness_seed is not None:
            other_code, data, glob = h.witgen(gc, PO2, witness_seed)  # (a witness consistent in itself: only the top is foreign)
            bufs += [other_code, data]
        proof, mix = h.proof_begin(gc, PO2, cc, data, glob, top=(top, levels))
        # what the proof holds: as before, less the bottom levels of the DATA tree
        assert plain_bytes - r0.lib().r0h_proof_resident_bytes(proof) == 32 * (2 * DOMAIN - ((2 * DOMAIN) >> levels))
        if shrink:
            freed = ctypes.c_size_t(0)
            r0._check(r0.lib().r0h_proof_shrink(proof, ctypes.byref(freed)))
            assert freed.value == 16 * gc.group_size[r0.GROUP_DATA] << PO2
        accum = h.accum(gc, PO2, code, data, mix)
        bufs.append(accum)
        return h.proof_finish(proof, accum)  # consumed, whatever comes of it
    finally:
        cc.free()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("levels,shrink", [(6, False), (1, False), (6, True), (3, True)])
def test_the_seal_is_the_golden_one(hal, blob, levels, shrink):
    gc = hal.load_circuit(blob)
    assert np.array_equal(through_the_top(hal, gc, 1, levels, shrink), np.load(GOLDEN))
    gc.free()


@pytest.mark.parametrize("levels", [6, 1])
def test_under_sha256_the_seal_is_prove_segments(sha, blob, levels):
    gc = sha.load_circuit(blob)
    code, data, glob = sha.witgen(gc, PO2, 1)
    want = sha.prove_segment(gc, PO2, code, data, glob)
    assert r0.verify_seal(blob, want, hashfn="sha-256")[:2] == (0, "ok") and not np.array_equal(want, np.load(GOLDEN))
    assert np.array_equal(through_the_top(sha, gc, 1, levels), want)
    assert np.array_equal(through_the_top(sha, gc, 1, levels, shrink=True), want)
    for b in (code, data):
        b.free()
    gc.free()


def test_a_top_of_another_witness_fails_the_proof_and_leaves_the_context_usable(hal, blob):
    gc = hal.load_circuit(blob)
    with pytest.raises(r0.R0HipError, match=r"r0h_proof_finish: tree top does not match the matrix under query \d+ \(row \d+\)"):
        through_the_top(hal, gc, 1, 6, witness_seed=2)
    code, data, glob = hal.witgen(gc, PO2, 1)
    assert np.array_equal(hal.prove_segment(gc, PO2, code, data, glob), np.load(GOLDEN))
    assert np.array_equal(through_the_top(hal, gc, 1, 6), np.load(GOLDEN))
    for b in (code, data):
        b.free()
    gc.free()


def test_levels_outside_the_tree_are_refused_by_name(hal, blob):
    gc = hal.load_circuit(blob)
    code, data, glob = hal.witgen(gc, PO2, 1)
    cc = hal.code_commit(gc, PO2)
    proof, _ = hal.proof_begin(gc, PO2, cc, data, glob)
    top = hal.alloc(2 * DOMAIN * 8)
    for levels in (0, 7, 9):
        with pytest.raises(r0.R0HipError, match=r"r0h_proof_data_top: levels %d outside \[1, 6\]" % levels):
            hal.proof_data_top(proof, PO2, levels, top)
    hal.proof_data_top(proof, PO2, 6, top)
    hal.proof_abort(proof)
    for levels, text in ((0, r"r0h_proof_begin_committed_top: levels 0 outside \[1, 8\]"), (9, r"r0h_proof_begin_committed_top: levels 9 outside \[1, 8\]"),
                         (7, r"r0h_proof_begin_committed_top: levels 7 outside \[1, 6\]")):
        with pytest.raises(r0.R0HipError, match=text):
            hal.proof_begin(gc, PO2, cc, data, glob, top=(top, levels))
    with pytest.raises(r0.R0HipError, match="takes a CodeCommit"):
        hal.proof_begin(gc, PO2, code, data, glob, top=(top, 6))
    proof, mix = hal.proof_begin(gc, PO2, cc, data, glob, top=(top, 6))
    accum = hal.accum(gc, PO2, code, data, mix)
    assert np.array_equal(hal.proof_finish(proof, accum), np.load(GOLDEN))
    cc.free()
    for b in (code, data, top, accum):
        b.free()
    gc.free()
