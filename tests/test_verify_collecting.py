"""The collecting verifier without a GPU (r0h_verify_seals_on with ctx == NULL: csrc/verify.cpp records every Merkle opening instead of
hashing it, hashes the batch afterwards -- here on the host -- and compares): verdict and reason must be the immediate verifier's
(r0h_verify_seal) for the untouched golden seal and for one mutation of every kind, the seal order must decide between two faults,
and a batch must keep its seals apart."""
import os

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path
from verify_mutations import mutations, regions

GOLDEN = os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy")
# what a mutation must come to whatever else the seal holds (Poseidon2): read off csrc/verify.cpp, not off a run
PINNED = {"untouched": 0, "leaf value, group tree": 3, "leaf value, FRI tree": 5, "path digest, group tree": 3, "path digest, FRI tree": 5,
          "non-canonical sibling": 9, "non-canonical leaf value": 3, "coeff_u word": 4, "truncation inside an opening": 1, "one extra word": 8,
          "two faults: path digest in query 3, FRI value in query 1": 5}


@pytest.fixture(scope="module")
def blob():
    return np.fromfile(circuit_path("tiny"), dtype=np.uint32)


@pytest.fixture(scope="module")
def cases(blob):
    return mutations(blob, np.load(GOLDEN))


def test_the_layout_the_mutations_rest_on_is_the_seals():
    """a check of the helper (tests/verify_mutations.py), not of the feature: it passes wherever the golden seal's layout is this one"""
    seal = np.load(GOLDEN)
    r = regions(np.fromfile(circuit_path("tiny"), dtype=np.uint32), seal)
    assert r["words"] == seal.size and r["po2"] == 9 and r["fri"] == ["fri0"]


def test_verdict_and_reason_are_the_immediate_verifiers_for_every_kind_of_mutation(blob, cases):
    assert len(cases) == 14
    for label, seal in cases:
        want = r0.verify_seal(blob, seal)
        got = r0.verify_seals(blob, [seal])[0]
        assert got[:3] == want, "%s: collecting %r, immediate %r" % (label, got[:3], want)
        if label in PINNED:
            assert got[0] == PINNED[label], (label, got)
        assert (got[0] == 0) == (label == "untouched"), (label, got)


def test_two_faults_are_settled_in_seal_order(blob, cases):
    """a path digest in query 3 (group tree: 3) and a FRI value in query 1 (FRI tree: 5): the immediate verifier reports the first
    failing query, so the collecting one must not report the first failing tree, or the first job of the batch's sorted order"""
    label, seal = cases[-1]
    assert label.startswith("two faults")
    assert r0.verify_seals(blob, [seal])[0][:2] == r0.verify_seal(blob, seal)[:2] == (5, "fri merkle path rejected")
    only_q3 = dict(cases)["path digest, group tree"]
    assert r0.verify_seals(blob, [only_q3])[0][0] == 3


def test_a_batch_keeps_its_seals_apart(blob, cases):
    good, broken = cases[0][1], dict(cases)["path digest, FRI tree"]
    got = r0.verify_seals(blob, [good, broken, good])
    assert [g[:2] for g in got] == [(0, "ok"), (5, "fri merkle path rejected"), (0, "ok")]
    assert [g[2] for g in got] == [9, 9, 9]
    # seals of different lengths in one batch: the cut one is its own verdict, its neighbours are untouched by it
    cut = dict(cases)["truncation inside an opening"]
    got = r0.verify_seals(blob, [cut, good, cases[-2][1]])
    assert [g[0] for g in got] == [1, 0, 8]
    assert r0.verify_seals(blob, []) == []


def test_every_mutation_in_one_batch_gets_the_verdict_it_gets_alone(blob, cases):
    """14 seals in one batch (their openings share one hashing pass), three times over"""
    alone = [r0.verify_seal(blob, seal) for _, seal in cases]
    for _ in range(3):
        got = r0.verify_seals(blob, [seal for _, seal in cases])
        assert [g[:3] for g in got] == alone


def test_roots_and_bound_verification_are_r0h_verify_seal_roots(blob, cases):
    good = cases[0][1]
    root = r0.seal_code_root(blob, good)
    other = root.copy()
    other[0] = (int(other[0]) + 1) % 2013265921
    got = r0.verify_seals(blob, [good, good], code_roots=[root, other])
    assert got[0][:2] == r0.verify_seal(blob, good, code_root=root)[:2] == (0, "ok")
    assert got[1][:2] == r0.verify_seal(blob, good, code_root=other)[:2] == (10, "code root is not the expected control root")
    # the DATA root is the one the immediate form recomputes
    want = np.zeros(8, dtype=np.uint32)
    verdict, po2 = r0._c.c_int(-1), r0._u32(0)
    b, s = np.ascontiguousarray(blob), np.ascontiguousarray(good)
    r0._check(r0.lib().r0h_verify_seal_roots(b.ctypes.data, b.size, s.ctypes.data, s.size, None, r0.ctypes.byref(verdict), r0.ctypes.byref(po2), want.ctypes.data))
    assert verdict.value == 0 and want.any() and np.array_equal(got[0][3], want)
    with pytest.raises(r0.R0HipError, match="not canonical"):
        r0.verify_seals(blob, [good], code_roots=[np.full(8, 2013265921, np.uint32)])
    with pytest.raises(r0.R0HipError, match="circuit blob"):
        r0.verify_seals(np.zeros(8, np.uint32), [good])
