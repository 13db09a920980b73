"""r0h_hash_fold_top and r0h_ctx_set_merkle_fused_tops: the levels of up to 8192 parents of a Merkle tree built by merkle_subtree_kernel
in at most two launches (csrc/merkle.hip, the plan in csrc/merkle_fused_plan.hpp) instead of one launch of r0h_hash_fold per level.  The
switch changes launches and nothing else, so everything here is equality, word for word, between the switch on and the switch off --
node buffers of every tree shape from 1 row to 2^15 under both suites (and against the oracle / the SHA-256 restatement where those are
quick), the entry point alone against the loop of hash_fold at the sizes where the plan changes shape, another Poseidon2 table, seals in
the three forms of a proof, a session's receipt with the image proof and with an evicted segment replayed from its tree top, a lift and
a join -- plus the launch counts that say the fused kernel is what ran.

The split is 2^7: 128 workgroups fold down to the level of 128 nodes, one workgroup from there; a top of at most 7 levels (64
parents) is one launch."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
import sha_suite_ref
from conftest import circuit_path
from hyperfridge_r0_amd import recursion
from test_gpu_p2_dot_schedule import DIAG, RC, UNCOVERED
from test_gpu_session_enqueue import PO2 as SESSION_PO2, Run

pytestmark = pytest.mark.gpu
SUITES = ["poseidon2", "sha-256"]
SPLIT = 7                       # MERKLE_FUSED_SPLIT
FILL = 0xC3C3C3C3               # what words nobody may write hold
FOLD_KERNEL = {"poseidon2": "hash_fold_kernel", "sha-256": "sha256_hash_fold_kernel"}          # r0h_hash_fold's family (both its forms)
SUBTREE_KERNEL = {"poseidon2": "merkle_subtree_kernel", "sha-256": "sha256_merkle_subtree_kernel"}


@pytest.fixture(scope="module")
def hals():
    """a context per suite, the switch off on both"""
    hs = {}
    for suite in SUITES:
        hs[suite] = r0.Hal(0)
        hs[suite].set_hashfn(suite)
        hs[suite].set_merkle_fused_tops(False)
    yield hs
    for h in hs.values():
        h.close()


def words(suite, seed, n):
    rng = np.random.default_rng(seed)
    if suite == "poseidon2":
        return rng.integers(0, r0.P, size=n, dtype=np.uint32)
    return rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)


def build(h, on, m, rows, cols):
    """merkle_build into a buffer of 2 * rows digests and 64 words more, all FILL before -> every word of it"""
    h.set_merkle_fused_tops(on)
    try:
        nodes, matrix = h.copy_from(np.full(2 * rows * 8 + 64, FILL, np.uint32)), h.copy_from(m)
        h.merkle_build(nodes, matrix, rows, cols)
        out = nodes.to_host()
        nodes.free(), matrix.free()
        return out
    finally:
        h.set_merkle_fused_tops(False)


# ---- 1. every tree shape
@pytest.mark.parametrize("cols", [1, 17])
@pytest.mark.parametrize("k", range(16))
@pytest.mark.parametrize("suite", SUITES)
def test_a_tree_has_the_same_nodes_with_the_switch_on(hals, orc, suite, k, cols):
    h, rows = hals[suite], 1 << k
    m = words(suite, 1000 * k + cols, rows * cols)
    off, on = build(h, False, m, rows, cols), build(h, True, m, rows, cols)
    assert np.array_equal(on, off)
    assert (on[:8] == FILL).all() and (on[2 * rows * 8:] == FILL).all() and len(on) == 2 * rows * 8 + 64     # node 0, and behind the tree
    assert not (on[8:2 * rows * 8] == FILL).any()
    if suite == "poseidon2" and k <= 10:
        assert np.array_equal(on[8:2 * rows * 8], orc.merkle_build(m, rows, cols)[8:])
    if suite == "sha-256" and k <= 8:
        assert np.array_equal(on[8:2 * rows * 8], sha_suite_ref.merkle_build(m, rows, cols)[8:])


# ---- 2. the entry point alone
@pytest.mark.parametrize("output_size", [1, 2, 1 << (SPLIT - 1), 1 << SPLIT, 1 << (SPLIT + 1), 8192])
@pytest.mark.parametrize("suite", SUITES)
def test_hash_fold_top_is_the_loop_of_hash_fold(hals, suite, output_size):
    h = hals[suite]
    host = np.full(4 * output_size * 8 + 64, FILL, np.uint32)
    host[2 * output_size * 8:4 * output_size * 8] = words(suite, output_size, 2 * output_size * 8)
    loop, top = h.copy_from(host), h.copy_from(host)
    sz = output_size
    while sz >= 1:
        h.hash_fold(loop, sz)
        sz //= 2
    h.hash_fold_top(top, output_size)
    got, want = top.to_host(), loop.to_host()
    assert np.array_equal(got, want)
    assert (got[:8] == FILL).all() and (got[4 * output_size * 8:] == FILL).all() and np.array_equal(got[2 * output_size * 8:], host[2 * output_size * 8:])
    loop.free(), top.free()


@pytest.mark.parametrize("suite", SUITES)
def test_what_hash_fold_top_does_nothing_for_and_what_it_refuses(hals, suite):
    h = hals[suite]
    host = np.full(4 * 16 * 8 + 8, FILL, np.uint32)
    nodes = h.copy_from(host)
    h.hash_fold_top(nodes, 0)
    assert np.array_equal(nodes.to_host(), host)
    for bad in (3, 16384, 8192 + 4096):
        with pytest.raises(r0.R0HipError, match="r0h_hash_fold_top: output_size %d is not a power of two up to 8192" % bad):
            h.hash_fold_top(nodes, bad)
    with pytest.raises(r0.R0HipError, match="r0h_hash_fold_top: output_size 32 needs 4096 bytes of nodes"):
        h.hash_fold_top(nodes, 32)
    with pytest.raises(r0.R0HipError, match="r0h_hash_fold_top: node buffer must be 16-byte aligned"):
        h.hash_fold_top(nodes.slice(1, 4 * 16 * 8), 16)
    with pytest.raises(r0.R0HipError, match="r0h_hash_fold_top: NULL argument"):
        r0._check(r0.lib().r0h_hash_fold_top(h.ctx, None, 16))
    assert np.array_equal(nodes.to_host(), host)          # a refusal wrote nothing
    nodes.free()


# ---- 3. another constants table: the lanes form reads the table the context holds, under the safe schedule's kernels for the rest
def test_a_table_the_tight_schedule_does_not_cover(hals):
    h, rows, cols = hals["poseidon2"], 1 << 15, 17
    m = words("poseidon2", 3, rows * cols)
    default = build(h, True, m, rows, cols)
    try:
        h.poseidon2_set_consts(np.array(RC, np.uint32), np.array(UNCOVERED, np.uint32))
        assert h.poseidon2_dot_schedule() == "safe"
        off, on = build(h, False, m, rows, cols), build(h, True, m, rows, cols)
    finally:
        h.poseidon2_set_consts(np.array(RC, np.uint32), np.array(DIAG, np.uint32))
    assert np.array_equal(on, off) and not np.array_equal(on[8:16], default[8:16])
    assert np.array_equal(build(h, True, m, rows, cols), default)


# ---- 4. launch counts.  r0h_kernel_stats files both forms of r0h_hash_fold -- hash_fold_kernel and, under Poseidon2 up to 8192
# parents, hash_fold_lanes_kernel -- under the suite's fold family: a tree of 2^15 leaves is 15 launches of it, the level of 16384
# parents and the fourteen below.
def launches(h, on, rows=1 << 15, cols=3):
    m = words(h.hashfn, 4, rows * cols)
    h.kernel_timing(True)
    try:
        build(h, on, m, rows, cols)
        return {name: st["launches"] for name, st in h.kernel_stats().items()}
    finally:
        h.kernel_timing(False)


@pytest.mark.parametrize("suite", SUITES)
def test_the_fourteen_launches_become_two(hals, suite):
    h = hals[suite]
    off, on = launches(h, False), launches(h, True)
    print(suite, "off", off, "on", on)
    assert off.get(FOLD_KERNEL[suite], 0) == 1 + 14 and off.get(SUBTREE_KERNEL[suite], 0) == 0
    assert on.get(FOLD_KERNEL[suite], 0) == 1                      # the level of 16384 parents; none of the fourteen
    assert on.get("hash_fold_lanes_kernel", 0) == 0
    assert 1 <= on.get(SUBTREE_KERNEL[suite], 0) <= 2
    small = launches(h, True, rows=1 << SPLIT)                     # 64 parents: one workgroup, one launch
    assert small.get(FOLD_KERNEL[suite], 0) == 0 and small.get(SUBTREE_KERNEL[suite], 0) == 1


def test_the_environment_sets_the_default_and_the_context_overrides_it():
    h = r0.Hal(0)       # a context that was never told
    m = words("poseidon2", 5, (1 << 15) * 2)

    def count():
        nodes, matrix = h.alloc(2 * (1 << 15) * 8), h.copy_from(m)
        h.kernel_timing(True)
        h.merkle_build(nodes, matrix, 1 << 15, 2)
        st = h.kernel_stats()
        h.kernel_timing(False)
        nodes.free(), matrix.free()
        return st["hash_fold_kernel"]["launches"]
    try:
        assert count() == 15
        os.environ["R0H_MERKLE_FUSED_TOPS"] = "1"
        assert count() == 1
        h.set_merkle_fused_tops(False)
        assert count() == 15
        del os.environ["R0H_MERKLE_FUSED_TOPS"]
        h.set_merkle_fused_tops(True)
        assert count() == 1
    finally:
        os.environ.pop("R0H_MERKLE_FUSED_TOPS", None)
        h.close()


# ---- 5. whole proofs
@pytest.mark.parametrize("form", ["host transcript", "device transcript", "device finish"])
@pytest.mark.parametrize("name,po2", [("tiny", 9), ("small", 12)])
@pytest.mark.parametrize("suite", SUITES)
def test_a_seal_is_the_same_with_the_switch_on(hals, suite, name, po2, form):
    h = hals[suite]
    blob = np.fromfile(circuit_path(name), dtype=np.uint32)
    gc = h.load_circuit(blob, None if name == "tiny" else entry.code_object_path(name))
    h.set_device_transcript(form == "device transcript")
    h.set_device_finish(form == "device finish")
    seals = {}
    try:
        for on in (False, True):
            h.set_merkle_fused_tops(on)
            code, data, glob = h.witgen(gc, po2, 1)
            seals[on] = h.prove_segment(gc, po2, code, data, glob)
            code.free(), data.free()
    finally:
        h.set_merkle_fused_tops(False)
        h.set_device_transcript(False)
        h.set_device_finish(False)
        gc.free()
    assert np.array_equal(seals[True], seals[False])
    assert r0.verify_seal(blob, seals[True], hashfn=suite)[:3] == (0, "ok", po2)


@pytest.fixture(scope="module")
def run(hal):
    hal.set_merkle_fused_tops(False)
    r = Run(hal)
    yield r
    r.close()


def prove_session(run, on, **kw):
    run.hal.set_merkle_fused_tops(on)
    try:
        return run.prove(False, image=True, **kw)
    finally:
        run.hal.set_merkle_fused_tops(False)


def test_a_session_gives_the_same_receipt_with_the_switch_on(run):
    want_json, want_id, n = run.reference(True)               # the switch off
    assert n >= 3
    receipt, image_id, _, _ = prove_session(run, True)
    assert receipt.to_json() == want_json and image_id == want_id
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")
    assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")
    assert run.hal.session_held_bytes() == 0


def test_an_evicted_segment_replayed_from_its_tree_top_gives_the_same_receipt(run):
    want_json, want_id, _ = run.reference(True)
    _, _, _, roomy = prove_session(run, True, limit=1 << 50)  # (a limit nothing reaches: the count is kept)
    receipt, image_id, _, dev = prove_session(run, True, limit=roomy["peak_counted_bytes"] - 1, tops=6)
    assert dev["evicted"] == dev["replayed"] == 1 and run.hal.last_session_tree_tops()["replayed_from_top"] == 1
    assert receipt.to_json() == want_json and image_id == want_id
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")
    assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")
    assert run.hal.session_held_bytes() == 0
    assert SESSION_PO2 == 16


def test_a_lift_and_a_join_give_the_same_nodes_with_the_switch_on(hal):
    hal.set_merkle_fused_tops(False)
    seg_blob, rec_blob = np.fromfile(circuit_path("small"), dtype=np.uint32), np.fromfile(circuit_path("recursion"), dtype=np.uint32)
    seg, po2 = hal.load_circuit(seg_blob, entry.code_object_path("small")), 12
    claims, _ = r0.session_claims(2, r0.serde_encode_str('{"segments":2}'))
    seals = []
    for k in range(2):
        code, data, glob = hal.witgen(seg, po2, 1000 + k, globals_in=claims[k].globals())
        seals.append(hal.prove_segment(seg, po2, code, data, glob))
        code.free(), data.free()
    rec = recursion.Recursor(hal, rec_blob, seg_blob, entry.code_object_path("recursion"), po2=16)
    nodes = {}
    try:
        for on in (False, True):
            hal.set_merkle_fused_tops(on)
            lifted = [rec.lift(seals[k], claims[k]) for k in range(2)]
            nodes[on] = lifted + [rec.join(lifted[0], lifted[1])]
    finally:
        hal.set_merkle_fused_tops(False)
    for a, b in zip(nodes[True], nodes[False]):
        assert np.array_equal(a.seal, b.seal) and bytes(a.claim) == bytes(b.claim)
        assert rec.verify(a)
    rec.close()
    seg.free()
