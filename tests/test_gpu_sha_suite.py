"""The SHA-256 hash suite on the device: kernels, seals, refusals and suite state, all held to the Python restatement
(tests/sha_suite_ref.py) by exact equality.  The field side of a proof does not depend on the suite and stays pinned by the
oracle parity tests; what the suite changes -- leaf and pair hashing, top layers, the commit order, the generator, the query
positions -- is recomputed here by the restatement's transcript replayer from the seal alone."""
import os

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
import sha_suite_ref as ref
from conftest import ROOT, circuit_path

pytestmark = pytest.mark.gpu

SHA = "sha-256"


@pytest.fixture(scope="module")
def sha():
    """a context of its own on the SHA-256 suite (the session-wide `hal` fixture stays on Poseidon2)"""
    h = r0.Hal(0)
    h.set_hashfn(SHA)
    assert h.hashfn == SHA
    yield h
    h.close()


def _blob(name):
    return np.fromfile(circuit_path(name), dtype=np.uint32)


def _load(h, name):
    co = entry.code_object_path(name)
    return h.load_circuit(_blob(name), co if name != "tiny" else None)


def _words(rng, n):
    return rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 4096])
def test_hash_rows_equals_the_reference(sha, rows):
    rng = np.random.default_rng(rows)
    for cols in (0, 1, 15, 16, 17, 40, 128):
        m = _words(rng, rows * cols)
        matrix, digests = sha.copy_from(m), sha.alloc(rows * 8)
        sha.hash_rows(digests, matrix, rows, cols)
        got = digests.to_host().reshape(rows, 8)
        assert np.array_equal(got, ref.hash_rows(m, rows, cols)), (rows, cols)
        matrix.free(); digests.free()


def test_hash_fold_and_merkle_build_equal_the_reference(sha):
    rng = np.random.default_rng(77)
    for out in (1, 2, 64, 255, 8192, 16384):
        host = _words(rng, 4 * out * 8)
        nodes = sha.copy_from(host)
        sha.hash_fold(nodes, out)
        assert np.array_equal(nodes.to_host(), ref.hash_fold(host, out)), out
        nodes.upload(host)
        sha.hash_fold_io(nodes, 2 * out, out)
        assert np.array_equal(nodes.to_host(), ref.hash_fold(host, out)), out
        nodes.free()
    n = sha.alloc(64)
    with pytest.raises(r0.R0HipError, match="2 \\* output_size"):
        sha.hash_fold_io(n, 3, 2)
    n.free()
    for rows, cols in ((2, 3), (1024, 17), (4096, 64)):
        m = _words(rng, rows * cols)
        matrix, nodes = sha.copy_from(m), sha.alloc(2 * rows * 8)
        sha.zero(nodes)
        sha.merkle_build(nodes, matrix, rows, cols)
        assert np.array_equal(nodes.to_host()[8:], ref.merkle_build(m, rows, cols)[8:]), (rows, cols)
        matrix.free(); nodes.free()


# ---------------------------------------------------------------- seals
def _prove_all_ways(h, gc, po2, seed):
    code, data, glob = h.witgen(gc, po2, seed)
    seal = h.prove_segment(gc, po2, code, data, glob)
    cc = h.code_commit(gc, po2)
    assert np.array_equal(h.prove_segment(gc, po2, cc, data, glob), seal), "r0h_prove_segment_committed gives another seal"
    proof, mix = h.proof_begin(gc, po2, code, data, glob)
    accum = h.accum(gc, po2, code, data, mix)
    assert np.array_equal(h.proof_finish(proof, accum), seal), "r0h_proof_begin / r0h_proof_finish give another seal"
    root = cc.root()
    assert np.array_equal(root, h.code_root(gc, po2))
    for b in (code, data, accum):
        b.free()
    cc.free()
    return seal, root


@pytest.mark.parametrize("name,po2", [("tiny", 9), ("tiny", 12), ("small", 14), ("bench", 18)])
def test_sha256_seal_verifies_and_the_replayer_recomputes_every_opening(sha, name, po2):
    blob = _blob(name)
    gc = _load(sha, name)
    seal, root = _prove_all_ways(sha, gc, po2, seed=3)
    gc.free()
    assert r0.verify_seal(blob, seal, code_root=root, hashfn=SHA) == (0, "ok", po2)
    assert r0.verify_seal(blob, seal, hashfn=SHA) == (0, "ok", po2)
    if po2 <= 14:
        assert np.array_equal(r0.control_root_host(blob, po2, hashfn=SHA), root)
    t = ref.replay_seal(blob, seal)
    n_rounds = len(t["fri_mix"])
    print("replayed %s po2 %d: %d of %d openings, %d of %d words" % (name, po2, t["openings_ok"], t["openings_total"], t["words"], t["seal_words"]))
    assert t["po2"] == po2 and t["words"] == t["seal_words"] == seal.size
    assert t["openings_total"] == ref.QUERIES * (4 + n_rounds) and n_rounds >= 1
    assert t["openings_ok"] == t["openings_total"], "first opening the restatement cannot recompute: %r" % (t["first_bad"],)
    assert np.array_equal(t["roots"][0], root)  # the CODE commitment is the control root
    # the other suite's verifier refuses it with a verdict (no error, no crash), and so does a verifier bound to another root
    verdict, reason, _ = r0.verify_seal(blob, seal)
    assert verdict != 0 and reason != "ok"
    other = root.copy(); other[3] ^= 1
    assert r0.verify_seal(blob, seal, code_root=other, hashfn=SHA)[0] == 10


def test_poseidon2_seal_is_refused_by_the_sha256_verifier(hal):
    blob = _blob("tiny")
    gc = hal.load_circuit(blob)
    code, data, glob = hal.witgen(gc, 9, 1)
    seal = hal.prove_segment(gc, 9, code, data, glob)
    assert r0.verify_seal(blob, seal)[:2] == (0, "ok") and r0.verify_seal(blob, seal, hashfn="poseidon2")[:2] == (0, "ok")
    verdict, reason, _ = r0.verify_seal(blob, seal, hashfn=SHA)
    assert verdict != 0 and reason != "ok"
    for b in (code, data):
        b.free()
    gc.free()


def test_tamper_matrix(sha):
    """one flipped word in each region of the seal: every one is refused"""
    name, po2 = "small", 10
    blob = _blob(name)
    gc = _load(sha, name)
    code, data, glob = sha.witgen(gc, po2, 9)
    seal = sha.prove_segment(gc, po2, code, data, glob)
    for b in (code, data):
        b.free()
    gc.free()
    assert r0.verify_seal(blob, seal, hashfn=SHA) == (0, "ok", po2)
    t = ref.replay_seal(blob, seal)
    reg = t["regions"]
    assert t["openings_ok"] == t["openings_total"]
    spots = {"public input": reg["globals"][0] + 1}
    for g in ("code", "data", "accum", "check"):
        spots["top-layer digest of " + g] = reg[g + "_top"][0] + 8 * 3 + 2
    spots["coeff_u word"] = reg["coeff_u"][0] + 5
    spots["fri round top"] = reg["fri0_top"][0] + 9
    spots["final coefficient"] = reg["final"][0] + 7
    by_tree = {}
    for tree, q, start, path, end in reg["opening"]:
        by_tree.setdefault(tree, (q, start, path, end))
    for tree in ("accum", "code", "data", "check", "fri0"):
        q, start, path, end = by_tree[tree]
        assert end > path > start
        spots["opened value of " + tree] = start
        spots["path digest of " + tree] = path + 3
    assert len(spots) == 18
    for what, at in spots.items():
        bad = seal.copy()
        bad[at] ^= 1
        verdict, reason, _ = r0.verify_seal(blob, bad, hashfn=SHA)
        assert verdict != 0, "a flipped %s (word %d) was accepted" % (what, at)
        if "digest" in what or "top" in what or "opened" in what:
            assert ref.replay_seal(blob, bad)["openings_ok"] < t["openings_total"], what  # the restatement sees it too
    # high bits: a digest word is any 32-bit value under this suite, the flip is refused for what it does to the tree, not as "not canonical"
    bad = seal.copy()
    bad[reg["data_top"][0]] ^= 0x80000000
    assert r0.verify_seal(blob, bad, hashfn=SHA)[0] not in (0, 9)
    assert r0.verify_seal(blob, seal[:-1], hashfn=SHA)[0] == 1 and r0.verify_seal(blob, np.append(seal, np.uint32(0)), hashfn=SHA)[0] == 8


# ---------------------------------------------------------------- suite state
def test_switching_to_sha256_and_back_reproduces_the_frozen_poseidon2_seal():
    want = np.load(os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy"))
    h = r0.Hal(0)
    try:
        assert h.hashfn == "poseidon2"
        gc = h.load_circuit(_blob("tiny"))
        code, data, glob = h.witgen(gc, 9, 1)
        h.set_hashfn(SHA)
        other = h.prove_segment(gc, 9, code, data, glob)
        assert other.size == want.size and not np.array_equal(other, want)
        assert r0.verify_seal(_blob("tiny"), other, hashfn=SHA)[:2] == (0, "ok")
        with pytest.raises(r0.R0HipError, match="unknown hash function"):
            h.set_hashfn("blake2b")
        assert h.hashfn == SHA  # a refused name changes nothing
        h.set_hashfn("poseidon2")
        assert h.hashfn == "poseidon2"
        assert np.array_equal(h.prove_segment(gc, 9, code, data, glob), want)
        gc.free()
    finally:
        h.close()


def test_code_commit_and_proof_remember_their_suite():
    h = r0.Hal(0)
    try:
        gc = h.load_circuit(_blob("tiny"))
        code, data, glob = h.witgen(gc, 9, 4)
        cc_p2 = h.code_commit(gc, 9)
        h.set_hashfn(SHA)
        with pytest.raises(r0.R0HipError, match="poseidon2.*sha-256"):
            h.prove_segment(gc, 9, cc_p2, data, glob)
        with pytest.raises(r0.R0HipError, match="poseidon2.*sha-256"):
            h.proof_begin(gc, 9, cc_p2, data, glob)
        cc_sha = h.code_commit(gc, 9)
        assert not np.array_equal(cc_sha.root(), cc_p2.root())
        proof, mix = h.proof_begin(gc, 9, cc_sha, data, glob)
        accum = h.accum(gc, 9, code, data, mix)
        h.set_hashfn("poseidon2")
        with pytest.raises(r0.R0HipError, match="sha-256.*poseidon2"):
            h.prove_segment(gc, 9, cc_sha, data, glob)
        with pytest.raises(r0.R0HipError, match="begun under the sha-256"):
            h.proof_finish(proof, accum)  # (consumes the proof)
        seal = h.prove_segment(gc, 9, cc_p2, data, glob)
        assert r0.verify_seal(_blob("tiny"), seal, code_root=cc_p2.root())[:2] == (0, "ok")
        cc_p2.free(); cc_sha.free(); gc.free()
    finally:
        h.close()


def test_receipt_level_entry_points_refuse_a_sha256_context():
    from hyperfridge_r0_amd import recursion
    h = r0.Hal(0)
    try:
        tiny = h.load_circuit(_blob("tiny"))
        rec = recursion.Recursor(h, _blob("recursion"), _blob("small"), entry.code_object_path("recursion"), po2=16)
        node = recursion.Node.from_parts(np.zeros(64, dtype=np.uint32), r0.ReceiptClaim())
        h.set_hashfn(SHA)
        doc = "receipts, sessions, image proofs and recursion nodes are poseidon2 only"
        with pytest.raises(r0.R0HipError, match=doc):
            h.prove_elf(tiny, b"\x7fELF" + bytes(60), [0])
        with pytest.raises(r0.R0HipError, match=doc):
            h.session_begin(tiny, b"\x7fELF" + bytes(60), [0])
        with pytest.raises(r0.R0HipError, match=doc):
            h.prove_image(tiny, b"\x7fELF" + bytes(60), np.zeros(16, dtype=np.uint32))
        with pytest.raises(r0.R0HipError, match=doc):
            rec.lift(np.zeros(64, dtype=np.uint32), r0.ReceiptClaim())
        with pytest.raises(r0.R0HipError, match=doc):
            rec.join(node, node)
        with pytest.raises(r0.R0HipError, match=doc):
            recursion.Recursor(h, _blob("recursion"), _blob("small"), entry.code_object_path("recursion"), po2=16)
        h.set_hashfn("poseidon2")
        rec.close(); tiny.free()
    finally:
        h.close()


def test_cli_proves_and_verifies_a_sha256_seal(tmp_path):
    import subprocess
    prove, verify = (os.path.join(ROOT, "hyperfridge-r0_amd", n) for n in ("r0h_prove", "r0h_verify"))
    seal = str(tmp_path / "seal.bin")
    out = subprocess.run([prove, circuit_path("tiny"), "--po2", "10", "--hashfn", SHA, "--seal-out", seal, "--verify", "1"], capture_output=True, text=True)
    assert out.returncode == 0 and "seals verified" in out.stderr, out.stdout + out.stderr
    words = np.fromfile(seal, dtype=np.uint32)
    assert r0.verify_seal(_blob("tiny"), words, hashfn=SHA) == (0, "ok", 10)
    assert ref.replay_seal(_blob("tiny"), words)["first_bad"] is None
    ok = subprocess.run([verify, circuit_path("tiny"), seal, "--hashfn", SHA], capture_output=True, text=True)
    assert ok.returncode == 0 and '"accepted": true' in ok.stdout
    assert subprocess.run([verify, circuit_path("tiny"), seal], capture_output=True, text=True).returncode == 1
