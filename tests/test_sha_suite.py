"""The SHA-256 hash suite on the host (no GPU): the Python restatement (tests/sha_suite_ref.py) is pinned to hashlib, and the library's
host primitives, its host control root and its name handling are pinned to the restatement.  The Poseidon2 names of the same entry
points are pinned to the oracle."""
import hashlib
import os
import struct

import numpy as np
import pytest

import sha_suite_ref as ref
from conftest import ROOT, circuit_path

LENGTHS = (0, 1, 15, 16, 17, 33)


def _padded_block(msg):
    assert len(msg) <= 55
    return msg + b"\x80" + bytes(55 - len(msg)) + struct.pack(">Q", 8 * len(msg))


@pytest.mark.parametrize("msg", [b"", b"abc", b"Hello", b"World", bytes(range(55))])
def test_reference_compression_is_sha256(msg):
    block = _padded_block(msg)
    state = ref.compress(ref.IV, list(struct.unpack(">16I", block)))
    assert struct.pack(">8I", *state) == hashlib.sha256(msg).digest()
    # ... and the suite's word convention: the 64 bytes read as 16 little-endian input words, the digest's bytes in memory big-endian
    words = np.frombuffer(block, dtype="<u4")
    assert ref.hash_pair(words[:8], words[8:]).tobytes() == hashlib.sha256(msg).digest()
    assert ref.hash_elem_slice(words).tobytes() == hashlib.sha256(msg).digest()


def test_reference_vector_forms_agree_with_the_scalar_ones():
    rng = np.random.default_rng(11)
    for cols in (0, 1, 15, 16, 17, 40):
        m = rng.integers(0, 2**32, size=(cols, 5), dtype=np.uint64).astype(np.uint32)
        got = ref.hash_rows(m.reshape(-1), 5, cols)
        for r in range(5):
            assert np.array_equal(got[r], ref.hash_elem_slice(m[:, r])), (cols, r)
    nodes = rng.integers(0, 2**32, size=8 * 8, dtype=np.uint64).astype(np.uint32)
    folded = ref.hash_fold(nodes, 2).reshape(-1, 8)
    for i in (2, 3):
        assert np.array_equal(folded[i], ref.hash_pair(nodes.reshape(-1, 8)[2 * i], nodes.reshape(-1, 8)[2 * i + 1]))
    assert np.array_equal(ref.hash_elem_slice([]), np.array([ref.bswap(v) for v in ref.IV], dtype=np.uint32))


def test_host_primitives_equal_the_reference():
    import hyperfridge_r0_amd as r0
    rng = np.random.default_rng(5)
    for trial in range(4):
        for n in LENGTHS + (64, 100):
            w = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)  # any 32-bit words: not field elements
            assert np.array_equal(r0.hash_elems_host("sha-256", w), ref.hash_elem_slice(w)), n
        a, b = (rng.integers(0, 2**32, size=8, dtype=np.uint64).astype(np.uint32) for _ in range(2))
        assert np.array_equal(r0.hash_pair_host("sha-256", a, b), ref.hash_pair(a, b))
    assert np.array_equal(r0.hash_elems_host("sha-256", []), np.array([ref.bswap(v) for v in ref.IV], dtype=np.uint32))


def test_poseidon2_name_equals_the_oracle(orc):
    import hyperfridge_r0_amd as r0
    rng = np.random.default_rng(6)
    for n in LENGTHS:
        w = rng.integers(0, ref.P, size=n, dtype=np.uint64).astype(np.uint32)
        assert np.array_equal(r0.hash_elems_host("poseidon2", w), orc.hash_elem_slice(w)), n
    a, b = (rng.integers(0, ref.P, size=8, dtype=np.uint64).astype(np.uint32) for _ in range(2))
    assert np.array_equal(r0.hash_pair_host("poseidon2", a, b), orc.hash_pair(a, b))
    with pytest.raises(r0.R0HipError, match="canonical"):
        r0.hash_pair_host("poseidon2", a, np.full(8, ref.P, dtype=np.uint32))


@pytest.mark.parametrize("name,po2", [("tiny", 9), ("small", 10)])
def test_host_control_root_equals_the_reference_tree(orc, name, po2):
    """The CODE columns the oracle generates, interpolated, shifted and evaluated on the 4N coset by the oracle's transforms (the field
    side does not depend on the suite), hashed and folded by the restatement."""
    import hyperfridge_r0_amd as r0
    blob = np.fromfile(circuit_path(name), dtype=np.uint32)
    c = orc.circuit(blob)
    count = c.group_size[1]
    code = c.witgen(po2, 0)[0]
    coeffs = orc.zk_shift(orc.batch_interpolate_ntt(code, count, po2), count, po2)
    evaluated = orc.batch_expand_into_evaluate_ntt(coeffs, count, po2, 2)
    want = ref.merkle_build(evaluated, 4 << po2, count).reshape(-1, 8)[1]
    assert np.array_equal(r0.control_root_host(blob, po2, hashfn="sha-256"), want)
    assert np.array_equal(r0.control_root_host(blob, po2, hashfn="poseidon2"), r0.control_root_host(blob, po2))
    assert not np.array_equal(r0.control_root_host(blob, po2), want)


def test_unknown_hashfn_is_an_error():
    import hyperfridge_r0_amd as r0
    blob = np.fromfile(circuit_path("tiny"), dtype=np.uint32)
    seal = np.load(os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy"))
    z = np.zeros(8, dtype=np.uint32)
    for bad in ("blake2b", "sha256", "SHA-256", ""):
        with pytest.raises(r0.R0HipError, match="unknown hash function"):
            r0.hash_pair_host(bad, z, z)
        with pytest.raises(r0.R0HipError, match="unknown hash function"):
            r0.hash_elems_host(bad, z)
        with pytest.raises(r0.R0HipError, match="unknown hash function"):
            r0.control_root_host(blob, 9, hashfn=bad)
        with pytest.raises(r0.R0HipError, match="unknown hash function"):
            r0.verify_seal(blob, seal, hashfn=bad)
    # the golden Poseidon2 seal: accepted under its own name through the new entry point, refused (a verdict, not an error) under the other
    assert r0.verify_seal(blob, seal, hashfn="poseidon2")[:2] == (0, "ok")
    verdict, reason, _ = r0.verify_seal(blob, seal, hashfn="sha-256")
    assert verdict != 0 and reason != "ok"


def test_reference_rng_known_start():
    g = ref.Sha256Rng()
    assert g.pool0.tobytes() == hashlib.sha256(b"Hello").digest() and g.pool1.tobytes() == hashlib.sha256(b"World").digest()
    first = [g.random_u32() for _ in range(8)]
    assert first == [int(x) for x in np.frombuffer(hashlib.sha256(b"Hello").digest(), dtype="<u4")]
    g.random_u32()  # the ninth draw steps the pools
    assert g.used == 1 and g.pool0.tobytes() != hashlib.sha256(b"Hello").digest()
    assert all(0 <= g.random_elem() < ref.P for _ in range(20)) and g.random_bits(5) < 32


def test_prove_cli_refuses_sha256_with_receipt_options(tmp_path):
    """`r0h_prove --hashfn sha-256` is for bare seals: with any receipt option or --elf it stops with a message before touching a device"""
    import subprocess
    exe = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    for extra in (["--receipt-out", str(tmp_path / "r.json")], ["--receipt-dir", str(tmp_path)], ["--elf", "guest.elf"], ["--receipt-prefix", "x"],
                  ["--image-circuit", circuit_path("image")]):
        out = subprocess.run([exe, circuit_path("tiny"), "--hashfn", "sha-256"] + extra, capture_output=True, text=True)
        assert out.returncode == 1 and "receipts name poseidon2 only" in out.stderr, extra
    out = subprocess.run([exe, circuit_path("tiny"), "--hashfn", "blake2b"], capture_output=True, text=True)
    assert out.returncode == 1 and "--hashfn is poseidon2 or sha-256" in out.stderr


def test_verify_cli_takes_hashfn_for_a_bare_seal(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_verify")
    seal = str(tmp_path / "seal.bin")
    np.load(os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy")).tofile(seal)
    ok = subprocess.run([exe, circuit_path("tiny"), seal, "--hashfn", "poseidon2"], capture_output=True, text=True)
    assert ok.returncode == 0 and '"accepted": true' in ok.stdout
    no = subprocess.run([exe, circuit_path("tiny"), seal, "--hashfn", "sha-256"], capture_output=True, text=True)
    assert no.returncode == 1 and '"accepted": false' in no.stdout
    bad = subprocess.run([exe, circuit_path("tiny"), seal, "--hashfn", "md5"], capture_output=True, text=True)
    assert bad.returncode == 2 and "unknown hash function" in bad.stderr
