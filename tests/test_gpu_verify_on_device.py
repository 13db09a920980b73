"""Seals and receipts verified with the device hashing their Merkle openings (r0h_verify_seals_on, r0h_receipt_verify_elf_on /
_image_on): the host walks every seal and makes every comparison, the device computes the digests of one batch of openings.  Verdict
and reason must be the host verifier's for every input: the mutation list of tests/verify_mutations.py over seals of circuits/tiny.r0c
at po2 9 and circuits/small.r0c at po2 11 proved here, one of them also under SHA-256, alone and as one batch of mixed po2; a receipt
of the small trace guest (2^16-row segments) good, with one altered seal word and with one altered journal byte."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path
from verify_mutations import mutations

pytestmark = pytest.mark.gpu
WORDS = [7, 0x01020304]


def _blob(name):
    return np.fromfile(circuit_path(name), dtype=np.uint32)


def _load(h, name):
    co = entry.code_object_path(name)
    return h.load_circuit(_blob(name), co if name != "tiny" and os.path.exists(co) else None)


@pytest.fixture(scope="module")
def sha():
    h = r0.Hal(0)
    h.set_hashfn("sha-256")
    yield h
    h.close()


def _seal(h, name, po2, seed):
    gc = _load(h, name)
    code, data, glob = h.witgen(gc, po2, seed)
    seal = h.prove_segment(gc, po2, code, data, glob)
    root = h.code_root(gc, po2)
    gc.free()
    return seal, root


@pytest.fixture(scope="module")
def tiny9(hal):
    return _seal(hal, "tiny", 9, 1)


@pytest.fixture(scope="module")
def small11(hal):
    return _seal(hal, "small", 11, 2)


@pytest.fixture(scope="module")
def tiny9_sha(sha):
    return _seal(sha, "tiny", 9, 1)


def _held_to_the_host(h, blob, cases, suite, root=None):
    seen = set()
    for label, seal in cases:
        want = r0.verify_seal(blob, seal, code_root=root, hashfn=suite)
        got = h.verify_seals(blob, [seal], None if root is None else [root])[0]
        assert got[:3] == want, "%s: device-hashed %r, host %r" % (label, got[:3], want)
        assert (got[0] == 0) == (label == "untouched"), (label, got)
        seen.add(got[0])
    return seen


def test_tiny_po2_9_every_mutation_gives_the_hosts_verdict(hal, tiny9):
    seal, root = tiny9
    seen = _held_to_the_host(hal, _blob("tiny"), mutations(_blob("tiny"), seal), "poseidon2", root)
    assert {0, 1, 3, 4, 5, 8, 9} <= seen


def test_small_po2_11_every_mutation_gives_the_hosts_verdict(hal, small11):
    seal, root = small11
    seen = _held_to_the_host(hal, _blob("small"), mutations(_blob("small"), seal), "poseidon2", root)
    assert {0, 1, 3, 4, 5, 8, 9} <= seen


def test_sha256_seals_are_verified_on_a_sha256_context(hal, sha, tiny9, tiny9_sha):
    seal, _ = tiny9_sha
    blob = _blob("tiny")
    seen = _held_to_the_host(sha, blob, mutations(blob, seal), "sha-256")
    assert {0, 1, 3, 5, 8} <= seen  # (a digest word raised by p is just another digest under this suite)
    # a seal of the other suite is a verdict, as on the host
    assert sha.verify_seals(blob, [tiny9[0]])[0][:2] == r0.verify_seal(blob, tiny9[0], hashfn="sha-256")[:2] != (0, "ok")
    assert hal.verify_seals(blob, [seal])[0][:2] == r0.verify_seal(blob, seal)[:2] != (0, "ok")


def test_a_batch_of_mixed_po2_is_one_launch_and_every_seal_its_own_verdict(hal):
    """one circuit, seals of 2^9 and 2^11 rows side by side (their trees differ in path length, so their jobs land in different waves),
    every mutation of both in ONE batch: each verdict the host's, the DATA roots r0h_verify_seal_roots's"""
    blob = _blob("tiny")
    s9, r9 = _seal(hal, "tiny", 9, 4)
    s11, r11 = _seal(hal, "tiny", 11, 5)
    cases = [(l, s, r9) for l, s in mutations(blob, s9)] + [(l, s, r11) for l, s in mutations(blob, s11)]
    order = np.random.default_rng(3).permutation(len(cases))
    cases = [cases[i] for i in order]
    hal.kernel_timing(True)
    before = hal.kernel_stats().get("merkle_climb_kernel", {"launches": 0})["launches"]
    got = hal.verify_seals(blob, [s for _, s, _ in cases], [r for _, _, r in cases])
    launches = hal.kernel_stats()["merkle_climb_kernel"]["launches"] - before
    hal.kernel_timing(False)
    assert launches == 1
    for (label, seal, root), g in zip(cases, got):
        assert g[:3] == r0.verify_seal(blob, seal, code_root=root), label
        want = np.zeros(8, dtype=np.uint32)
        verdict, po2 = r0._c.c_int(-1), r0._u32(0)
        s_, rt = np.ascontiguousarray(seal), np.ascontiguousarray(root)
        r0._check(r0.lib().r0h_verify_seal_roots(blob.ctypes.data, blob.size, s_.ctypes.data, s_.size, rt.ctypes.data, r0.ctypes.byref(verdict), r0.ctypes.byref(po2), want.ctypes.data))
        assert verdict.value == g[0] and np.array_equal(g[3], want), label
    assert sorted(g[2] for g in got if g[0] == 0) == [9, 11]


class Proved:
    pass


@pytest.fixture(scope="module")
def proved(hal):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    p = Proved()
    p.blob, p.iblob = _blob("trace"), _blob("image")
    p.gc = hal.load_circuit(p.blob, entry.code_object_path("trace"))
    p.ic = hal.load_circuit(p.iblob, entry.code_object_path("image"))
    p.elf = elf_of(_guest(300), 0x400)
    hal.set_image_circuit(p.ic)
    p.receipt, p.image_id, _ = hal.prove_elf(p.gc, p.elf, WORDS, segment_po2=11)
    hal.set_image_circuit(None)
    p.seals, p.claims = [s for _, s in p.receipt.seals()], p.receipt.claims()
    p.roots = {}
    for s in p.seals:
        size = r0.verify_seal(p.blob, s)[2]
        assert size == 16
        if size not in p.roots:
            p.roots[size] = hal.code_root(p.gc, size)
    yield p
    p.ic.free()
    p.gc.free()


def test_a_receipt_verifies_with_the_elf_and_with_its_image_proof_as_on_the_host(hal, proved):
    p = proved
    assert len(p.seals) >= 2
    assert p.receipt.verify(p.blob, p.roots, None, elf=p.elf, hal=hal) == p.receipt.verify(p.blob, p.roots, None, elf=p.elf) == (0, "ok", 0, 0)
    assert p.receipt.verify_image(p.blob, p.roots, p.iblob, p.image_id, hal=hal) == p.receipt.verify_image(p.blob, p.roots, p.iblob, p.image_id) == (0, "ok", 0, 0)


def test_an_altered_seal_word_and_an_altered_journal_byte_get_the_hosts_verdicts(hal, proved):
    p = proved
    bad = [s.copy() for s in p.seals]
    bad[1][-1] ^= 1  # the last path digest of the last query of segment 1
    broken = r0.Receipt.new(p.receipt.journal, bad, p.claims)
    broken.image_proof = p.receipt.image_proof
    want = broken.verify(p.blob, p.roots, None, elf=p.elf)
    assert want[0] == 2 and want[2] == 1 and want[3] != 0
    assert broken.verify(p.blob, p.roots, None, elf=p.elf, hal=hal) == want
    assert broken.verify_image(p.blob, p.roots, p.iblob, p.image_id, hal=hal) == broken.verify_image(p.blob, p.roots, p.iblob, p.image_id)
    # an altered image seal: the image proof is what is refused, before any segment
    worse = r0.Receipt.new(p.receipt.journal, p.seals, p.claims)
    image = p.receipt.image_proof.copy()
    image[-1] ^= 1
    worse.image_proof = image
    want = worse.verify_image(p.blob, p.roots, p.iblob, p.image_id)
    assert want[0] == 16 and want[3] != 0
    assert worse.verify_image(p.blob, p.roots, p.iblob, p.image_id, hal=hal) == want
    journal = bytearray(p.receipt.journal)
    journal[-1] ^= 1
    other = r0.Receipt.new(bytes(journal), p.seals, p.claims)
    other.image_proof = p.receipt.image_proof
    want = other.verify(p.blob, p.roots, None, elf=p.elf)
    assert want[0] == 7
    assert other.verify(p.blob, p.roots, None, elf=p.elf, hal=hal) == want
    assert other.verify_image(p.blob, p.roots, p.iblob, p.image_id, hal=hal) == other.verify_image(p.blob, p.roots, p.iblob, p.image_id)
    # a size without a control root: the walk stops before that seal, and so does the batch
    assert p.receipt.verify(p.blob, {15: p.roots[16]}, None, elf=p.elf, hal=hal) == p.receipt.verify(p.blob, {15: p.roots[16]}, None, elf=p.elf)


def test_the_compiled_prover_verifies_what_it_made_on_its_proving_context(tmp_path):
    """`r0h_prove --verify-device 1`: the after-proof check of --verify (bare seals, both suites) and of an --elf run's receipts (with
    the ELF and, given the image circuit, with the image id alone) through the _on forms on the contexts that proved"""
    import json
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    for suite in ("poseidon2", "sha-256"):
        out = subprocess.run([prove, circuit_path("small"), "--po2", "11", "--seed", "9", "--hashfn", suite, "--verify", "1", "--verify-device", "1"],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "seals verified" in out.stderr, out.stdout + out.stderr
    elf, words, receipt = tmp_path / "guest.elf", tmp_path / "words.bin", str(tmp_path / "r.json")
    elf.write_bytes(elf_of(_guest(300), 0x400))
    np.array(WORDS, dtype=np.uint32).tofile(str(words))
    out = subprocess.run([prove, circuit_path("trace"), "--code-object", entry.code_object_path("trace"), "--elf", str(elf), "--input", str(words), "--po2", "11",
                          "--receipt-out", receipt, "--image-circuit", circuit_path("image"), "--image-code-object", entry.code_object_path("image"),
                          "--verify-device", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["receipts_verified_with_the_elf"] == 1 and report["receipts_verified_with_the_image_id_alone"] == 1 and report["segments"] >= 2
