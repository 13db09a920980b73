"""r0h_compress: a receipt compressed to one root in one call, on 1, 2 and 4 prover lanes -- the root the sequential fold of r0h_lift /
r0h_join gives, word for word, with its leaves' session parts -- and the root held to its session (r0h_root_verify_session_*).  Shapes
are those of tests/test_recursion.py's proved-run test: the small guest, segment_po2 = 11 (2^16-row seals), recursion traces of 2^17
rows.  One session is proved per module."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from hyperfridge_r0_amd import recursion
from conftest import ROOT, circuit_path

pytestmark = pytest.mark.gpu
WORDS = [7, 0x01020304]
P = 2013265921


def _blob(name):
    return np.fromfile(circuit_path(name), dtype=np.uint32)


class Proved:
    pass


@pytest.fixture(scope="module")
def proved(hal):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    p = Proved()
    p.blob, p.rec_blob, p.iblob = _blob("trace"), _blob("recursion"), _blob("image")
    p.gc = hal.load_circuit(p.blob, entry.code_object_path("trace"))
    p.ic = hal.load_circuit(p.iblob, entry.code_object_path("image"))
    p.elf = elf_of(_guest(2000), 0x400)
    hal.set_image_circuit(p.ic)  # the receipt carries its image proof: the image id alone verifies the root's session
    p.receipt, p.image_id, _ = hal.prove_elf(p.gc, p.elf, WORDS, segment_po2=11)
    hal.set_image_circuit(None)
    p.seals, p.claims = [s for _, s in p.receipt.seals()], p.receipt.claims()
    assert len(p.seals) >= 8
    p.roots = {}
    for s in p.seals:
        size = r0.verify_seal(p.blob, s)[2]
        if size not in p.roots:
            cc = hal.code_commit(p.gc, size)
            p.roots[size] = cc.root()
            cc.free()
    p.rec = recursion.Recursor(hal, p.rec_blob, p.blob, entry.code_object_path("recursion"), po2=17, segment_roots=p.roots)
    p.by_hand = p.rec.fold([p.rec.lift(s, cl) for s, cl in zip(p.seals, p.claims)])
    yield p
    p.rec.close()
    p.ic.free()
    p.gc.free()


def test_the_hand_built_root_carries_its_leaves_session_parts(proved):
    p = proved
    want = np.stack([r0.trace_seal_session_part(p.blob, s) for s in p.seals])
    assert p.by_hand.session.shape == (len(p.seals), r0.NODE_SESSION_WORDS) and np.array_equal(p.by_hand.session, want)
    assert np.array_equal(want[:, :20], np.stack([s[:20] for s in p.seals]))
    assert p.rec.verify(p.by_hand)
    assert recursion.Recursor.verify_session(p.by_hand, p.blob, p.receipt.journal, elf=p.elf)[:2] == (0, "ok")
    # a root that arrived as claim + seal has no part: its session cannot be checked, and the verifier says so
    with pytest.raises(r0.R0HipError, match="no session part"):
        recursion.Recursor.verify_session(recursion.Node.from_words(p.by_hand.to_words()), p.blob, p.receipt.journal, elf=p.elf)
    back = recursion.Node.from_wire(p.by_hand.to_wire())
    assert p.rec.verify(back) and recursion.Recursor.verify_session(back, p.blob, p.receipt.journal, elf=p.elf)[0] == 0


@pytest.mark.parametrize("lanes", [1, 2, 4])
def test_compress_gives_the_root_of_the_sequential_fold_word_for_word(proved, lanes):
    p = proved
    root = p.rec.compress(p.receipt, lanes=lanes)
    assert np.array_equal(root.seal, p.by_hand.seal) and bytes(root.claim) == bytes(p.by_hand.claim) and np.array_equal(root.session, p.by_hand.session)
    assert p.rec.verify(root)
    assert recursion.Recursor.verify_session(root, p.blob, p.receipt.journal, elf=p.elf)[:2] == (0, "ok")
    assert recursion.Recursor.verify_session(root, p.blob, p.receipt.journal, image_id=p.image_id, image_blob=p.iblob, image_proof=p.receipt.image_proof)[:2] == (0, "ok")
    halting = next(k for k, cl in enumerate(p.claims) if cl.exit_system <= 1)
    want = r0.ReceiptClaim.make(p.claims[0].pre, p.claims[-1].post, p.claims[halting].exit_system, p.claims[halting].exit_user, bytes(p.claims[halting].output_digest))
    assert root.claim.digest() == want.digest() and bytes(root.claim.output_digest) == r0.output_digest(p.receipt.journal)
    assert root.claim.pre.digest() == bytes(p.image_id)


def test_compress_with_the_default_lanes_and_refused_lane_counts(proved):
    p = proved
    assert np.array_equal(p.rec.compress(p.receipt).seal, p.by_hand.seal)
    with pytest.raises(r0.R0HipError, match="1 to 4"):
        p.rec.compress(p.receipt, lanes=5)


def test_a_self_chosen_challenge_is_refused_by_compress_and_named_by_the_roots_session(hal, proved):
    """Two shares of one session, each finished under records in which the OTHER share's first record is altered (a share refuses to
    finish under a record of its own that it did not commit): every seal verifies, every seal carries a challenge that is not the
    session's.  lift / join take them one by one, as they always did; compress refuses before it proves anything; the hand-built
    root's session says 13 at the same leaf as the receipt's verifier."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    p = proved
    elf = elf_of(_guest(300), 0x400)
    shares = [hal.session_begin(p.gc, elf, WORDS, segment_po2=11, part=k, parts=2) for k in range(2)]
    n_seg = shares[0].n_segments
    assert n_seg >= 2
    records = np.zeros((n_seg, r0.SESSION_RECORD_WORDS), dtype=np.uint32)
    for ses in shares:
        idx, rec = ses.records()
        records[idx] = rec
    parts = []
    for k, ses in enumerate(shares):
        lied = records.copy()
        lied[1 - k, 20] = (int(lied[1 - k, 20]) + 1) % P  # a DATA root word of a segment the other share owns
        parts.append(ses.finish(lied)[0])
    forged = r0.Receipt.merge(parts)
    for ses in shares:
        ses.close()
    seals, claims = [s for _, s in forged.seals()], forged.claims()
    roots = dict(p.roots)
    for s in seals:
        size = r0.verify_seal(p.blob, s)[2]
        if size not in roots:
            cc = hal.code_commit(p.gc, size)
            roots[size] = cc.root()
            cc.free()
        assert r0.verify_seal(p.blob, s, code_root=roots[size])[:2] == (0, "ok")
    verdict = forged.verify(p.blob, roots, None, elf=elf)
    assert verdict[0] == 13, verdict
    rec = recursion.Recursor(hal, p.rec_blob, p.blob, entry.code_object_path("recursion"), po2=17, segment_roots=roots)
    with pytest.raises(r0.R0HipError, match="r0h_compress: segment %d: a seal's session number, closing flag or challenge is not this session's" % verdict[2]):
        rec.compress(forged, lanes=2)
    by_hand = rec.fold([rec.lift(s, cl) for s, cl in zip(seals, claims)])
    assert rec.verify(by_hand)
    assert recursion.Recursor.verify_session(by_hand, p.blob, forged.journal, elf=elf)[::2] == (13, verdict[2])
    rec.close()


def test_a_receipt_that_cannot_be_lifted_returns_lifts_error_and_leaves_no_lane_running(proved):
    p = proved
    bad = [s.copy() for s in p.seals]
    bad[3][-1] ^= 1
    broken = r0.Receipt.new(p.receipt.journal, bad, p.claims)
    with pytest.raises(r0.R0HipError, match="lift: the seal to be consumed does not verify"):
        p.rec.compress(broken, lanes=4)
    # a claim that is not the seal's: refused by a lift inside the queue, after other lanes have started -- every lane is joined
    swapped = list(p.claims)
    swapped[2], swapped[3] = swapped[3], swapped[2]
    with pytest.raises(r0.R0HipError, match="r0h_lift: the segment seal's public inputs do not name this claim"):
        p.rec.compress(r0.Receipt.new(p.receipt.journal, p.seals, swapped), lanes=4)
    root = p.rec.compress(p.receipt, lanes=4)  # the same recursor, afterwards: nothing is left running or held
    assert np.array_equal(root.seal, p.by_hand.seal)


def test_the_compiled_hosts_compress_a_receipt_and_verify_the_root(proved, tmp_path):
    """`r0h_prove --elf .. --compress .. --root-out root.bin` then `r0h_verify --root root.bin --receipt r.json ..`: accepted with the
    ELF (exit status 0); with another ELF refused with verdict 8 (exit status non-zero)."""
    import json
    import subprocess
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import ADDI, _guest
    prove, verify = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove"), os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_verify")
    prog = _guest(300)
    elf, other, words = tmp_path / "guest.elf", tmp_path / "other.elf", tmp_path / "words.bin"
    elf.write_bytes(elf_of(prog, 0x400))
    other.write_bytes(elf_of(prog[:-4] + [ADDI(0, 0, 0)] + prog[-3:], 0x400))
    np.array(WORDS, dtype=np.uint32).tofile(str(words))
    receipt, root = str(tmp_path / "r.json"), str(tmp_path / "root.bin")
    out = subprocess.run([prove, circuit_path("trace"), "--code-object", entry.code_object_path("trace"), "--elf", str(elf), "--input", str(words), "--po2", "11",
                          "--receipt-out", receipt, "--compress", "--recursion-circuit", circuit_path("recursion"), "--recursion-code-object",
                          entry.code_object_path("recursion"), "--recursion-po2", "17", "--root-out", root], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    report = json.loads(out.stdout.strip().splitlines()[-1])
    assert report["root"] == root and report["root_leaves"] == report["segments"] >= 2
    node = recursion.Node.from_wire(np.fromfile(root, dtype=np.uint32))
    assert node.session.shape[0] == report["segments"]
    common = [verify, "--root", root, "--receipt", receipt, circuit_path("trace"), "--recursion-circuit", circuit_path("recursion")]
    out = subprocess.run(common + ["--elf", str(elf)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and json.loads(out.stdout)["accepted"] is True and json.loads(out.stdout)["verdict"] == 0, out.stdout + out.stderr
    out = subprocess.run(common + ["--elf", str(other)], capture_output=True, text=True, timeout=300)
    verdict = json.loads(out.stdout)
    assert out.returncode != 0 and verdict["accepted"] is False and verdict["verdict"] == 8 and verdict["reason"] == "the first pre-state is not the expected image id", out.stdout
