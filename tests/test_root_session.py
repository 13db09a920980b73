"""A root of the lift / join tree held to its session (r0h_root_verify_session_elf / _image, csrc/claim.cpp): the same verdict and the
same leaf as r0h_receipt_verify_elf / _image give for the receipt the root stands for -- honest and forged sessions proved by the
oracle (tests/session_by_hand.py) -- and named verdicts for session parts tampered with on their way to the root.  The verifier never
reads a node's seal, so the nodes here are r0h_node_new_with_session over a placeholder seal, their claims composed in Python the way
r0h_join composes them.  No GPU."""
import hashlib
import os
import queue
import sys
import threading

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from hyperfridge_r0_amd import recursion
from conftest import ROOT, circuit_path
from test_rv32im import _guest

sys.path.insert(0, os.path.join(ROOT, "tools"))
import session_by_hand as sbh  # noqa: E402

P = 2013265921
W = r0.NODE_SESSION_WORDS
PLACEHOLDER = np.arange(32, dtype=np.uint32)  # stands for a node's seal: the session verifier does not read it


def compose(claims):
    """the claim r0h_join gives the root over these leaves: pre of the first, post of the last, the way of ending of the leaf that ends the run"""
    term = next((k for k, c in enumerate(claims) if c.exit_system <= 1), len(claims) - 1)
    return r0.ReceiptClaim.make(claims[0].pre, claims[-1].post, claims[term].exit_system, claims[term].exit_user, bytes(claims[term].output_digest))


def root_of(blob, receipt, claims=None):
    parts = np.stack([r0.trace_seal_session_part(blob, s) for _, s in receipt.seals()])
    return recursion.Node.from_parts(PLACEHOLDER, compose(claims or receipt.claims()), parts)


class Case:
    pass


@pytest.fixture(scope="module")
def case(orc):
    """the two-segment run of tests/test_trace_circuit.py's session test, proved once by the oracle"""
    from bench_session import elf_of
    c = Case()
    c.blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    c.pv = sbh.OracleProver(orc.circuit(c.blob))
    c.prog, c.base = _guest(160), 0x400
    c.elf = elf_of(c.prog, c.base)
    c.elf_of = elf_of

    def run(elf=c.elf):
        vm = r0.Vm()
        vm.load_elf(elf)
        vm.set_input([7, 0x01020304])
        assert vm.run(segment_po2=10, keep_trace=True, boundary_rows=True) == (0, 0)
        return vm

    c.run = run
    c.vm = run()
    c.receipt, c.roots = sbh.prove_session(c.pv, c.vm)
    c.seals = [s for _, s in c.receipt.seals()]
    assert len(c.seals) == 2
    c.node = root_of(c.blob, c.receipt)
    return c


def same_as_receipt(c, receipt, roots, node, elf, journal=None):
    want = receipt.verify(c.blob, roots, None, elf=elf)
    got = recursion.Recursor.verify_session(node, c.blob, receipt.journal if journal is None else journal, elf=elf)
    assert got[:2] == want[:2] and got[2] == want[2], (got, want)
    return got


def test_the_session_part_of_a_seal_is_the_layout_the_header_states(case):
    c = case
    parts = c.node.session
    assert parts.shape == (2, W) and W == r0.SESSION_RECORD_WORDS + 16 + 4
    early = r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS
    for part, seal in zip(parts, c.seals):
        assert np.array_equal(part[:early], seal[:early])
        assert np.array_equal(part[28:44], seal[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16]) and np.array_equal(part[44:48], seal[r0.TRACE_SUM:r0.TRACE_SUM + 4])
    # words [0, 28) are the session's records: the challenge every honest seal carries is derived from exactly them
    assert np.array_equal(r0.session_challenge(np.ascontiguousarray(parts[:, :28])), c.seals[0][r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16])
    # ... and the DATA root among them is the one the prover committed to (the oracle's own root of the witness's DATA group)
    wit = sbh.witnesses(c.vm)
    for part, (size, data, _) in zip(parts, wit):
        assert np.array_equal(part[early:28], c.pv.data_root(size, data))
    with pytest.raises(r0.R0HipError, match="does not verify"):
        bad = c.seals[0].copy()
        bad[-1] ^= 1
        r0.trace_seal_session_part(c.blob, bad)
    with pytest.raises(r0.R0HipError, match="not the trace circuit"):
        r0.trace_seal_session_part(np.fromfile(circuit_path("small"), dtype=np.uint32), c.seals[0])


def test_an_honest_root_verifies_with_the_elf_and_a_forged_session_gets_the_receipts_verdict(case, orc):
    from test_rv32im import ADDI
    c = case
    assert same_as_receipt(c, c.receipt, c.roots, c.node, c.elf)[:2] == (0, "ok")
    # another ELF (one instruction the run never reached differs): its image id is not the claim's pre-state.  The root's verifier
    # looks at the image id before the session section and says 8; the receipt's reaches the balance first and may say 14
    other = c.elf_of(c.prog[:-4] + [ADDI(0, 0, 0)] + c.prog[-3:], c.base)
    assert recursion.Recursor.verify_session(c.node, c.blob, c.receipt.journal, elf=other)[::2] == (8, 0)
    assert c.receipt.verify(c.blob, c.roots, None, elf=other)[0] in (8, 14)
    # another journal: the claim commits to the one the run wrote
    journal = bytearray(c.receipt.journal)
    journal[0] ^= 1
    swapped = r0.Receipt.new(bytes(journal), c.seals, c.receipt.claims())
    assert same_as_receipt(c, swapped, c.roots, c.node, c.elf, journal=bytes(journal))[0] == 7
    # a journal byte altered with the output digest recomputed: the COMMIT rows named another word
    vm3 = c.run()
    claims = vm3.claims()
    claims[-1] = r0.ReceiptClaim.make(claims[-1].pre, claims[-1].post, 0, 0, output_digest=r0.output_digest(bytes(journal)))
    forged, roots3 = sbh.prove_session(c.pv, vm3, claims=claims, journal=bytes(journal))
    assert same_as_receipt(c, forged, roots3, root_of(c.blob, forged), c.elf)[0] == 14
    # program B executed, program A's state planted as the first claim
    elf_a = c.elf_of([ADDI(0, 0, 1)] + c.prog[1:], c.base)
    vm4 = c.run()
    claims = vm4.claims()
    vm_a = r0.Vm()
    vm_a.load_elf(elf_a)
    assert vm_a.run(max_cycles=1)[0] == r0.Vm.LIMIT
    claims[0] = r0.ReceiptClaim.make(vm_a.segments()[0].pre, claims[0].post, 2, 0)
    forged, roots4 = sbh.prove_session(c.pv, vm4, claims=claims)
    assert same_as_receipt(c, forged, roots4, root_of(c.blob, forged), elf_a)[0] == 14
    # a challenge of the prover's own choosing: every seal verifies, lift and join would take them, the root's session does not hold
    forged, roots5 = sbh.prove_session(c.pv, c.run(), challenge=lambda rec: r0.session_challenge(rec[::-1].copy()))
    assert same_as_receipt(c, forged, roots5, root_of(c.blob, forged), c.elf)[:3] == (13, "a seal's session number, closing flag or challenge is not this session's", 0)


def test_a_value_altered_between_two_segments_is_refused_like_the_receipt(case, orc):
    """test_trace_circuit's case (iii): segment 1 'finds' another word than segment 0 left.  The receipt's verifier says 2 (the seal
    itself) or 14; with 2 there is no leaf to extract -- r0h_trace_seal_session_part refuses the seal, as r0h_lift would."""
    from trace_corners import COL
    c = case
    vm2 = c.run()
    segs, b1 = vm2.segments(), vm2.boundary(1)
    j = next(i for i, b in enumerate(b1) if b.prev_seg == 1 and b.addr < r0.REG_BASE and b.first_value == b.last_value)
    n1 = segs[1].user_cycles

    def alter(k, data, glob):
        if k != 1:
            return False
        n = 1 << r0.TRACE_MIN_PO2
        v = b1[j].first_value ^ 0x40
        for col, val in (("after_lo", v & 0xFFFF), ("zq", (v & 0xFFFF) >> 2), ("before_lo", v & 0xFFFF)):
            data[COL[col] * n + n1 + j] = orc.enc(val)
        for r, w in enumerate(vm2.preflight(1)):
            if w.mem_kind and (w.mem_addr >> 2) == b1[j].addr:
                for col in ("before_lo", "after_lo"):
                    data[COL[col] * n + r] = orc.enc(v & 0xFFFF)
        return True

    forged, roots2 = sbh.prove_session(c.pv, vm2, edit=alter)
    verdict = forged.verify(c.blob, roots2, None, elf=c.elf)
    assert verdict[0] in (2, 14), verdict
    if verdict[0] == 2:
        with pytest.raises(r0.R0HipError, match="does not verify"):
            root_of(c.blob, forged)
    else:
        assert same_as_receipt(c, forged, roots2, root_of(c.blob, forged), c.elf)[0] == 14


def test_the_image_proof_stands_for_the_elf_at_a_root_as_it_does_at_a_receipt(case, orc):
    c = case
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    oi = orc.circuit(iblob)
    image_id = r0.compute_image_id(c.elf)
    challenge = c.seals[0][r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16]

    def image_seal(of_elf, under=challenge):
        po2 = r0.image_po2(of_elf)
        data, glob = r0.image_witness(of_elf, po2)
        glob[r0.IMAGE_GAMMA:r0.IMAGE_GAMMA + 16] = under
        code = oi.witgen(po2, 0)[0]
        return oi.prove(po2, code, data.reshape(-1), oi.logup_totals(po2, code, data.reshape(-1), glob))

    def both(proof, with_id=image_id):
        c.receipt.image_proof = proof
        want = c.receipt.verify_image(c.blob, c.roots, iblob, with_id)
        got = recursion.Recursor.verify_session(c.node, c.blob, c.receipt.journal, image_id=with_id, image_blob=iblob, image_proof=proof)
        c.receipt.image_proof = None
        assert got[:2] == want[:2] and got[2] == want[2], (got, want)
        return got[0]

    from test_rv32im import ADDI
    good = image_seal(c.elf)
    assert both(good) == 0                                                                                  # the 32 bytes of the image id, no ELF
    assert both(None) == 16                                                                                 # no image proof
    assert both(image_seal(c.elf_of(c.prog[:-4] + [ADDI(0, 0, 0)] + c.prog[-3:], c.base))) == 16            # another program's
    assert both(image_seal(c.elf, under=np.roll(challenge, 4))) == 16                                       # another session's
    assert both(good, r0.compute_image_id(c.elf_of(c.prog, c.base + 4))) == 8                               # another image id
    assert recursion.Recursor.verify_session(c.node, c.blob, c.receipt.journal, image_id=image_id, image_blob=iblob, image_proof=good,
                                             image_control_root=r0.control_root_host(iblob, r0.image_po2(c.elf) + 1))[0] == 16


def test_session_parts_tampered_in_transit_are_named(case):
    """The parts travel beside the node.  What each alteration of an honest root's parts runs into, with the ELF in hand:"""
    c = case
    claim, parts, journal = c.node.claim, c.node.session, c.receipt.journal

    def verdict(session):
        return recursion.Recursor.verify_session(recursion.Node.from_parts(PLACEHOLDER, claim, session), c.blob, journal, elf=c.elf)[::2]

    def bumped(leaf, word):
        out = parts.copy()
        out[leaf, word] = (int(out[leaf, word]) + 1) % P
        return out

    assert verdict(parts) == (0, 0)
    assert verdict(bumped(1, 44)) == (14, 0)        # one sum word: the sums no longer balance (the balance is the session's, leaf 0 is named)
    assert verdict(bumped(0, 20)) == (13, 0)        # one record word (a DATA root word): the challenge derived from the records is no leaf's
    assert verdict(bumped(1, 20)) == (13, 0)        # ... whichever leaf's record it is, the first leaf already disagrees
    assert verdict(bumped(1, 28)) == (13, 1)        # one challenge word: that leaf carries another challenge than the session's
    assert verdict(parts[:1]) == (5, 0)             # the last leaf dropped: the leaf that now ends the run does not end the way the claim says
    assert verdict(parts[1:]) == (6, 0)             # the first leaf dropped: the run does not start at the claim's first pc
    assert verdict(parts[::-1]) == (6, 0)           # two leaves swapped: likewise
    assert verdict(parts[[0, 0, 1]]) == (6, 1)      # a leaf duplicated: leaf 1 does not start where leaf 0 stopped
    assert verdict(bumped(0, 15)) == (13, 0)        # a record word the chain does not read (the segment's number): numbers count 1..n


def test_what_cannot_be_read_as_a_session_is_an_error_not_a_verdict(case):
    c = case
    claim, journal = c.node.claim, c.receipt.journal
    check = lambda node: recursion.Recursor.verify_session(node, c.blob, journal, elf=c.elf)
    with pytest.raises(r0.R0HipError, match="no session part"):
        check(recursion.Node.from_parts(PLACEHOLDER, claim))
    with pytest.raises(r0.R0HipError, match="no session part"):
        check(recursion.Node.from_parts(PLACEHOLDER, claim, np.zeros((0, W), dtype=np.uint32)))
    bad = c.node.session.copy()
    bad[1, 30] = P
    with pytest.raises(r0.R0HipError, match="leaf 1's session part is not a canonical field word"):
        check(recursion.Node.from_parts(PLACEHOLDER, claim, bad))
    # 2^20 leaves: a segment's number would share its field slot with R0H_SESSION_TAG_IMAGE; refused on the count alone (the parts are
    # fabricated -- all zero -- and would fail every later check; the error comes first)
    many = recursion.Node.from_parts(PLACEHOLDER, claim, np.zeros((1 << 20, W), dtype=np.uint32))
    with pytest.raises(r0.R0HipError, match="fewer than 2\\^20 segments"):
        check(many)
    many.free()
    with pytest.raises(r0.R0HipError, match="not the trace circuit"):
        recursion.Recursor.verify_session(c.node, np.fromfile(circuit_path("small"), dtype=np.uint32), journal, elf=c.elf)


def test_a_node_travels_in_wire_form_with_and_without_its_session_part(case):
    c = case
    for node in (c.node, recursion.Node.from_parts(PLACEHOLDER, c.node.claim)):
        wire = node.to_wire()
        back = recursion.Node.from_wire(wire)
        assert np.array_equal(back.seal, node.seal) and back.claim.digest() == node.claim.digest() and np.array_equal(back.session, node.session)
        assert back.session.shape == node.session.shape and np.array_equal(back.to_wire(), wire)
        assert np.array_equal(recursion.Node.from_words(node.to_words()).seal, node.seal)  # (the claim + seal form is unchanged and carries no part)
        for cut in (wire[:-1], wire[:recursion.CLAIM_WORDS + 1], wire[:recursion.CLAIM_WORDS + 2], np.concatenate([wire, wire[:1]])):
            with pytest.raises(r0.R0HipError, match="wire form"):
                recursion.Node.from_wire(cut)
    assert recursion.Node.from_words(c.node.to_words()).session.shape == (0, W)


class _PartRecursor:
    """Stand-in prover for the transport: a join's 'seal' is a hash of its children's, its session part their parts, left then right
    (what r0h_join does with them); the nodes are real r0h_nodes, so they travel in the library's wire form."""

    def __init__(self, claim):
        self.claim = claim

    def leaf(self, i):
        part = np.full((1, W), i + 1, dtype=np.uint32)
        return recursion.Node.from_parts(np.frombuffer(hashlib.sha256(b"leaf%d" % i).digest(), dtype=np.uint32) % P, self.claim, part)

    def join(self, a, b):
        seal = np.frombuffer(hashlib.sha256(a.seal.tobytes() + b.seal.tobytes()).digest(), dtype=np.uint32) % P
        return recursion.Node.from_parts(seal, self.claim, np.concatenate([a.session, b.session]))

    def node_from_wire(self, words):
        return recursion.Node.from_wire(words)


@pytest.mark.parametrize("world", [1, 2, 5])
def test_the_parts_reach_the_root_in_leaf_order_across_ranks(case, world):
    rec = _PartRecursor(case.node.claim)
    boxes = {(s, d): queue.Queue() for s in range(world) for d in range(world)}
    results = [None] * world

    def run(rank):
        send = lambda words, dst: boxes[(rank, dst)].put(words.copy())
        recv = lambda src: boxes[(src, rank)].get(timeout=10)
        results[rank] = recursion.join_across_ranks(rec, rec.leaf(rank), rank, world, send, recv, with_session=True)

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join(20) for t in threads]
    assert all(r is None for r in results[1:])
    assert results[0].session.shape == (world, W) and results[0].session[:, 0].tolist() == list(range(1, world + 1))
