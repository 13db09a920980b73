"""r0h_ctx_set_session_enqueue: the second phase of a trace-circuit session driven by the calling thread alone -- every segment's session
sum, late inputs, accumulation and finish enqueued on its lane's stream, one segment per lane in flight, collected in the order they
were enqueued.  A session of three segments of 2^16 rows (with two lanes one lane holds two of them: the rotation runs): the receipt
is byte for byte the receipt of the lanes' form, with one lane and with two, with the image circuit set, with a segment evicted and
with its tree top kept; it verifies with the ELF and with the image id alone; phase 2 ran on one thread and waited, per segment, for
the collect's read-back and the close of the lane's profile and for nothing else of its own.

The session check (r0h_ctx_set_check_session) with the switch on: an honest session gives the same receipt, 'check_session' stands in the
profile before any phase of phase 2, nothing stays held.  A forged row cannot be carried through r0h_session_finish: the check's
verifier side is made from the ELF the session itself executed, and an honest executor balances (tests/test_gpu_session_balance.py says
the same of the lanes' form).  So one of that file's forgeries is re-stated here the way it states them, through a SessionBalance
handle: the pending segments of a session begun with the switch on (r0h_session_balance_add_session, what the check adds) against the
image of another ELF; the handle names the word that differs, in the sequencer's words, before phase 2 -- and the session then finishes.

A segment that fails: between the two phases of a session the test puts the session's own context on the other hash suite, so the
late step of the first segment that context holds is refused (the helper lane's segments are not); the session's error is that
refusal, word for word; what was in flight is collected, every other proof is aborted, nothing stays held, and the context proves the
next session as before.  Which lane took which segment in phase 1 is the executor's pace, and the library has no hook to choose: with
one lane the first segment fails with nothing in flight; with two the test records, from the waits phase 2 made, how many segments
were in flight and collected when the refusal came (none if the context's lane came first in the round; all of them, and a whole
receipt, if the helper lane took every segment), and holds each outcome to what it must be."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import circuit_path
from test_rv32im import _guest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_session import elf_of  # noqa: E402

pytestmark = pytest.mark.gpu
PO2 = 16
WORDS = [7, 0x01020304]


class Run:
    def __init__(self, hal):
        self.hal = hal
        self.blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
        self.iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
        self.gc = hal.load_circuit(self.blob, entry.code_object_path("trace"))
        self.ic = hal.load_circuit(self.iblob, entry.code_object_path("image"))
        self.elf = elf_of(_guest(25000), 0x400)      # 175,000 cycles: three segments of 2^16 rows
        self.roots = {PO2: r0.control_root_host(self.blob, PO2)}
        self.off = {}

    def prove(self, enqueue, lanes="2", image=False, limit=0, tops=0):
        h = self.hal
        os.environ["R0H_SESSION_LANES"] = lanes
        h.set_session_enqueue(enqueue)
        h.set_image_circuit(self.ic if image else None)
        h.set_session_device_limit(limit)
        h.set_session_tree_tops(tops)
        try:
            receipt, image_id, _ = h.prove_elf(self.gc, self.elf, WORDS, segment_po2=PO2)
        finally:
            del os.environ["R0H_SESSION_LANES"]
            h.set_session_enqueue(False)
            h.set_image_circuit(None)
            h.set_session_device_limit(0)
            h.set_session_tree_tops(0)
        return receipt, image_id, h.last_session_phase2(), h.last_session_device()

    def reference(self, image):
        """the lanes' form, made once"""
        if image not in self.off:
            receipt, image_id, phase2, _ = self.prove(False, image=image)
            assert phase2["host_threads"] == 2
            self.off[image] = (receipt.to_json(), image_id, len(receipt.seals()))
        return self.off[image]

    def close(self):
        self.gc.free()
        self.ic.free()


@pytest.fixture(scope="module")
def run(hal):
    r = Run(hal)
    yield r
    r.close()


def own_waits(phase2):
    """what phase 2 waited for besides the ring's wrap-arounds, the replays of evicted segments and the image proof"""
    return phase2["blocking_waits"] - phase2["ring_waits"] - phase2["replay_and_image_waits"]


@pytest.mark.parametrize("image", [False, True], ids=["segments alone", "with the image proof"])
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_the_receipt_is_the_lanes_receipt_and_one_thread_made_it(run, lanes, image):
    want_json, want_id, n = run.reference(image)
    assert n >= 3
    receipt, image_id, phase2, _ = run.prove(True, lanes=lanes, image=image)
    assert receipt.to_json() == want_json and image_id == want_id
    assert phase2["host_threads"] == 1
    # by design: the collect's read-back and the close of the lane's profile, per segment; the enqueues wait for nothing
    assert own_waits(phase2) == 2 * n, phase2
    assert (phase2["replay_and_image_waits"] > 0) == image
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")
    if image:
        assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")
    assert run.hal.session_held_bytes() == 0


@pytest.mark.parametrize("tops", [0, 6], ids=["hashing replay", "replay from the tree top"])
def test_an_evicted_segment_is_replayed_by_the_calling_thread(run, tops):
    want_json, want_id, n = run.reference(True)
    _, _, _, roomy = run.prove(False, image=True, limit=1 << 50)      # (a limit nothing reaches: the count is kept)
    limit = roomy["peak_counted_bytes"] - 1                           # room for all segments but one
    receipt, image_id, phase2, dev = run.prove(True, image=True, limit=limit, tops=tops)
    assert dev["evicted"] == dev["replayed"] == 1
    assert run.hal.last_session_tree_tops()["replayed_from_top"] == (1 if tops else 0)
    assert receipt.to_json() == want_json and image_id == want_id
    assert phase2["host_threads"] == 1 and own_waits(phase2) == 2 * n and phase2["replay_and_image_waits"] > 0, phase2
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")
    assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")
    assert run.hal.session_held_bytes() == 0


def test_the_environment_sets_the_default_and_the_context_overrides_it(run):
    want_json, _, _ = run.reference(False)
    h = r0.Hal(0)       # a context that was never told
    gc = h.load_circuit(run.blob, entry.code_object_path("trace"))
    os.environ["R0H_SESSION_ENQUEUE"] = "1"
    try:
        receipt, _, _ = h.prove_elf(gc, run.elf, WORDS, segment_po2=PO2)
        assert h.last_session_phase2()["host_threads"] == 1 and receipt.to_json() == want_json
        h.set_session_enqueue(False)
        h.prove_elf(gc, run.elf, WORDS, segment_po2=PO2)
        assert h.last_session_phase2()["host_threads"] == 2
    finally:
        del os.environ["R0H_SESSION_ENQUEUE"]
        gc.free()
        h.close()


REFUSAL = "r0h_proof_late_device: the proof was begun under the poseidon2 hash suite, its context is now on sha-256"


def fail_once(run, lanes):
    """a session whose own context changes suite between the phases -> ("refused", segments collected before the refusal) or
    ("whole", 0) when that context held no segment; every assertion of either outcome is made here"""
    want_json, _, n = run.reference(False)
    h = run.hal
    os.environ["R0H_SESSION_LANES"] = lanes
    h.set_session_enqueue(True)
    try:
        ses = h.session_begin(run.gc, run.elf, WORDS, segment_po2=PO2)
    finally:
        del os.environ["R0H_SESSION_LANES"]
        h.set_session_enqueue(False)
    try:
        idx, records = ses.records()
        assert list(idx) == list(range(n)) and h.session_held_bytes() > 0
        h.set_hashfn("sha-256")          # the proofs of this context were begun under Poseidon2
        error = receipt = None
        try:
            receipt = ses.finish(records)[0]
        except r0.R0HipError as e:
            error = str(e)
        finally:
            h.set_hashfn("poseidon2")
        phase2 = h.last_session_phase2()
        assert h.session_held_bytes() == 0          # no proof alive, no witness, no rows
        assert phase2["host_threads"] == 1 and phase2["ring_waits"] == 0 and phase2["replay_and_image_waits"] == 0
        if error is None:                            # the helper lane took every segment in phase 1: nothing of this context's to refuse
            assert lanes == "2" and receipt.to_json() == want_json and phase2["blocking_waits"] == 2 * n
            return "whole", 0
        assert error == REFUSAL                      # the failing segment's message, as r0h_session_finish returns it
        # every segment in flight at the refusal was collected (two waits each); the refused proof and the ones never begun wait for nothing
        assert phase2["blocking_waits"] % 2 == 0 and phase2["blocking_waits"] // 2 <= (0 if lanes == "1" else n - 1), phase2
        return "refused", phase2["blocking_waits"] // 2
    finally:
        ses.close()
        assert h.session_held_bytes() == 0


@pytest.mark.parametrize("lanes", ["1", "2"])
def test_a_segment_that_fails_aborts_the_others_and_leaves_nothing_held(run, lanes):
    want_json, _, _ = run.reference(False)
    outcomes = [fail_once(run, lanes) for _ in range(1 if lanes == "1" else 4)]
    print("lanes", lanes, "outcomes (what, segments collected before the refusal):", outcomes)
    if lanes == "1":
        assert outcomes == [("refused", 0)]
    receipt, _, phase2, _ = run.prove(True)         # the context goes on as before
    assert receipt.to_json() == want_json and phase2["host_threads"] == 1


def test_the_session_check_runs_before_phase_2_and_the_receipt_is_the_same(run):
    want_json, want_id, n = run.reference(False)
    h = run.hal
    h.set_check_session(True)
    try:
        receipt, image_id, phase2, _ = run.prove(True)
    finally:
        h.set_check_session(False)
    assert receipt.to_json() == want_json and image_id == want_id
    names = [name for name, _ in h.last_profile()]
    assert "check_session" in names
    if "accum" in names:     # (the context's own lane held a segment: its phase 2 stands behind the check)
        assert names.index("check_session") < names.index("accum") and "commit_accum" in names[names.index("accum"):]
    assert phase2["host_threads"] == 1 and h.session_held_bytes() == 0
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")


def test_a_forged_image_is_named_before_phase_2(run):
    """'another elf' of tests/test_session_balance.py: the verifier's image has one word the run's image has not"""
    from test_rv32im import ADDI
    want_json, _, n = run.reference(False)
    h = run.hal
    prog = _guest(25000)
    other_elf = elf_of(prog[:-4] + [ADDI(0, 0, 0)] + prog[-3:], 0x400)
    other_word, nop = (0x400 >> 2) + len(prog) - 4, ADDI(0, 0, 0)
    os.environ["R0H_SESSION_LANES"] = "2"
    h.set_session_enqueue(True)
    try:
        ses = h.session_begin(run.gc, run.elf, WORDS, segment_po2=PO2)
    finally:
        del os.environ["R0H_SESSION_LANES"]
        h.set_session_enqueue(False)
    try:
        for elf, honest in ((run.elf, True), (other_elf, False)):
            sb = r0.SessionBalance(run.blob, h)
            try:
                sb.add_session(ses)
                sb.add_verifier_side(elf, ses.journal)
                found = sb.report()
                if honest:
                    assert found == [] and sb.message() is None
                    continue
                assert any(source == r0.SESSION_SOURCE_IMAGE and values[1] == (-other_word) % r0.P and values[2] == (-(nop & 0xFFFF)) % r0.P and values[3] == (-(nop >> 16)) % r0.P
                           for source, _, _, _, _, values in found), found
                source, row, fraction, net, members, values = found[0]
                assert sb.message() == "session fraction %d does not balance: net %d over %d tuples, first in source %d at row %d, class (%s); %d classes in all" % (
                    fraction, net, members, source, row, ", ".join(str(v) for v in values), len(found))
            finally:
                sb.free()
        _, records = ses.records()
        assert ses.finish(records)[0].to_json() == want_json        # the handles took nothing from the session
    finally:
        ses.close()
    assert h.session_held_bytes() == 0
