"""r0h_ctx_set_session_enqueue_begin: a trace-circuit session driven by its calling thread in both phases.  The guest is the corner
program that loops long enough to be cut (tests/trace_corners.py lookup_program: three segments of 2^16 rows).  The receipt is the default
form's byte for byte with one lane and with two, with the image proof, with a device limit that evicts every segment but the first, and
with that limit and tree tops kept at 6 levels; it verifies with the ELF and with the image id alone.  Phase 1 starts no lane thread and
waits once per lane (the gathered roots' read-back) and once per evicted segment (its root, before it gives up its proof); phase 2 is
r0h_ctx_set_session_enqueue's."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import circuit_path

import trace_corners as tcr

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
        self.elf = elf_of(tcr.lookup_program(25000), tcr.BASE)      # 150,000 cycles and their boundary rows: more than two segments of 2^16 rows
        self.roots = {PO2: r0.control_root_host(self.blob, PO2)}
        self.made = {}
        # the image circuit's CODE group is committed once per context and trace size, by the first two-call image proof (a wait of its
        # own): made here, so that every session below finds it
        hal.set_device_finish(True)
        hal.prove_image_collect(hal.prove_image_enqueue(self.ic, self.elf, np.arange(1, 17, dtype=np.uint32)))
        hal.set_device_finish(False)

    def prove(self, form, lanes="2", image=False, limit=0, tops=0):
        """form: "default", "enqueue" (r0h_ctx_set_session_enqueue) or "begin" (r0h_ctx_set_session_enqueue_begin)"""
        h = self.hal
        os.environ["R0H_SESSION_LANES"] = lanes
        h.set_session_enqueue(form == "enqueue")
        h.set_session_enqueue_begin(form == "begin")
        h.set_image_circuit(self.ic if image else None)
        h.set_session_device_limit(limit)
        h.set_session_tree_tops(tops)
        try:
            receipt, image_id, _ = h.prove_elf(self.gc, self.elf, WORDS, segment_po2=PO2)
        finally:
            del os.environ["R0H_SESSION_LANES"]
            h.set_session_enqueue(False)
            h.set_session_enqueue_begin(False)
            h.set_image_circuit(None)
            h.set_session_device_limit(0)
            h.set_session_tree_tops(0)
        return receipt, image_id, h.last_session_phase1(), h.last_session_phase2(), h.last_session_device()

    def reference(self, form, image):
        """the default form and r0h_ctx_set_session_enqueue's, two lanes, made once each"""
        if (form, image) not in self.made:
            receipt, image_id, phase1, phase2, _ = self.prove(form, image=image)
            self.made[form, image] = (receipt.to_json(), image_id, len(receipt.seals()), phase1, phase2)
        return self.made[form, image]

    def close(self):
        self.gc.free()
        self.ic.free()


@pytest.fixture(scope="module")
def run(hal):
    r = Run(hal)
    yield r
    r.close()


def own_waits(phase2):
    return phase2["blocking_waits"] - phase2["ring_waits"] - phase2["replay_and_image_waits"]


def check(run, receipt, image_id, image):
    assert receipt.verify(run.blob, run.roots, None, elf=run.elf)[:2] == (0, "ok")
    if image:
        assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")
    assert run.hal.session_held_bytes() == 0


@pytest.mark.parametrize("image", [False, True], ids=["segments alone", "with the image proof"])
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_the_receipt_is_the_default_forms_and_no_lane_thread_made_it(run, lanes, image):
    want_json, want_id, n, default1, _ = run.reference("default", image)
    assert n >= 3 and default1["host_threads"] == 1 and default1["segments"] == n      # (two lanes: one thread beside the caller's)
    _, _, _, _, enqueue2 = run.reference("enqueue", image)
    receipt, image_id, phase1, phase2, _ = run.prove("begin", lanes=lanes, image=image)
    assert receipt.to_json() == want_json and image_id == want_id
    print("phase 1 %s, phase 2 %s; the default form's phase 1 %s" % (phase1, phase2, default1))
    # phase 1, by design (begin_enqueued): no thread started; nothing waits but the read-back of the gathered roots, once per lane
    # (every lane has a segment: they are dealt round robin, and there are more segments than lanes); no segment is evicted or lean
    assert phase1 == {"host_threads": 0, "blocking_waits": int(lanes), "segments": n, "evictions": 0}
    # phase 2 is r0h_ctx_set_session_enqueue's: one thread, per segment the collect's read-back and the close of the lane's profile
    assert phase2["host_threads"] == enqueue2["host_threads"] == 1
    assert own_waits(phase2) == own_waits(enqueue2) == 2 * n
    # the image proof waits twice on its helper context (the read-back, the profile's close); the blocking one waited more often
    assert phase2["replay_and_image_waits"] == (2 if image else 0)
    assert enqueue2["replay_and_image_waits"] > phase2["replay_and_image_waits"] or not image
    check(run, receipt, image_id, image)


@pytest.mark.parametrize("tops", [0, 6], ids=["hashing replay", "replay from the tree top"])
@pytest.mark.parametrize("lanes", ["1", "2"])
def test_every_segment_but_one_is_evicted_and_replayed_without_blocking(run, lanes, tops):
    want_json, want_id, n, _, _ = run.reference("default", True)
    _, _, _, _, roomy = run.prove("default", image=True, limit=1 << 50)      # (a limit nothing reaches: the count is kept)
    limit = roomy["peak_counted_bytes"] // n + 1                           # room for one segment (they all have 2^16 rows)
    receipt, image_id, phase1, phase2, dev = run.prove("begin", lanes=lanes, image=True, limit=limit, tops=tops)
    assert dev["evicted"] == dev["replayed"] == n - 1
    assert run.hal.last_session_tree_tops()["replayed_from_top"] == (n - 1 if tops else 0)
    assert receipt.to_json() == want_json and image_id == want_id
    print("phase 1 %s, phase 2 %s" % (phase1, phase2))
    # phase 1: the gathered words' read-back once per lane, and per evicted segment its root's read-back (r0h_proof_data_root) before it
    # gives up its proof -- the abort behind it finds the stream drained, the tree top was copied device to device in front of it
    assert phase1 == {"host_threads": 0, "blocking_waits": int(lanes) + (n - 1), "segments": n, "evictions": n - 1}
    # phase 2: per segment two waits as ever; per replayed segment one read-back of the root it committed, behind its seal; the image
    # proof's two
    assert phase2["host_threads"] == 1 and own_waits(phase2) == 2 * n
    assert phase2["replay_and_image_waits"] == (n - 1) + 2
    check(run, receipt, image_id, True)


@pytest.mark.parametrize("name", ["alu", "memory"])
def test_an_uncut_corner_program_leaves_a_lane_without_a_segment(run, name):
    """one segment, two lanes: the second lane has nothing to read back, so phase 1 waits once"""
    h = run.hal
    elf = elf_of(tcr.PROGRAMS[name](), tcr.BASE)
    os.environ["R0H_SESSION_LANES"] = "2"
    h.set_image_circuit(run.ic)
    try:
        want, want_id, _ = h.prove_elf(run.gc, elf, WORDS, segment_po2=PO2)
        assert len(want.seals()) == 1
        h.set_session_enqueue_begin(True)
        h.prove_elf(run.gc, elf, WORDS, segment_po2=PO2)      # (the image circuit's CODE group at this image's size, if no session has made it)
        receipt, image_id, _ = h.prove_elf(run.gc, elf, WORDS, segment_po2=PO2)
    finally:
        del os.environ["R0H_SESSION_LANES"]
        h.set_session_enqueue_begin(False)
        h.set_image_circuit(None)
    phase1, phase2 = h.last_session_phase1(), h.last_session_phase2()
    assert receipt.to_json() == want.to_json() and image_id == want_id
    assert phase1 == {"host_threads": 0, "blocking_waits": 1, "segments": 1, "evictions": 0}
    assert phase2["host_threads"] == 1 and own_waits(phase2) == 2 and phase2["replay_and_image_waits"] == 2
    assert receipt.verify(run.blob, run.roots, None, elf=elf)[:2] == (0, "ok")
    assert receipt.verify_image(run.blob, run.roots, run.iblob, image_id)[:2] == (0, "ok")


def test_the_environment_sets_the_default_and_the_context_overrides_it(run):
    want_json, _, n, _, _ = run.reference("default", False)
    h = r0.Hal(0)       # a context that was never told
    gc = h.load_circuit(run.blob, entry.code_object_path("trace"))
    os.environ["R0H_SESSION_ENQUEUE_BEGIN"] = "1"
    try:
        receipt, _, _ = h.prove_elf(gc, run.elf, WORDS, segment_po2=PO2)
        assert h.last_session_phase1()["host_threads"] == 0 and h.last_session_phase2()["host_threads"] == 1 and receipt.to_json() == want_json
        h.set_session_enqueue_begin(False)
        receipt, _, _ = h.prove_elf(gc, run.elf, WORDS, segment_po2=PO2)
        assert h.last_session_phase1()["host_threads"] == 1 and h.last_session_phase2()["host_threads"] == 2 and receipt.to_json() == want_json
    finally:
        del os.environ["R0H_SESSION_ENQUEUE_BEGIN"]
        gc.free()
        h.close()


def test_a_sharded_session_refuses_the_switch(run):
    h = run.hal
    h.set_session_enqueue_begin(True)
    try:
        with pytest.raises(r0.R0HipError, match="r0h_session_begin: r0h_ctx_set_session_enqueue_begin is on and this is part 0 of 2"):
            h.session_begin(run.gc, run.elf, WORDS, segment_po2=PO2, part=0, parts=2)
    finally:
        h.set_session_enqueue_begin(False)
