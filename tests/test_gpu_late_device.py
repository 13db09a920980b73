"""The late public inputs on the device transcript (r0h_proof_late_device) and the log-derivative steps that read their challenges and
their mix from device buffers (r0h_logup_totals_device, r0h_accum_public_device), through the harness:

    proof_begin_committed -> totals (device form) -> proof_late_device -> accumulation (device form) -> proof_finish_enqueue / _collect

gives, word for word, the seal of the host-late path (r0h_logup_totals -> r0h_proof_late -> r0h_accum_public -> r0h_proof_finish, every
switch off), and the product's host verifier accepts it bound to the control root.  The cases: one 2^16-row trace-circuit segment under
Poseidon2 and under SHA-256 (under Poseidon2 also against the oracle's seal of the same witness: the oracle is the reference, the
host-late path the second witness); the image circuit at the rows the smallest guest's image needs, against r0h_prove_image's seal; a
circuit without late inputs (tiny, 2^9 rows) as far as the mix draw.  Then the refusals, each by its message."""
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
SIZE = r0.TRACE_MIN_PO2  # 2^16 rows: the lookup tables' size
N_EARLY = r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS


class Segment:
    """one small guest run: its only segment's DATA witness and early public inputs at 2^16 rows, under a challenge of the test's own
    (a segment proved alone takes any sixteen canonical words), and the ELF for the image circuit's case"""

    def __init__(self):
        self.blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
        self.elf, words = elf_of(_guest(300), 0x400), [7, 0x01020304]
        vm = r0.Vm()
        vm.load_elf(self.elf)
        vm.set_input(words)
        assert vm.run(segment_po2=16, keep_trace=True, boundary_rows=True) == (0, 0)
        self.data, glob = vm.trace_witness(0, SIZE, claim_globals=vm.claims()[0].globals())
        self.gamma = np.random.default_rng(23).integers(1, r0.P, size=16).astype(np.uint32)
        self.glob = np.asarray(glob, dtype=np.uint32).copy()
        self.glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = self.gamma
        self.glob[r0.TRACE_SUM:r0.TRACE_SUM + 4] = 0


@pytest.fixture(scope="module")
def segment():
    return Segment()


def host_late(h, gc, po2, cc, code, data, glob, n_late):
    """the existing path, every switch off: (seal, public inputs with the totals, mix)"""
    h.set_device_finish(False)
    full = h.logup_totals(gc, po2, code, data, glob)
    proof, _ = h.proof_begin(gc, po2, cc, data, full)
    mix = h.proof_late(proof, gc, full[gc.n_global - n_late:])
    accum = h.accum_public(gc, po2, code, data, full, mix)
    try:
        return h.proof_finish(proof, accum), full, mix
    finally:
        accum.free()


def device_late(h, gc, po2, cc, code, data, glob, n_late, spoil=None):
    """the new path: nothing of the totals, the late inputs or the mix is on the host before the collect.  -> (seal, device public
    inputs read back after the collect, device mix read back after it).  spoil(globals Buf): called between the totals and the late step."""
    h.set_device_finish(True)
    gbuf, mbuf = h.copy_from(glob), h.alloc(max(gc.n_mix, 1))
    accum = None
    try:
        proof, _ = h.proof_begin(gc, po2, cc, data, glob)
        waits = h.blocking_waits()
        h.logup_totals_device(gc, po2, code, data, gbuf)
        if spoil is not None:
            spoil(gbuf)
            waits = h.blocking_waits()      # (the test's own upload waits)
        late = gbuf.slice(gc.n_global - n_late, n_late)
        try:
            h.proof_late_device(proof, late, mbuf)
            accum = h.accum_public_device(gc, po2, code, data, gbuf, mbuf)
            h.proof_finish_enqueue(proof, accum)
            assert h.blocking_waits() == waits, "a step of the device path waited for the stream"
            seal = h.proof_finish_collect(proof)
            assert h.blocking_waits() == waits + 2      # the collect's read-back and the close of the profile
        finally:
            late.free()
        return seal, gbuf.to_host(), mbuf.to_host()[:gc.n_mix]
    finally:
        h.set_device_finish(False)
        for b in (gbuf, mbuf, accum):
            if b is not None:
                b.free()


@pytest.mark.parametrize("suite", ["poseidon2", "sha-256"])
def test_a_trace_segment_gives_the_seal_of_the_host_late_path(segment, orc, suite):
    h = r0.Hal(0)
    h.set_hashfn(suite)
    gc = h.load_circuit(segment.blob, entry.code_object_path("trace"))
    code, synthetic, _ = h.witgen(gc, SIZE, 0)
    synthetic.free()
    cc, data = h.code_commit(gc, SIZE, code), h.copy_from(segment.data)
    try:
        want, full, mix = host_late(h, gc, SIZE, cc, code, data, segment.glob, r0.TRACE_LATE_GLOBALS)
        got, dev_glob, dev_mix = device_late(h, gc, SIZE, cc, code, data, segment.glob, r0.TRACE_LATE_GLOBALS)
        assert np.array_equal(dev_glob, full) and np.any(full[r0.TRACE_SUM:r0.TRACE_SUM + 4])  # the session sum was left in the device copy
        assert np.array_equal(dev_mix, mix)
        assert np.array_equal(got, want)
        assert np.array_equal(got[:r0.TRACE_GLOBALS], full)        # the late words came home in the seal's opening block
        assert r0.verify_seal(segment.blob, got, code_root=cc.root(), hashfn=suite)[:3] == (0, "ok", SIZE)
        if suite == "poseidon2":  # the reference
            oc = orc.circuit(segment.blob)
            assert np.array_equal(got, oc.prove(SIZE, oc.witgen(SIZE, 0)[0], segment.data, full))
    finally:
        for b in (cc, data, code, gc):
            b.free()
        h.close()


def test_the_image_circuit_gives_the_seal_of_prove_image(hal, segment):
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = hal.load_circuit(iblob, entry.code_object_path("image"))
    po2 = r0.image_po2(segment.elf)
    assert 9 <= po2 <= 15
    idata, iglob = r0.image_witness(segment.elf, po2)
    iglob = np.asarray(iglob, dtype=np.uint32).copy()
    iglob[r0.IMAGE_GAMMA:r0.IMAGE_GAMMA + 16] = segment.gamma
    iglob[r0.IMAGE_SUM:r0.IMAGE_SUM + 4] = 0
    n_late = r0.IMAGE_GLOBALS - r0.IMAGE_GAMMA
    code, synthetic, _ = hal.witgen(ic, po2, 0)
    synthetic.free()
    cc, data = hal.code_commit(ic, po2, code), hal.copy_from(idata.reshape(-1))
    try:
        hal.set_device_finish(False)
        want = hal.prove_image(ic, segment.elf, segment.gamma)
        got, dev_glob, _ = device_late(hal, ic, po2, cc, code, data, iglob, n_late)
        assert np.array_equal(got, want) and np.array_equal(dev_glob, want[:r0.IMAGE_GLOBALS])
        assert r0.verify_seal(iblob, got, code_root=cc.root())[:3] == (0, "ok", po2)
    finally:
        for b in (cc, data, code, ic):
            b.free()


def test_without_late_inputs_the_device_draws_the_mix_the_host_drew(hal):
    gc = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
    code, data, glob = hal.witgen(gc, 9, 1)
    mbuf = hal.alloc(gc.n_mix)
    hal.set_device_finish(True)
    try:
        proof, mix = hal.proof_begin(gc, 9, code, data, glob)
        assert gc.n_mix >= 4 and np.any(mix)
        hal.proof_late_device(proof, None, mbuf)
        assert np.array_equal(mbuf.to_host(), mix)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the accumulation mix has been drawn already"):
            hal.proof_late_device(proof, None, mbuf)
        hal.proof_abort(proof)
    finally:
        hal.set_device_finish(False)
        for b in (code, data, mbuf, gc):
            b.free()


def test_refusals(hal, segment):
    gc = hal.load_circuit(segment.blob, entry.code_object_path("trace"))
    code, synthetic, _ = hal.witgen(gc, SIZE, 0)
    synthetic.free()
    cc, data = hal.code_commit(gc, SIZE, code), hal.copy_from(segment.data)
    n_late = r0.TRACE_LATE_GLOBALS

    def not_canonical(gbuf):
        gbuf.upload(np.array([r0.P], dtype=np.uint32), N_EARLY + 17)   # the second word of the session sum

    try:
        # a word that is no field element: found on the device, reported at the collect by its index
        with pytest.raises(r0.R0HipError, match="late public input 17 is not canonical"):
            device_late(hal, gc, SIZE, cc, code, data, segment.glob, n_late, spoil=not_canonical)
        hal.set_device_finish(True)
        gbuf, mbuf = hal.copy_from(hal.logup_totals(gc, SIZE, code, data, segment.glob)), hal.alloc(gc.n_mix)
        proof, _ = hal.proof_begin(gc, SIZE, cc, data, segment.glob)
        short, late = gbuf.slice(N_EARLY, n_late - 1), gbuf.slice(N_EARLY, n_late)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the late buffer holds 19 words, the circuit has 20 late public inputs"):
            hal.proof_late_device(proof, short, mbuf)
        hal.set_device_finish(False)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: .*r0h_ctx_set_device_finish off"):
            hal.proof_late_device(proof, late, mbuf)
        hal.set_device_finish(True)
        hal.proof_late_device(proof, late, mbuf)        # the refusals left the proof as it was
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the accumulation mix has been drawn already"):
            hal.proof_late_device(proof, late, mbuf)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late: the accumulation mix has been drawn already"):
            hal.proof_late(proof, gc, segment.glob[N_EARLY:])
        hal.proof_abort(proof)
        # a context whose suite changed since the begin
        proof, _ = hal.proof_begin(gc, SIZE, cc, data, segment.glob)
        hal.set_hashfn("sha-256")
        try:
            with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the proof was begun under the poseidon2 hash suite, its context is now on sha-256"):
                hal.proof_late_device(proof, late, mbuf)
        finally:
            hal.proof_abort(proof)
            hal.set_hashfn("poseidon2")
        for b in (short, late, gbuf, mbuf):
            b.free()
        # the device form of the accumulation is the log-derivative argument's
        tiny = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
        with pytest.raises(r0.R0HipError, match="r0h_accum_public_device: the circuit has no log-derivative argument"):
            tc, td, tg = hal.witgen(tiny, 9, 1)
            g, m = hal.copy_from(np.concatenate([tg, np.zeros(4, np.uint32)])), hal.alloc(max(tiny.n_mix, 1))
            try:
                hal.accum_public_device(tiny, 9, tc, td, g, m)
            finally:
                for b in (tc, td, g, m, tiny):
                    b.free()
    finally:
        hal.set_device_finish(False)
        for b in (cc, data, code, gc):
            b.free()
