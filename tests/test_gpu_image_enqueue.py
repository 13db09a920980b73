"""The image proof in two calls (r0h_prove_image_enqueue / r0h_prove_image_collect): the seal is r0h_prove_image's word for word, the
image circuit's CODE group is committed once per (context, trace size, suite) and read by every later call, and what r0h_prove_image
refuses is refused at the enqueue.  The ELFs are two corner programs of tests/trace_corners.py at the rows their images need."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

import trace_corners as tcr

sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_session import elf_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def image(hal):
    blob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = hal.load_circuit(blob, entry.code_object_path("image"))
    yield blob, ic
    hal.set_device_finish(False)
    ic.free()


def challenges():
    rng = np.random.default_rng(27)
    return [rng.integers(1, r0.P, size=16).astype(np.uint32), np.full(16, r0.P - 1, dtype=np.uint32)]


@pytest.mark.parametrize("name", ["alu", "memory"])
def test_the_seal_is_prove_images(hal, image, name):
    blob, ic = image
    elf = elf_of(tcr.PROGRAMS[name](), tcr.BASE)
    po2 = r0.image_po2(elf)
    assert 9 <= po2 <= 15
    for ch in challenges():
        hal.set_device_finish(False)
        want = hal.prove_image(ic, elf, ch)
        assert r0.verify_seal(blob, want)[:3] == (0, "ok", po2)
        hal.set_device_finish(True)
        hal.prove_image_collect(hal.prove_image_enqueue(ic, elf, ch))      # (the first of these at a trace size commits CODE, and waits for it)
        before = hal.blocking_waits()
        handle = hal.prove_image_enqueue(ic, elf, ch)
        assert hal.blocking_waits() == before, "an enqueue behind the first waited for the stream"
        got = hal.prove_image_collect(handle)
        assert hal.blocking_waits() == before + 2      # the read-back and the close of the profile
        assert np.array_equal(got, want)
        assert np.array_equal(got[r0.IMAGE_GAMMA:r0.IMAGE_GAMMA + 16], ch)
    hal.set_device_finish(False)


def test_the_code_group_is_committed_once(hal):
    """hash_rows_kernel runs once per tree: CODE, DATA, ACCUM, CHECK and the FRI rounds.  r0h_prove_image commits CODE in every call;
    the two-call form commits it in the first call on a circuit alone."""
    blob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = hal.load_circuit(blob, entry.code_object_path("image"))      # (a circuit of its own: nothing is cached for it)
    elf = elf_of(tcr.PROGRAMS["control"](), tcr.BASE)
    ch = challenges()[0]

    def counted(fn):
        hal.kernel_timing(True)
        seal = fn()
        launches = hal.kernel_stats()["hash_rows_kernel"]["launches"]
        hal.kernel_timing(False)
        return seal, launches

    try:
        hal.set_device_finish(False)
        want, n_blocking = counted(lambda: hal.prove_image(ic, elf, ch))
        hal.set_device_finish(True)
        runs = [counted(lambda: hal.prove_image_collect(hal.prove_image_enqueue(ic, elf, ch))) for _ in range(3)]
        print("hash_rows_kernel launches: r0h_prove_image %d, the two-call form %s" % (n_blocking, [n for _, n in runs]))
        assert [n for _, n in runs] == [n_blocking, n_blocking - 1, n_blocking - 1]
        for seal, _ in runs:
            assert np.array_equal(seal, want)
    finally:
        hal.set_device_finish(False)
        hal.kernel_timing(False)
        ic.free()


def test_abort_of_an_image_proof_in_flight_then_a_full_one(hal, image):
    blob, ic = image
    elf = elf_of(tcr.PROGRAMS["memory"](), tcr.BASE)
    ch = challenges()[0]
    hal.set_device_finish(True)
    try:
        want = hal.prove_image_collect(hal.prove_image_enqueue(ic, elf, ch))      # (commits CODE at this trace size, if nothing has)
        before = hal.blocking_waits()
        handle = hal.prove_image_enqueue(ic, elf, ch)
        assert hal.blocking_waits() == before
        hal.prove_image_abort(handle)                                            # the stream is busy with the proof just enqueued
        assert hal.blocking_waits() == before + 1                                # the abort waited for it, once
        assert np.array_equal(hal.prove_image_collect(hal.prove_image_enqueue(ic, elf, ch)), want)
        assert r0.verify_seal(blob, want)[:3] == (0, "ok", r0.image_po2(elf))
    finally:
        hal.set_device_finish(False)


def test_refusals_at_the_enqueue(hal, image):
    blob, ic = image
    elf = elf_of(tcr.PROGRAMS["alu"](), tcr.BASE)
    ch = challenges()[0]
    bad = ch.copy()
    bad[11] = r0.P
    hal.set_device_finish(True)
    try:
        with pytest.raises(r0.R0HipError, match="r0h_prove_image_enqueue: challenge word 11 is not a canonical field word"):
            hal.prove_image_enqueue(ic, elf, bad)
        hal.set_device_finish(False)
        with pytest.raises(r0.R0HipError, match="r0h_prove_image_enqueue: the context has r0h_ctx_set_device_finish off"):
            hal.prove_image_enqueue(ic, elf, ch)
        hal.set_device_finish(True)
        tiny = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
        with pytest.raises(r0.R0HipError, match="r0h_prove_image_enqueue: the circuit is not the image circuit"):
            hal.prove_image_enqueue(tiny, elf, ch)
        tiny.free()
        got = hal.prove_image_collect(hal.prove_image_enqueue(ic, elf, ch))      # the context goes on
        assert r0.verify_seal(blob, got)[:3] == (0, "ok", r0.image_po2(elf))
    finally:
        hal.set_device_finish(False)
