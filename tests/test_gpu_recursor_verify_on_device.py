"""r0h_recursor_set_verify_on_device: lift, join and compress verify the seals they consume as one batch with the lane's device hashing
the Merkle openings, instead of on host threads beside the proof.  Nothing a caller can see may change: the root of r0h_compress is the
switch-off run's word for word, and a lift or join of an altered seal is refused with the switch-off message.  Shapes as in
profiles/r12/compress.md: the small trace guest at segment_po2 11 (2^16-row seals), recursion traces of 2^17 rows."""
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
    p.blob, p.rec_blob = _blob("trace"), _blob("recursion")
    p.gc = hal.load_circuit(p.blob, entry.code_object_path("trace"))
    p.elf = elf_of(_guest(300), 0x400)
    p.receipt, p.image_id, _ = hal.prove_elf(p.gc, p.elf, WORDS, segment_po2=11)
    p.seals, p.claims = [s for _, s in p.receipt.seals()], p.receipt.claims()
    assert len(p.seals) >= 2
    p.roots = {}
    for s in p.seals:
        size = r0.verify_seal(p.blob, s)[2]
        if size not in p.roots:
            p.roots[size] = hal.code_root(p.gc, size)
    p.rec = recursion.Recursor(hal, p.rec_blob, p.blob, entry.code_object_path("recursion"), po2=17, segment_roots=p.roots)
    yield p
    p.rec.close()
    p.gc.free()


def _message(fn):
    with pytest.raises(r0.R0HipError) as e:
        fn()
    return str(e.value)


def test_compress_gives_the_switch_off_root_word_for_word(hal, proved):
    p = proved
    off = p.rec.compress(p.receipt, lanes=2)
    hal.kernel_timing(True)
    before = hal.kernel_stats().get("merkle_climb_kernel", {"launches": 0})["launches"]
    p.rec.set_verify_on_device(True)
    try:
        on = p.rec.compress(p.receipt, lanes=2)
    finally:
        p.rec.set_verify_on_device(False)
    launches = hal.kernel_stats()["merkle_climb_kernel"]["launches"] - before
    hal.kernel_timing(False)
    assert np.array_equal(on.seal, off.seal) and bytes(on.claim) == bytes(off.claim) and np.array_equal(on.session, off.session)
    assert p.rec.verify(on)
    assert launches >= 1  # the leaves' batch ran on the recursor's own context (the joins' batches run on their lanes')


def test_lift_and_join_refuse_an_altered_seal_with_the_switch_off_message(proved):
    p = proved
    flipped = p.seals[0].copy()
    flipped[-9] ^= 1  # a word inside the last opening of the last query
    want = _message(lambda: p.rec.lift(flipped, p.claims[0]))
    assert "lift: the seal to be consumed does not verify" in want
    a, b = p.rec.lift(p.seals[0], p.claims[0]), p.rec.lift(p.seals[1], p.claims[1])
    altered = b.seal.copy()
    altered[-1] ^= 1
    bad_b = recursion.Node.from_parts(altered, b.claim, b.session)
    want_join = _message(lambda: p.rec.join(a, bad_b))
    assert "join (right): the seal to be consumed does not verify" in want_join
    joined_off = p.rec.join(a, b)
    p.rec.set_verify_on_device(True)
    try:
        assert _message(lambda: p.rec.lift(flipped, p.claims[0])) == want
        assert _message(lambda: p.rec.join(a, bad_b)) == want_join
        a_on = p.rec.lift(p.seals[0], p.claims[0])
        assert np.array_equal(a_on.seal, a.seal) and np.array_equal(a_on.session, a.session)
        assert np.array_equal(p.rec.join(a_on, b).seal, joined_off.seal)
    finally:
        p.rec.set_verify_on_device(False)
