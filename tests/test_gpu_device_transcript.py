"""r0h_ctx_set_device_transcript: with the switch on, r0h_proof_finish runs its FRI commitments and its queries on a transcript on the
device (csrc/iop.hip) and reads both steps' seal words back at once.  The seals are the seals of the host transcript word for word --
every form of a proof, both hash suites, one to three FRI rounds, trees kept as their tops, sessions and recursion over helper
contexts -- and the number of times the library waits for the stream drops by exactly 2 R + 4 for R FRI rounds."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from hyperfridge_r0_amd import recursion
from conftest import ROOT, circuit_path

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy")
SUITES = ["poseidon2", "sha-256"]
# rows -> FRI rounds: 2^9 one round and 32 final coefficients; 2^12 one round and exactly R0H_FRI_MIN_DEGREE left; 2^13 two; 2^17 three
ROUNDS = {9: 1, 12: 1, 13: 2, 17: 3}
NEW_KERNELS = {"poseidon2": ("iop_commit_kernel", "iop_commit_elems_kernel", "iop_draw_kernel", "iop_queries_kernel", "fri_fold_buf_kernel"),
               "sha-256": ("sha256_iop_commit_kernel", "sha256_iop_commit_elems_kernel", "sha256_iop_draw_kernel", "sha256_iop_queries_kernel", "fri_fold_buf_kernel")}


class Bench:
    """a context per suite, the two circuits loaded on each, and the host-transcript seal of every (suite, circuit, rows) made once"""

    def __init__(self):
        self.hal, self.gc, self.blob, self.seals = {}, {}, {}, {}
        for name in ("tiny", "small"):
            self.blob[name] = np.fromfile(circuit_path(name), dtype=np.uint32)
        for suite in SUITES:
            h = self.hal[suite] = r0.Hal(0)
            h.set_hashfn(suite)
            for name in ("tiny", "small"):
                self.gc[suite, name] = h.load_circuit(self.blob[name], entry.code_object_path(name) if name == "small" else None)

    def witness(self, suite, name, po2):
        return self.hal[suite].witgen(self.gc[suite, name], po2, 1)

    def host_seal(self, suite, name, po2):
        key = (suite, name, po2)
        if key not in self.seals:
            h = self.hal[suite]
            h.set_device_transcript(False)
            code, data, glob = self.witness(suite, name, po2)
            self.seals[key] = h.prove_segment(self.gc[suite, name], po2, code, data, glob)
            assert r0.verify_seal(self.blob[name], self.seals[key], hashfn=suite)[:3] == (0, "ok", po2)
            code.free(), data.free()
        return self.seals[key]

    def close(self):
        for g in self.gc.values():
            g.free()
        for h in self.hal.values():
            h.close()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


def prove(h, gc, po2, code, data, glob, form, top_levels=0, top_from=None):
    """one proof in the given form; top_levels: the two-phase form begun from the DATA tree's top (taken from `top_from`'s witness if given)"""
    if form == "segment":
        return h.prove_segment(gc, po2, code, data, glob)
    cc = h.code_commit(gc, po2)
    bufs = []
    try:
        if form == "committed":
            return h.prove_segment(gc, po2, cc, data, glob)
        top = None
        if top_levels:
            src_data, src_glob = top_from if top_from is not None else (data, glob)
            first, _ = h.proof_begin(gc, po2, cc, src_data, src_glob)
            top = h.proof_data_top(first, po2, top_levels)
            bufs.append(top)
            h.proof_abort(first)
        proof, mix = h.proof_begin(gc, po2, cc, data, glob, top=(top, top_levels) if top is not None else None)
        accum = h.accum(gc, po2, code, data, mix)
        bufs.append(accum)
        return h.proof_finish(proof, accum)
    finally:
        cc.free()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("form", ["segment", "committed", "two-phase"])
@pytest.mark.parametrize("po2", sorted(ROUNDS))
@pytest.mark.parametrize("name", ["tiny", "small"])
@pytest.mark.parametrize("suite", SUITES)
def test_the_seal_is_the_host_transcripts(bench, suite, name, po2, form):
    h, gc = bench.hal[suite], bench.gc[suite, name]
    want = bench.host_seal(suite, name, po2)
    code, data, glob = bench.witness(suite, name, po2)
    h.set_device_transcript(True)
    try:
        got = prove(h, gc, po2, code, data, glob, form)
    finally:
        h.set_device_transcript(False)
    assert np.array_equal(got, want)
    root = h.code_root(gc, po2)
    assert r0.verify_seal(bench.blob[name], got, code_root=root, hashfn=suite)[:3] == (0, "ok", po2)  # r0h_verify_seal_bound
    if (suite, name, po2) == ("poseidon2", "tiny", 9):
        assert np.array_equal(got, np.load(GOLDEN))
    code.free(), data.free()


@pytest.mark.parametrize("suite", SUITES)
def test_a_tree_kept_as_its_top_gives_the_same_seal_at_6_levels_and_at_1(bench, suite):
    h, gc = bench.hal[suite], bench.gc[suite, "tiny"]
    want = bench.host_seal(suite, "tiny", 9)
    code, data, glob = bench.witness(suite, "tiny", 9)
    h.set_device_transcript(True)
    try:
        for levels in (6, 1):
            assert np.array_equal(prove(h, gc, 9, code, data, glob, "two-phase", top_levels=levels), want)
    finally:
        h.set_device_transcript(False)
    code.free(), data.free()


def test_a_top_of_another_witness_fails_as_it_always_did_and_leaves_the_context_usable(bench):
    h, gc = bench.hal["poseidon2"], bench.gc["poseidon2", "tiny"]
    code, data, glob = bench.witness("poseidon2", "tiny", 9)
    other = h.witgen(gc, 9, 2)
    text = r"r0h_proof_finish: tree top does not match the matrix under query \d+ \(row \d+\)"
    messages = []
    try:
        for on in (False, True):
            h.set_device_transcript(on)
            with pytest.raises(r0.R0HipError, match=text) as err:
                prove(h, gc, 9, code, data, glob, "two-phase", top_levels=6, top_from=(other[1], other[2]))
            messages.append(str(err.value))
            assert np.array_equal(prove(h, gc, 9, code, data, glob, "two-phase", top_levels=6), np.load(GOLDEN))
            assert np.array_equal(h.prove_segment(gc, 9, code, data, glob), np.load(GOLDEN))
    finally:
        h.set_device_transcript(False)
    assert messages[0] == messages[1]
    for b in (code, data, other[0], other[1]):
        b.free()


@pytest.mark.parametrize("po2", [9, 13, 17])
def test_proof_finish_waits_2r_plus_4_times_less(bench, po2):
    """host transcript: a read-back per FRI top (R), the final coefficients (1), a packed opening per tree (4 + R) = 2 R + 5 in the two
    steps; device transcript: one.  Steps 3-6 and the profile's close wait the same number of times in both."""
    h, gc = bench.hal["poseidon2"], bench.gc["poseidon2", "small"]
    code, data, glob = bench.witness("poseidon2", "small", po2)
    cc = h.code_commit(gc, po2)
    waits, seals = {}, {}
    try:
        for on in (False, True):
            h.set_device_transcript(on)
            proof, mix = h.proof_begin(gc, po2, cc, data, glob)
            accum = h.accum(gc, po2, code, data, mix)
            h.sync()
            before = h.blocking_waits()
            seals[on] = h.proof_finish(proof, accum)
            waits[on] = h.blocking_waits() - before
            accum.free()
    finally:
        h.set_device_transcript(False)
    print("blocking waits of proof_finish at 2^%d rows: host transcript %d, device transcript %d" % (po2, waits[False], waits[True]))
    assert np.array_equal(seals[True], seals[False])
    assert waits[False] - waits[True] == 2 * ROUNDS[po2] + 4
    before = h.blocking_waits()
    h.sync()
    assert h.blocking_waits() == before + 1
    cc.free(), code.free(), data.free()


@pytest.mark.parametrize("suite", SUITES)
def test_the_profile_keeps_its_phases_and_the_new_kernels_run_only_with_the_switch_on(bench, suite):
    h, gc = bench.hal[suite], bench.gc[suite, "small"]
    code, data, glob = bench.witness(suite, "small", 13)
    try:
        for on in (False, True):
            h.set_device_transcript(on)
            h.kernel_timing(True)
            h.prove_segment(gc, 13, code, data, glob)
            stats = h.kernel_stats()
            h.kernel_timing(False)
            names = [n for n, _ in h.last_profile()]
            assert "fri_commit" in names and "queries" in names and names.index("fri_commit") < names.index("queries")
            ran = {k for k, v in stats.items() if v["launches"]}
            if on:
                assert set(NEW_KERNELS[suite]) <= ran
                assert stats[NEW_KERNELS[suite][0]]["launches"] == 2 and stats["fri_fold_buf_kernel"]["launches"] == 2  # two FRI rounds
                assert stats[NEW_KERNELS[suite][1]]["launches"] == 1 and stats[NEW_KERNELS[suite][3]]["launches"] == 1
            else:
                assert not ran & (set(NEW_KERNELS["poseidon2"]) | set(NEW_KERNELS["sha-256"]))
    finally:
        h.set_device_transcript(False)
        h.kernel_timing(False)
    code.free(), data.free()


def test_a_session_and_its_compressed_root_are_the_same_on_and_off(hal):
    """the small guest smoke() proves, in segments of 2^16 rows on two lanes (the default): the switch reaches the helper contexts of the
    session's lanes and of the recursion's; receipt and root are the same bytes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    blob, rec_blob = np.fromfile(circuit_path("trace"), dtype=np.uint32), np.fromfile(circuit_path("recursion"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    elf, words = elf_of(_guest(300), 0x400), [7, 0x01020304]
    receipts, roots = {}, {}
    try:
        for on in (False, True):
            hal.set_device_transcript(on)
            receipts[on], _, _ = hal.prove_elf(gc, elf, words, segment_po2=11)
            seals = [s for _, s in receipts[on].seals()]
            assert len(seals) >= 2 and all(r0.verify_seal(blob, s)[2] == 16 for s in seals)
            if not on:
                cc = hal.code_commit(gc, 16)
                control = {16: cc.root()}
                cc.free()
                rec = recursion.Recursor(hal, rec_blob, blob, entry.code_object_path("recursion"), po2=17, segment_roots=control)
            roots[on] = rec.compress(receipts[on], lanes=2)
    finally:
        hal.set_device_transcript(False)
    assert receipts[True].to_json() == receipts[False].to_json()
    assert receipts[True].verify(blob, control, None, elf=elf)[:2] == (0, "ok")
    assert np.array_equal(roots[True].seal, roots[False].seal) and bytes(roots[True].claim) == bytes(roots[False].claim)
    assert rec.verify(roots[True])
    rec.close()
    gc.free()
