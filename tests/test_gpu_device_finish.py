"""r0h_ctx_set_device_finish: with the switch on, r0h_proof_finish runs every step of a proof's second half -- ACCUM, CHECK, the openings
at z, DEEP, FRI, the queries -- on a transcript on the device and reads the seal words of all of them back at once; and it splits into
r0h_proof_finish_enqueue, which waits for nothing, and r0h_proof_finish_collect, which waits for the read-back.  The reference is the
host-transcript seal of the same witness, made with both switches off in the same process and accepted by the verifier: the seals are
the same words in every form of a proof, under both hash suites."""
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from hyperfridge_r0_amd import recursion
from conftest import ROOT, circuit_path

import evalcheck_circuits as hand

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden", "seal_tiny_po2_9_seed_1.npy")
SUITES = ["poseidon2", "sha-256"]
P = hand.P
# the kernels that run only with the switch on ...
OWN_KERNELS = ("ext_powers_kernel", "deep_points_kernel", "interpolate_regs_kernel", "deep_head_kernel", "divide_jobs_kernel", "divide_report_kernel")
# ... and the device transcript's, which r0h_ctx_set_device_transcript launches too (commit, commit_elems, draw, queries)
IOP_KERNELS = {"poseidon2": ("iop_commit_kernel", "iop_commit_elems_kernel", "iop_draw_kernel", "iop_queries_kernel"),
               "sha-256": ("sha256_iop_commit_kernel", "sha256_iop_commit_elems_kernel", "sha256_iop_draw_kernel", "sha256_iop_queries_kernel")}


class Bench:
    """a context per suite, the circuits loaded on each as they are asked for, and the host-transcript seal of every (suite, circuit,
    rows) made once, with both switches off"""

    def __init__(self):
        self.hal, self.gc, self.blob, self.seals = {}, {}, {}, {}
        for suite in SUITES:
            self.hal[suite] = r0.Hal(0)
            self.hal[suite].set_hashfn(suite)

    def circuit(self, suite, name):
        if name not in self.blob:
            self.blob[name] = np.fromfile(circuit_path(name), dtype=np.uint32)
        if (suite, name) not in self.gc:
            self.gc[suite, name] = self.hal[suite].load_circuit(self.blob[name], None if name == "tiny" else entry.code_object_path(name))
        return self.gc[suite, name]

    def witness(self, suite, name, po2):
        return self.hal[suite].witgen(self.circuit(suite, name), po2, 1)

    def host_seal(self, suite, name, po2):
        key = (suite, name, po2)
        if key not in self.seals:
            h = self.hal[suite]
            h.set_device_transcript(False)
            h.set_device_finish(False)
            code, data, glob = self.witness(suite, name, po2)
            self.seals[key] = h.prove_segment(self.circuit(suite, name), po2, code, data, glob)
            assert r0.verify_seal(self.blob[name], self.seals[key], hashfn=suite)[:3] == (0, "ok", po2)
            self.seals[key].setflags(write=False)
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


def prove(h, gc, po2, code, data, glob, form, top_levels=0, top_from=None, shrink=False):
    """one proof in the given form; top_levels: the two-phase form begun from the DATA tree's top (taken from `top_from`'s witness if
    given); shrink: r0h_proof_shrink between begin and finish"""
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
        if shrink:
            r0._check(r0.lib().r0h_proof_shrink(proof, None))
        return h.proof_finish(proof, accum)
    finally:
        cc.free()
        for b in bufs:
            b.free()


# ---- 1. seal equality: one FRI round (2^9: 32 final coefficients) and two (2^13), both suites, the three forms
@pytest.mark.parametrize("form", ["segment", "committed", "two-phase"])
@pytest.mark.parametrize("po2", [9, 13])
@pytest.mark.parametrize("name", ["tiny", "small"])
@pytest.mark.parametrize("suite", SUITES)
def test_the_seal_is_the_host_transcripts(bench, suite, name, po2, form):
    h, gc = bench.hal[suite], bench.circuit(suite, name)
    want = bench.host_seal(suite, name, po2)
    code, data, glob = bench.witness(suite, name, po2)
    h.set_device_finish(True)
    try:
        got = prove(h, gc, po2, code, data, glob, form)
    finally:
        h.set_device_finish(False)
    assert np.array_equal(got, want)
    root = h.code_root(gc, po2)
    assert r0.verify_seal(bench.blob[name], got, code_root=root, hashfn=suite)[:3] == (0, "ok", po2)  # r0h_verify_seal_bound
    if (suite, name, po2) == ("poseidon2", "tiny", 9):
        assert np.array_equal(got, np.load(GOLDEN))
    code.free(), data.free()


# ---- 2. bench: 2,824 powers of poly_mix (a table of twelve workgroups), 496 taps (eight workgroups of registers), 256 columns of mix powers
def test_bench_at_2_to_the_12_is_the_host_seal_and_verifies(bench):
    suite, po2 = "poseidon2", 12
    h, gc = bench.hal[suite], bench.circuit(suite, "bench")
    want = bench.host_seal(suite, "bench", po2)
    code, data, glob = bench.witness(suite, "bench", po2)
    h.set_device_finish(True)
    try:
        got = prove(h, gc, po2, code, data, glob, "committed")
    finally:
        h.set_device_finish(False)
    assert np.array_equal(got, want)
    assert r0.verify_seal(bench.blob["bench"], got, code_root=h.code_root(gc, po2), hashfn=suite)[:3] == (0, "ok", po2)
    code.free(), data.free()


# ---- 3. registers with more than two taps: the `taps` family, backs {0, 1, 2, 63} on column 0 of each group
@pytest.mark.parametrize("suite", SUITES)
def test_registers_of_four_taps_interpolate_to_the_hosts_words(bench, suite):
    """Random CODE / DATA / ACCUM words satisfy no constraint, so no verifier accepts either seal; the openings are honest all the same
    (every DEEP remainder is zero), both paths return a seal, and the two seals are the same words.  The four-tap registers go through
    interpolate_regs_kernel's general path (master polynomial, synthetic division per tap), which one- and two-tap registers barely touch."""
    h, po2 = bench.hal[suite], 9
    blob = hand.FAMILIES["taps"]()
    gc = h.load_circuit(blob)
    rng = np.random.default_rng(22)
    code, data, accum = (h.copy_from(rng.integers(0, P, size=2 << po2, dtype=np.uint32)) for _ in range(3))
    glob = rng.integers(0, P, size=hand.N_GLOBAL, dtype=np.uint32)
    seals = {}
    try:
        for on in (False, True):
            h.set_device_finish(on)
            proof, mix = h.proof_begin(gc, po2, code, data, glob)
            assert mix.size == hand.N_MIX
            seals[on] = h.proof_finish(proof, accum)
    finally:
        h.set_device_finish(False)
    assert seals[False].size > 0 and np.array_equal(seals[True], seals[False])
    for b in (code, data, accum):
        b.free()
    gc.free()


# ---- 4. the DATA tree kept as its top
@pytest.mark.parametrize("suite", SUITES)
def test_a_tree_kept_as_its_top_gives_the_same_seal_at_6_levels_and_at_1(bench, suite):
    h, gc = bench.hal[suite], bench.circuit(suite, "tiny")
    want = bench.host_seal(suite, "tiny", 9)
    code, data, glob = bench.witness(suite, "tiny", 9)
    h.set_device_finish(True)
    try:
        for levels in (6, 1):
            assert np.array_equal(prove(h, gc, 9, code, data, glob, "two-phase", top_levels=levels), want)
    finally:
        h.set_device_finish(False)
    code.free(), data.free()


def test_a_top_of_another_witness_fails_at_collect_as_it_always_did_and_leaves_the_context_usable(bench):
    h, gc = bench.hal["poseidon2"], bench.circuit("poseidon2", "tiny")
    code, data, glob = bench.witness("poseidon2", "tiny", 9)
    other = h.witgen(gc, 9, 2)
    text = r"r0h_proof_finish: tree top does not match the matrix under query \d+ \(row \d+\)"
    messages = []
    try:
        for on in (False, True):
            h.set_device_finish(on)
            with pytest.raises(r0.R0HipError, match=text) as err:
                prove(h, gc, 9, code, data, glob, "two-phase", top_levels=6, top_from=(other[1], other[2]))
            messages.append(str(err.value))
            assert np.array_equal(prove(h, gc, 9, code, data, glob, "two-phase", top_levels=6), np.load(GOLDEN))
        # the same proof in two calls: the enqueue succeeds, the error is the collect's
        cc = h.code_commit(gc, 9)
        first, _ = h.proof_begin(gc, 9, cc, other[1], other[2])
        top = h.proof_data_top(first, 9, 6)
        h.proof_abort(first)
        proof, mix = h.proof_begin(gc, 9, cc, data, glob, top=(top, 6))
        accum = h.accum(gc, 9, code, data, mix)
        h.proof_finish_enqueue(proof, accum)
        with pytest.raises(r0.R0HipError, match=text) as err:
            h.proof_finish_collect(proof)
        messages.append(str(err.value))
        assert np.array_equal(h.prove_segment(gc, 9, code, data, glob), np.load(GOLDEN))
        for b in (top, accum):
            b.free()
        cc.free()
    finally:
        h.set_device_finish(False)
    assert messages[0] == messages[1] == messages[2]
    for b in (code, data, other[0], other[1]):
        b.free()


# ---- 5. a shrunk proof
@pytest.mark.parametrize("suite", SUITES)
def test_a_shrunk_proof_gives_the_same_seal(bench, suite):
    h, gc = bench.hal[suite], bench.circuit(suite, "small")
    want = bench.host_seal(suite, "small", 9)
    code, data, glob = bench.witness(suite, "small", 9)
    h.set_device_finish(True)
    try:
        got = prove(h, gc, 9, code, data, glob, "two-phase", shrink=True)
        names = [n for n, _ in h.last_profile()]
    finally:
        h.set_device_finish(False)
    assert np.array_equal(got, want)
    assert "evaluate_data_again" in names  # the evaluations were given back and made again
    code.free(), data.free()


# ---- 6. wait counts
@pytest.mark.parametrize("po2", [9, 13, 17])
def test_proof_finish_waits_four_times_less_than_with_the_device_transcript_alone(po2):
    """r0h_ctx_set_device_transcript leaves steps 3-6 waiting four times (the ACCUM top, the CHECK top, the evaluations at z, the DEEP
    remainders), then the tail's read-back and the profile's close: six.  r0h_ctx_set_device_finish: the read-back and the close, two
    (the close is not folded into the read-back's wait).
    stage_h2d waits when the context's 8 MiB staging ring wraps, which would add one to either count.  The context is made here, for this
    test alone; what it stages before and in the two proofs is parameter blocks of `small` (a few KiB each: generator state, eval_check
    parameters, tables of taps and columns), a few hundred KiB in all whatever the row count -- nowhere near a wrap."""
    h = r0.Hal(0)
    blob = np.fromfile(circuit_path("small"), dtype=np.uint32)
    gc = h.load_circuit(blob, entry.code_object_path("small"))
    code, data, glob = h.witgen(gc, po2, 1)
    cc = h.code_commit(gc, po2)
    waits, seals = {}, {}
    try:
        for which in ("transcript", "finish"):
            h.set_device_transcript(which == "transcript")
            h.set_device_finish(which == "finish")
            proof, mix = h.proof_begin(gc, po2, cc, data, glob)
            accum = h.accum(gc, po2, code, data, mix)
            h.sync()
            before = h.blocking_waits()
            seals[which] = h.proof_finish(proof, accum)
            waits[which] = h.blocking_waits() - before
            accum.free()
    finally:
        h.set_device_transcript(False)
        h.set_device_finish(False)
    print("blocking waits of proof_finish at 2^%d rows: device_transcript %d, device_finish %d" % (po2, waits["transcript"], waits["finish"]))
    assert np.array_equal(seals["finish"], seals["transcript"])
    assert waits["transcript"] - waits["finish"] == 4
    assert waits["finish"] == 2
    cc.free(), code.free(), data.free(), gc.free()
    h.close()


@pytest.mark.parametrize("name,po2", [("tiny", 9), ("small", 13)])
@pytest.mark.parametrize("suite", SUITES)
def test_both_switches_on_is_the_device_finish(bench, suite, name, po2):
    """r0h_ctx_set_device_transcript and r0h_ctx_set_device_finish together: the transcript is handed over once, before step 3 (whatever
    the first switch says), so the seal is the host's and r0h_proof_finish waits for the read-back and the profile's close, twice.  A
    context of its own, as in the test above: nothing near a wrap of the staging ring."""
    want = bench.host_seal(suite, name, po2)
    h = r0.Hal(0)
    h.set_hashfn(suite)
    gc = h.load_circuit(bench.blob[name], None if name == "tiny" else entry.code_object_path(name))
    code, data, glob = h.witgen(gc, po2, 1)
    cc = h.code_commit(gc, po2)
    h.set_device_transcript(True)
    h.set_device_finish(True)
    proof, mix = h.proof_begin(gc, po2, cc, data, glob)
    accum = h.accum(gc, po2, code, data, mix)
    h.sync()
    before = h.blocking_waits()
    got = h.proof_finish(proof, accum)
    waits = h.blocking_waits() - before
    print("blocking waits of proof_finish with both switches on, %s at 2^%d under %s: %d" % (name, po2, suite, waits))
    assert np.array_equal(got, want)
    assert waits == 2
    accum.free(), cc.free(), code.free(), data.free(), gc.free()
    h.close()


# ---- 7. enqueue / collect
def test_one_thread_keeps_two_contexts_in_flight(bench):
    """begin A, begin B, enqueue A, enqueue B: neither context's count of blocking waits moves across the enqueues (fresh contexts, so
    no staging ring is near its wrap -- see the wait-count test).  Collect B, then A: the host seals."""
    suite, po2 = "poseidon2", 13
    want = bench.host_seal(suite, "small", po2)
    blob = bench.blob["small"]
    hs = [r0.Hal(0), r0.Hal(0)]
    held = []
    try:
        work = []
        for h in hs:
            h.set_device_finish(True)
            gc = h.load_circuit(blob, entry.code_object_path("small"))
            code, data, glob = h.witgen(gc, po2, 1)
            cc = h.code_commit(gc, po2)
            held += [code, data, cc, gc]
            work.append((h, gc, code, data, glob, cc))
        begun = []
        for h, gc, code, data, glob, cc in work:
            proof, mix = h.proof_begin(gc, po2, cc, data, glob)
            accum = h.accum(gc, po2, code, data, mix)
            held.insert(0, accum)
            begun.append((h, proof, accum))
        before = [h.blocking_waits() for h in hs]
        for h, proof, accum in begun:
            h.proof_finish_enqueue(proof, accum)
        assert [h.blocking_waits() for h in hs] == before
        got = {}
        for k in (1, 0):
            h, proof, _ = begun[k]
            got[k] = h.proof_finish_collect(proof)
            assert h.blocking_waits() == before[k] + 2  # the read-back, the profile's close
        assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
        assert [n for n, _ in hs[0].last_profile()][-2:] == ["fri_commit", "queries"]
    finally:
        for b in held:
            b.free()
        for h in hs:
            h.close()


def test_what_enqueue_and_collect_refuse_and_what_abort_leaves(bench):
    h, gc = bench.hal["poseidon2"], bench.circuit("poseidon2", "tiny")
    code, data, glob = bench.witness("poseidon2", "tiny", 9)
    cc = h.code_commit(gc, 9)
    try:
        # the switch off: enqueue is refused by name (and consumes the proof, as r0h_proof_finish's errors do)
        proof, mix = h.proof_begin(gc, 9, cc, data, glob)
        accum = h.accum(gc, 9, code, data, mix)
        with pytest.raises(r0.R0HipError, match="r0h_proof_finish_enqueue: .*r0h_ctx_set_device_finish"):
            h.proof_finish_enqueue(proof, accum)
        h.set_device_finish(True)
        # collect of a proof that was not enqueued is refused; the proof is still good
        proof, mix = h.proof_begin(gc, 9, cc, data, glob)
        with pytest.raises(r0.R0HipError, match="r0h_proof_finish_collect: the proof has not been enqueued"):
            h.proof_finish_collect(proof)
        h.proof_finish_enqueue(proof, accum)
        assert np.array_equal(h.proof_finish_collect(proof), np.load(GOLDEN))
        # abort of an enqueued proof: the context goes on to prove the golden seal, with the switch on and off
        proof, mix = h.proof_begin(gc, 9, cc, data, glob)
        h.proof_finish_enqueue(proof, accum)
        h.proof_abort(proof)
        assert np.array_equal(h.prove_segment(gc, 9, code, data, glob), np.load(GOLDEN))
        h.set_device_finish(False)
        assert np.array_equal(h.prove_segment(gc, 9, code, data, glob), np.load(GOLDEN))
        accum.free()
    finally:
        h.set_device_finish(False)
    cc.free(), code.free(), data.free()


# ---- 8. kernel stats
@pytest.mark.parametrize("suite", SUITES)
def test_the_profile_keeps_its_phases_and_the_new_kernels_run_only_with_the_switch_on(bench, suite):
    """`small` at 2^13 rows, two FRI rounds, one r0h_prove_segment.  With the switch on:
      ext_powers_kernel        6: the powers of poly_mix for eval_check, the per-column powers of the DEEP mix for each of the four
                                  groups (ACCUM, CODE, DATA, CHECK), the powers of the DEEP mix for the head
      deep_points_kernel, interpolate_regs_kernel, deep_head_kernel, divide_jobs_kernel, divide_report_kernel: 1 each
      commit                   4: the roots of ACCUM and CHECK, and of the two FRI rounds
      commit_elems             2: coeff_u, the final coefficients
      draw                     5: poly_mix, z, the DEEP mix, the two fold mixes
      queries                  1;  fri_fold_buf_kernel 2"""
    h, gc = bench.hal[suite], bench.circuit(suite, "small")
    code, data, glob = bench.witness(suite, "small", 13)
    want = {k: 1 for k in OWN_KERNELS}
    want["ext_powers_kernel"] = 6
    want.update(dict(zip(IOP_KERNELS[suite], (4, 2, 5, 1))))
    want["fri_fold_buf_kernel"] = 2
    phases = {}
    try:
        for on in (False, True):
            h.set_device_finish(on)
            h.kernel_timing(True)
            h.prove_segment(gc, 13, code, data, glob)
            stats = h.kernel_stats()
            h.kernel_timing(False)
            phases[on] = [n for n, _ in h.last_profile()]
            ran = {k: v["launches"] for k, v in stats.items() if v["launches"]}
            if on:
                assert {k: ran.get(k, 0) for k in want} == want
            else:
                assert not set(ran) & (set(OWN_KERNELS) | set(IOP_KERNELS["poseidon2"]) | set(IOP_KERNELS["sha-256"]) | {"fri_fold_buf_kernel"})
    finally:
        h.set_device_finish(False)
        h.kernel_timing(False)
    assert phases[True] == phases[False]  # the same names in the same order
    code.free(), data.free()


# ---- 9. a session with its image proof, and its compressed root
def test_a_session_its_image_proof_and_its_compressed_root_are_the_same_on_and_off(hal):
    """the small guest smoke() proves, in segments of 2^16 rows on two lanes (the default), the image circuit set: the switch reaches
    the helper contexts of the session's lanes and of the recursion's, and the image proof; receipt and root are the same bytes"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    blob, rec_blob = np.fromfile(circuit_path("trace"), dtype=np.uint32), np.fromfile(circuit_path("recursion"), dtype=np.uint32)
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    ic = hal.load_circuit(iblob, entry.code_object_path("image"))
    elf, words = elf_of(_guest(300), 0x400), [7, 0x01020304]
    receipts, roots = {}, {}
    hal.set_image_circuit(ic)
    try:
        for on in (False, True):
            hal.set_device_finish(on)
            receipts[on], image_id, _ = hal.prove_elf(gc, elf, words, segment_po2=11)
            seals = [s for _, s in receipts[on].seals()]
            assert len(seals) >= 2 and all(r0.verify_seal(blob, s)[2] == 16 for s in seals) and receipts[on].image_proof is not None
            if not on:
                cc = hal.code_commit(gc, 16)
                control = {16: cc.root()}
                cc.free()
                rec = recursion.Recursor(hal, rec_blob, blob, entry.code_object_path("recursion"), po2=17, segment_roots=control)
            roots[on] = rec.compress(receipts[on], lanes=2)
    finally:
        hal.set_device_finish(False)
        hal.set_image_circuit(None)
    assert receipts[True].to_json() == receipts[False].to_json()
    assert np.array_equal(receipts[True].image_proof, receipts[False].image_proof)
    assert receipts[True].verify(blob, control, None, elf=elf)[:2] == (0, "ok")
    assert receipts[True].verify_image(blob, control, iblob, image_id)[:2] == (0, "ok")
    assert np.array_equal(roots[True].seal, roots[False].seal) and bytes(roots[True].claim) == bytes(roots[False].claim)
    assert rec.verify(roots[True])
    rec.close()
    ic.free()
    gc.free()
