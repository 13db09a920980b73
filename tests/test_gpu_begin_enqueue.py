"""A proof's first half enqueued: the transcript handed over to the device before the DATA commitment
(r0h_proof_begin_committed[_top]_enqueue), the DATA root gathered on the device (r0h_proof_data_root_device), the synthetic
accumulation from device mix words (r0h_accum_mixbuf) and a whole proof submitted and collected
(r0h_prove_segment_committed_enqueue / r0h_prove_segment_collect).  The reference is the seal of the blocking form of the same witness,
made with every switch off in the same process and accepted by the verifiers: the seals are the same words.

Sizes: `tiny` at 2^9 rows (one FRI round, a top layer that is the whole level), `small` at 2^13 (two rounds), the trace circuit at its
minimum of 2^16 rows."""
import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import circuit_path

import trace_corners as tcr

pytestmark = pytest.mark.gpu
SUITES = ["poseidon2", "sha-256"]
SIZES = [("tiny", 9), ("small", 13)]
P = r0.P
TRACE_PO2 = r0.TRACE_MIN_PO2
N_EARLY = r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS


class Bench:
    """a context per suite; per (suite, circuit, rows) the circuit, its kept CODE commitment, one witness, and the seal of the blocking
    form (r0h_prove_segment_committed, both device switches off), made once and left unchanged"""

    def __init__(self):
        self.hal, self.blob, self.made, self.finish = {}, {}, {}, False
        for suite in SUITES:
            self.hal[suite] = r0.Hal(0)
            self.hal[suite].set_hashfn(suite)

    def case(self, suite, name, po2):
        key = (suite, name, po2)
        if key not in self.made:
            h = self.hal[suite]
            if name not in self.blob:
                self.blob[name] = np.fromfile(circuit_path(name), dtype=np.uint32)
            gc = next((c["gc"] for k, c in self.made.items() if k[:2] == key[:2]), None)
            if gc is None:
                gc = h.load_circuit(self.blob[name], None if name == "tiny" else entry.code_object_path(name))
            code, data, glob = h.witgen(gc, po2, 1)
            cc = h.code_commit(gc, po2)
            h.set_device_finish(False)
            seal = h.prove_segment(gc, po2, cc, data, glob)
            h.set_device_finish(self.finish)
            seal.setflags(write=False)
            self.made[key] = dict(h=h, gc=gc, cc=cc, code=code, data=data, glob=glob, seal=seal, blob=self.blob[name], po2=po2, suite=suite)
        return self.made[key]

    def set_finish(self, on):
        self.finish = on
        for h in self.hal.values():
            h.set_device_finish(on)

    def close(self):
        for c in self.made.values():
            for b in (c["cc"], c["code"], c["data"]):
                b.free()
        for gc in {id(c["gc"]): c["gc"] for c in self.made.values()}.values():
            gc.free()
        for h in self.hal.values():
            h.close()


@pytest.fixture(scope="module")
def bench():
    b = Bench()
    yield b
    b.close()


@pytest.fixture
def finish_on(bench):
    """r0h_ctx_set_device_finish on for the test, on both contexts, and off again behind it"""
    bench.set_finish(True)
    yield
    bench.set_finish(False)


# ---- 1. seals
@pytest.mark.parametrize("name,po2", SIZES)
@pytest.mark.parametrize("suite", SUITES)
def test_the_seal_of_enqueue_and_collect_is_the_blocking_forms(bench, orc, finish_on, suite, name, po2):
    c = bench.case(suite, name, po2)
    h = c["h"]
    proof = h.prove_segment_enqueue(c["gc"], po2, c["cc"], c["data"], c["glob"])
    got = h.prove_segment_collect(proof)
    assert np.array_equal(got, c["seal"])
    root = c["cc"].root()
    if suite == "poseidon2":
        assert orc.circuit(c["blob"]).verify(got, code_root=root) == (0, "ok")
    assert r0.verify_seal(c["blob"], got, code_root=root, hashfn=suite)[:3] == (0, "ok", po2)


# ---- 2. waits
@pytest.mark.parametrize("name,po2", SIZES)
def test_a_whole_proof_waits_twice(bench, finish_on, name, po2):
    """The blocking form under r0h_ctx_set_device_finish waits four times: the DATA tree's top layer read back (commit_tree on the host
    generator), the DATA root read back, the read-back of the tail and the close of the profile.  The enqueue form keeps the last two."""
    c = bench.case("poseidon2", name, po2)
    h = c["h"]
    before = h.blocking_waits()
    assert np.array_equal(h.prove_segment(c["gc"], po2, c["cc"], c["data"], c["glob"]), c["seal"])
    blocking = h.blocking_waits() - before
    before = h.blocking_waits()
    proof = h.prove_segment_enqueue(c["gc"], po2, c["cc"], c["data"], c["glob"])
    assert h.blocking_waits() == before, "the enqueue waited for the stream"
    got = h.prove_segment_collect(proof)
    enqueued = h.blocking_waits() - before
    print("blocking waits: r0h_prove_segment_committed %d, enqueue + collect %d" % (blocking, enqueued))
    assert np.array_equal(got, c["seal"])
    assert blocking == 4
    assert enqueued == 2


# ---- 3. r0h_accum_mixbuf against r0h_accum, bit for bit
@pytest.mark.parametrize("name,po2", SIZES)
def test_accum_mixbuf_is_accum_bit_for_bit(bench, name, po2):
    c = bench.case("poseidon2", name, po2)
    h, gc = c["h"], c["gc"]
    n_mix = gc.n_mix
    assert n_mix >= 8
    drawn = np.random.default_rng(27).integers(0, P, size=n_mix).astype(np.uint32)
    mixes = {"zero": np.zeros(n_mix, np.uint32), "one": np.ones(n_mix, np.uint32), "p - 1": np.full(n_mix, P - 1, np.uint32), "drawn": drawn}
    for label, mix in mixes.items():
        want_buf = h.accum(gc, po2, c["code"], c["data"], mix)
        want = want_buf.to_host()
        want_buf.free()
        for offset in (0, 5):
            words = np.full(n_mix + 8, 0xFFFFFFFF, np.uint32)  # (what surrounds the mix is not a field element: it must not be read)
            words[offset:offset + n_mix] = mix
            mbuf = h.copy_from(words)
            got_buf = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf, offset)
            got = got_buf.to_host()
            got_buf.free(), mbuf.free()
            assert np.array_equal(got, want), (label, offset)
    short = h.alloc(8)
    with pytest.raises(r0.R0HipError, match=r"r0h_accum_mixbuf: buffers too small for 2\^%d rows" % po2):      # (the error names its entry point)
        r0._check(r0.lib().r0h_accum_mixbuf(h.ctx, gc.handle, po2, None, c["data"].handle, c["data"].handle, 0, short.handle))
    short.free()
    mbuf = h.alloc(n_mix + 8)
    with pytest.raises(r0.R0HipError, match=r"r0h_accum_mixbuf: the mix at words \[9, \+%d\) ends beyond a buffer of %d words" % (n_mix, n_mix + 8)):
        h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf, 9)
    mbuf.free()


def test_the_mix_drawn_at_the_begin_is_the_hosts(bench, finish_on):
    """begin-enqueue -> r0h_accum_mixbuf from mix_out -> finish-enqueue -> collect: the two-phase form, and the mix words themselves"""
    c = bench.case("poseidon2", "small", 13)
    h, gc, po2 = c["h"], c["gc"], 13
    h.set_device_finish(False)
    first, mix = h.proof_begin(gc, po2, c["cc"], c["data"], c["glob"])
    h.proof_abort(first)
    h.set_device_finish(True)
    mbuf = h.alloc(gc.n_mix + 3)
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf)
    accum = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf, 0)
    h.proof_finish_enqueue(proof, accum)
    got = h.proof_finish_collect(proof)
    assert np.array_equal(mbuf.to_host()[:gc.n_mix], mix)
    assert np.array_equal(got, c["seal"])
    accum.free(), mbuf.free()


# ---- 4. a circuit with late inputs: the trace circuit over a corner program
class Trace:
    def __init__(self):
        self.blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
        vm = tcr.run(tcr.PROGRAMS["alu"]())
        assert len(vm.segments()) == 1
        data, glob = vm.trace_witness(0, TRACE_PO2)
        self.data = np.asarray(data, dtype=np.uint32)
        self.glob = np.asarray(glob, dtype=np.uint32).copy()
        self.glob[N_EARLY:] = 0


def challenge_of(root):
    """what a session does with all its segments' roots, cut down to one: sixteen canonical words that depend on every word of the root"""
    return np.random.default_rng([int(w) for w in root]).integers(1, P, size=16).astype(np.uint32)


def test_late_inputs_follow_a_root_gathered_on_the_device(bench):
    t = Trace()
    h = bench.hal["poseidon2"]
    gc = h.load_circuit(t.blob, entry.code_object_path("trace"))
    code, synthetic, _ = h.witgen(gc, TRACE_PO2, 0)
    synthetic.free()
    cc, data = h.code_commit(gc, TRACE_PO2, code), h.copy_from(t.data.reshape(-1))
    n_late = r0.TRACE_LATE_GLOBALS
    bufs = [cc, data, code]
    try:
        # the all-blocking sequence, every switch off
        h.set_device_finish(False)
        proof, _ = h.proof_begin(gc, TRACE_PO2, cc, data, t.glob)
        want_root = h.proof_data_root(proof)
        glob = t.glob.copy()
        glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = challenge_of(want_root)
        full = h.logup_totals(gc, TRACE_PO2, code, data, glob)
        mix = h.proof_late(proof, gc, full[N_EARLY:])
        accum = h.accum_public(gc, TRACE_PO2, code, data, full, mix)
        want = h.proof_finish(proof, accum)
        accum.free()
        assert r0.verify_seal(t.blob, want, code_root=cc.root())[:3] == (0, "ok", TRACE_PO2)
        # the same with nothing waiting but the root's read-back (the test's own) and the collect
        h.set_device_finish(True)
        roots, mbuf = h.alloc(24), h.alloc(gc.n_mix)
        bufs += [roots, mbuf]
        before = h.blocking_waits()
        proof = h.proof_begin_enqueue(gc, TRACE_PO2, cc, data, t.glob)
        h.proof_data_root_device(proof, roots, 8)
        assert h.blocking_waits() == before, "the begin or the root's copy waited for the stream"
        root = roots.to_host()[8:16]
        assert np.array_equal(root, want_root)
        assert np.array_equal(h.proof_data_root(proof), want_root)      # (eight words read back: a wait, and the same root)
        glob = t.glob.copy()
        glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = challenge_of(root)
        gbuf = h.copy_from(glob)
        bufs.append(gbuf)
        before = h.blocking_waits()
        h.logup_totals_device(gc, TRACE_PO2, code, data, gbuf)
        late = gbuf.slice(N_EARLY, n_late)
        bufs.append(late)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late: the proof's transcript went to the device before its DATA commitment"):
            h.proof_late(proof, gc, full[N_EARLY:])
        h.proof_late_device(proof, late, mbuf)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the accumulation mix has been drawn already"):
            h.proof_late_device(proof, late, mbuf)
        accum = h.accum_public_device(gc, TRACE_PO2, code, data, gbuf, mbuf)
        bufs.append(accum)
        h.proof_finish_enqueue(proof, accum)
        assert h.blocking_waits() == before, "a step behind the root waited for the stream"
        got = h.proof_finish_collect(proof)
        assert h.blocking_waits() == before + 2
        assert np.array_equal(got, want)
        assert np.array_equal(mbuf.to_host(), mix)
    finally:
        h.set_device_finish(False)
        for b in reversed(bufs):
            b.free()
        gc.free()


# ---- 5. the DATA tree kept as its top
def test_a_kept_top_gives_the_tree_forms_seal(bench, finish_on):
    c = bench.case("poseidon2", "small", 13)
    h, gc, po2 = c["h"], c["gc"], 13
    first = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
    top = h.proof_data_top(first, po2, 6)
    h.proof_abort(first)
    mbuf = h.alloc(gc.n_mix)
    before = h.blocking_waits()
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf, top=(top, 6))
    accum = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf)
    h.proof_finish_enqueue(proof, accum)
    assert h.blocking_waits() == before
    assert np.array_equal(h.proof_finish_collect(proof), c["seal"])
    accum.free()
    # a top of other columns: the enqueues succeed, the existing error is the collect's, and the context goes on
    other_code, other_data, other_glob = h.witgen(gc, po2, 2)
    first = h.proof_begin_enqueue(gc, po2, c["cc"], other_data, other_glob)
    other_top = h.proof_data_top(first, po2, 6)
    h.proof_abort(first)
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf, top=(other_top, 6))
    accum = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf)
    h.proof_finish_enqueue(proof, accum)
    with pytest.raises(r0.R0HipError, match=r"r0h_proof_finish: tree top does not match the matrix under query \d+ \(row \d+\)"):
        h.proof_finish_collect(proof)
    accum.free()
    proof = h.prove_segment_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
    assert np.array_equal(h.prove_segment_collect(proof), c["seal"])
    for b in (top, other_top, mbuf, other_code, other_data):
        b.free()


# ---- 6. two proofs in flight on two contexts, from one thread
def test_two_contexts_in_flight_from_one_thread(bench, finish_on):
    a = bench.case("poseidon2", "small", 13)
    h2 = r0.Hal(0)
    h2.set_device_finish(True)
    gc2 = h2.load_circuit(a["blob"], entry.code_object_path("small"))
    code2, data2, glob2 = h2.witgen(gc2, 13, 5)
    cc2 = h2.code_commit(gc2, 13)
    try:
        h2.set_device_finish(False)
        want2 = h2.prove_segment(gc2, 13, cc2, data2, glob2)
        h2.set_device_finish(True)
        assert not np.array_equal(want2, a["seal"])
        pa = a["h"].prove_segment_enqueue(a["gc"], 13, a["cc"], a["data"], a["glob"])
        pb = h2.prove_segment_enqueue(gc2, 13, cc2, data2, glob2)
        got2 = h2.prove_segment_collect(pb)
        got = a["h"].prove_segment_collect(pa)
        assert np.array_equal(got2, want2) and np.array_equal(got, a["seal"])
    finally:
        for b in (cc2, code2, data2, gc2):
            b.free()
        h2.close()


# ---- 7. refusals, each by its message; the proof and the context are usable afterwards
def test_refusals(bench):
    c = bench.case("poseidon2", "tiny", 9)
    h, gc, po2 = c["h"], c["gc"], 9
    try:
        # r0h_ctx_set_device_finish off
        h.set_device_finish(False)
        with pytest.raises(r0.R0HipError, match="r0h_proof_begin_committed_enqueue: the context has r0h_ctx_set_device_finish off"):
            h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
        with pytest.raises(r0.R0HipError, match="r0h_prove_segment_committed_enqueue: the context has r0h_ctx_set_device_finish off"):
            h.prove_segment_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
        h.set_device_finish(True)
        # the columns form: in the harness, and in the library
        with pytest.raises(r0.R0HipError, match="proof_begin_enqueue: the columns form .* r0h_code_commit_new"):
            h.proof_begin_enqueue(gc, po2, c["code"], c["data"], c["glob"])
        g, pg = r0._u32arr(c["glob"])
        out = r0._vp()
        with pytest.raises(r0.R0HipError, match="r0h_prove_segment_committed_enqueue: no CODE commitment: the columns forms .* r0h_code_commit_new"):
            r0._check(r0.lib().r0h_prove_segment_committed_enqueue(h.ctx, gc.handle, po2, None, c["data"].handle, pg, r0.ctypes.byref(out)))
        small = h.alloc(gc.n_mix - 1)
        with pytest.raises(r0.R0HipError, match="r0h_proof_begin_committed_enqueue: mix_out holds %d words, the circuit draws %d" % (gc.n_mix - 1, gc.n_mix)):
            h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=small)
        small.free()
        # collect without enqueue, a second late step, a host late step: refused, and the proof goes on to its seal
        mbuf = h.alloc(gc.n_mix)
        proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf)
        with pytest.raises(r0.R0HipError, match="r0h_proof_finish_collect: the proof has not been enqueued"):
            h.prove_segment_collect(proof)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the accumulation mix has been drawn already"):
            h.proof_late_device(proof, None, mbuf)
        # the suite changed between the begin and the finish
        h.set_hashfn("sha-256")
        accum = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf)
        with pytest.raises(r0.R0HipError, match="r0h_proof_finish: the proof was begun under the poseidon2 hash suite, its context is now on sha-256"):
            h.proof_finish_enqueue(proof, accum)      # (an error in an enqueue consumes the proof)
        h.set_hashfn("poseidon2")
        proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf)
        h.proof_finish_enqueue(proof, accum)
        assert np.array_equal(h.proof_finish_collect(proof), c["seal"])
        accum.free(), mbuf.free()
    finally:
        h.set_hashfn("poseidon2")
        h.set_device_finish(False)


def test_the_suite_changed_between_begin_and_late_is_refused(bench):
    t = Trace()
    h = bench.hal["poseidon2"]
    gc = h.load_circuit(t.blob, entry.code_object_path("trace"))
    code, synthetic, _ = h.witgen(gc, TRACE_PO2, 0)
    synthetic.free()
    cc, data = h.code_commit(gc, TRACE_PO2, code), h.copy_from(t.data.reshape(-1))
    glob = t.glob.copy()
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = challenge_of(np.arange(8))
    gbuf, mbuf = h.copy_from(h.logup_totals(gc, TRACE_PO2, code, data, glob)), h.alloc(gc.n_mix)
    late = gbuf.slice(N_EARLY, r0.TRACE_LATE_GLOBALS)
    h.set_device_finish(True)
    try:
        proof = h.proof_begin_enqueue(gc, TRACE_PO2, cc, data, glob)
        h.set_hashfn("sha-256")
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: the proof was begun under the poseidon2 hash suite, its context is now on sha-256"):
            h.proof_late_device(proof, late, mbuf)
        h.set_hashfn("poseidon2")
        h.set_device_finish(False)
        with pytest.raises(r0.R0HipError, match="r0h_proof_late_device: .*r0h_ctx_set_device_finish off"):
            h.proof_late_device(proof, late, mbuf)
        h.set_device_finish(True)
        h.proof_late_device(proof, late, mbuf)        # the refusals left the proof as it was
        accum = h.accum_public_device(gc, TRACE_PO2, code, data, gbuf, mbuf)
        seal = h.proof_finish(proof, accum)
        accum.free()
        assert r0.verify_seal(t.blob, seal, code_root=cc.root())[:3] == (0, "ok", TRACE_PO2)
    finally:
        h.set_hashfn("poseidon2")
        h.set_device_finish(False)
        for b in (late, gbuf, mbuf, cc, data, code, gc):
            b.free()


# ---- 8. abort with the stream busy, then a full proof on the same context
def test_abort_after_a_begin_enqueue_then_a_full_proof(bench, finish_on):
    c = bench.case("poseidon2", "small", 13)
    h, gc, po2 = c["h"], c["gc"], 13
    before = h.blocking_waits()
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
    assert r0.lib().r0h_proof_resident_bytes(proof) > 0
    assert h.blocking_waits() == before
    h.proof_abort(proof)
    assert h.blocking_waits() == before + 1       # the abort waited for what the begin had enqueued
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
    freed = r0.ctypes.c_size_t(0)
    r0._check(r0.lib().r0h_proof_shrink(proof, r0.ctypes.byref(freed)))      # works as on any proof (and waits, as ever)
    assert freed.value == (gc.group_size[r0.GROUP_DATA] << (po2 + 2)) * 4
    h.proof_abort(proof)
    # a proof submitted whole keeps its ACCUM witness until the collect, and r0h_proof_resident_bytes counts it: the same proof enqueued
    # in two steps holds the same groups and leaves the witness with its caller
    mbuf = h.alloc(gc.n_mix)
    proof = h.proof_begin_enqueue(gc, po2, c["cc"], c["data"], c["glob"], mix_buf=mbuf)
    accum = h.accum_mixbuf(gc, po2, c["code"], c["data"], mbuf)
    h.proof_finish_enqueue(proof, accum)
    in_steps = r0.lib().r0h_proof_resident_bytes(proof)
    assert np.array_equal(h.proof_finish_collect(proof), c["seal"])
    accum.free(), mbuf.free()
    proof = h.prove_segment_enqueue(gc, po2, c["cc"], c["data"], c["glob"])
    assert r0.lib().r0h_proof_resident_bytes(proof) == in_steps + (gc.group_size[r0.GROUP_ACCUM] << po2) * 4
    assert np.array_equal(h.prove_segment_collect(proof), c["seal"])


# ---- a whole proof of a circuit with late inputs and a log-derivative accumulation: the late inputs are host words of `global`
def test_a_whole_proof_with_late_inputs_from_host_words(bench, finish_on):
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from bench_session import elf_of
    h = bench.hal["poseidon2"]
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = h.load_circuit(iblob, entry.code_object_path("image"))
    elf = elf_of(tcr.PROGRAMS["alu"](), tcr.BASE)
    po2 = r0.image_po2(elf)
    idata, _ = r0.image_witness(elf, po2)
    gamma = np.random.default_rng(31).integers(1, P, size=16).astype(np.uint32)
    h.set_device_finish(False)
    want = h.prove_image(ic, elf, gamma)
    h.set_device_finish(True)
    full = want[:r0.IMAGE_GLOBALS].copy()          # digest, challenge, and the total r0h_prove_image added up
    code, synthetic, _ = h.witgen(ic, po2, 0)
    synthetic.free()
    cc, data = h.code_commit(ic, po2, code), h.copy_from(idata.reshape(-1))
    try:
        before = h.blocking_waits()
        proof = h.prove_segment_enqueue(ic, po2, cc, data, full)
        assert h.blocking_waits() == before
        assert np.array_equal(h.prove_segment_collect(proof), want)
        bad = full.copy()
        bad[r0.IMAGE_SUM + 1] = P
        with pytest.raises(r0.R0HipError, match="r0h_prove_segment_committed_enqueue: late public input %d is not canonical" % (r0.IMAGE_SUM + 1 - r0.IMAGE_GAMMA)):
            h.prove_segment_enqueue(ic, po2, cc, data, bad)
    finally:
        for b in (cc, data, code, ic):
            b.free()
