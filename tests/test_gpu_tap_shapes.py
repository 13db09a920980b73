"""Whole proofs, on the device, of the circuits of tests/tap_circuits.py -- a 64-tap register over every back the format admits (65
DEEP points: a second workgroup of deep_points_kernel), registers of 3, 4 and 5 taps that are no prefix of 0, 1, 2, a combo that ACCUM
creates and DATA joins, a lone {0, 63} combo created last -- held against the oracle's proof of the same witness word for word, in
every form of the transcript, under both hash suites, accepted by all three verifiers; and the same with one cell spoiled.  Every proof
goes through proof_begin / proof_finish with the family's own accumulation: the circuits have no ACCUM section."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0

import check_ref
import evalcheck_circuits as hand
import tap_circuits as tc
from field_words import family
from test_tap_shapes import CASES, MISMATCH, made, spoiled

pytestmark = pytest.mark.gpu
P = tc.P
SUITES = ["poseidon2", "sha-256"]
SWITCHES = ["set_device_transcript", "set_device_finish"]


class Rig:
    """a context per suite (Poseidon2's is the session's), each family compiled once on each, the witnesses of test_tap_shapes.made
    uploaded once, and the host-transcript seal of every (suite, family, size) made once with both switches off"""

    def __init__(self, hal):
        self.hal = {"poseidon2": hal, "sha-256": r0.Hal(0)}
        self.hal["sha-256"].set_hashfn("sha-256")
        self.gc, self.bufs, self.seals = {}, {}, {}

    def circuit(self, suite, name):
        if (suite, name) not in self.gc:
            blob = hand.FAMILIES["taps"]() if name == "taps" else tc.FAMILIES[name].blob()
            self.gc[suite, name] = self.hal[suite].load_circuit(blob)  # compiled in-process
        return self.gc[suite, name]

    def witness(self, orc, suite, name, po2):
        if (suite, name, po2) not in self.bufs:
            _, _, code, data, _, _ = made(orc, name, po2)
            self.bufs[suite, name, po2] = (self.hal[suite].copy_from(code), self.hal[suite].copy_from(data))
        return self.bufs[suite, name, po2]

    def prove(self, suite, name, po2, code, data, accum_of, glob=tc.GLOB):
        """(seal, mix) of one proof: begin, the caller's accumulation of the mix, finish"""
        h = self.hal[suite]
        proof, mix = h.proof_begin(self.circuit(suite, name), po2, code, data, glob)
        accum = h.copy_from(accum_of(mix))
        try:
            return h.proof_finish(proof, accum), mix
        finally:
            accum.free()

    def host_seal(self, orc, suite, name, po2):
        if (suite, name, po2) not in self.seals:
            fam, (code, data) = tc.FAMILIES[name], self.witness(orc, suite, name, po2)
            host_data = made(orc, name, po2)[3]
            seal, mix = self.prove(suite, name, po2, code, data, lambda m: fam.accum(host_data, m))
            seal.setflags(write=False)
            self.seals[suite, name, po2] = (seal, mix)
        return self.seals[suite, name, po2]

    def close(self):
        for g in self.gc.values():
            g.free()
        for code, data in self.bufs.values():
            code.free(), data.free()
        self.hal["sha-256"].close()


@pytest.fixture(scope="module")
def rig(hal):
    r = Rig(hal)
    yield r
    r.close()


# ---- a. the host transcript under Poseidon2: the oracle's mix, the oracle's seal
@pytest.mark.parametrize("name,po2", CASES)
def test_the_seal_is_the_oracles_word_for_word(rig, orc, name, po2):
    blob, oc, _, _, want, want_mix = made(orc, name, po2)
    seal, mix = rig.host_seal(orc, "poseidon2", name, po2)
    assert np.array_equal(mix, want_mix)  # what proof_begin returns is what the oracle's callback was given
    differ = np.nonzero(seal[:min(seal.size, want.size)] != want[:min(seal.size, want.size)])[0]
    assert seal.size == want.size and differ.size == 0, "sizes %d / %d, first differing word %s" % (seal.size, want.size, differ[:1])


@pytest.mark.parametrize("po2", [9, 13])
def test_the_taps_family_on_random_words_is_the_oracles_seal_too(rig, orc, po2):
    """evalcheck_circuits.taps, backs {0, 1, 2, 63} on column 0 of every group: random words satisfy nothing, the openings are honest all
    the same, and both provers return a seal -- the same one, which both verifiers refuse at the constraint identity"""
    h = rig.hal["poseidon2"]
    blob = hand.FAMILIES["taps"]()
    oc = orc.circuit(blob)
    rng = np.random.default_rng([22, po2])
    code, data, accum = (rng.integers(0, P, size=2 << po2, dtype=np.uint32) for _ in range(3))
    glob = rng.integers(0, P, size=hand.N_GLOBAL, dtype=np.uint32)
    want = oc.prove(po2, code, data, glob, accum=lambda m: accum)
    cbuf, dbuf = h.copy_from(code), h.copy_from(data)
    try:
        seal, mix = rig.prove("poseidon2", "taps", po2, cbuf, dbuf, lambda m: accum, glob=glob)
        assert np.array_equal(mix, oc.last_mix) and np.array_equal(seal, want)
        for switch in SWITCHES:
            getattr(h, switch)(True)
            try:
                assert np.array_equal(rig.prove("poseidon2", "taps", po2, cbuf, dbuf, lambda m: accum, glob=glob)[0], want), switch
            finally:
                getattr(h, switch)(False)
    finally:
        cbuf.free(), dbuf.free()
    assert oc.verify(seal) == MISMATCH and r0.verify_seal(blob, seal)[:2] == MISMATCH


# ---- b. the forms of the transcript, both suites
@pytest.mark.parametrize("name,po2", CASES)
@pytest.mark.parametrize("suite", SUITES)
def test_the_device_transcripts_give_the_same_words(rig, orc, suite, name, po2):
    h, fam = rig.hal[suite], tc.FAMILIES[name]
    blob, _, _, host_data, oracle_seal, _ = made(orc, name, po2)
    want, want_mix = rig.host_seal(orc, suite, name, po2)
    if suite == "poseidon2":
        assert np.array_equal(want, oracle_seal)
    else:  # no oracle under SHA-256: the host transcript's seal, which the verifier accepts, and which is another seal than Poseidon2's
        assert r0.verify_seal(blob, want, hashfn=suite) == (0, "ok", po2)
        assert want.size != oracle_seal.size or not np.array_equal(want, oracle_seal)
    code, data = rig.witness(orc, suite, name, po2)
    for switch in SWITCHES:
        stats = None
        getattr(h, switch)(True)
        try:
            if (name, switch) == ("wide", "set_device_finish"):
                h.kernel_timing(True)
            got, mix = rig.prove(suite, name, po2, code, data, lambda m: fam.accum(host_data, m))
            if (name, switch) == ("wide", "set_device_finish"):
                stats = h.kernel_stats()
        finally:
            getattr(h, switch)(False)
            h.kernel_timing(False)
        assert np.array_equal(mix, want_mix) and np.array_equal(got, want), switch
        if stats is not None:  # 64 backs and z^4: 65 points, the table's second workgroup, in one launch
            ran = {k: v["launches"] for k, v in stats.items() if v["launches"]}
            assert ran.get("deep_points_kernel") == 1, ran
            assert ran.get("interpolate_regs_kernel", 0) >= 1 and ran.get("divide_jobs_kernel", 0) >= 1, ran


# ---- c. the three verifiers
@pytest.mark.parametrize("name,po2", CASES)
@pytest.mark.parametrize("suite", SUITES)
def test_every_verifier_accepts_the_honest_seal(rig, orc, suite, name, po2):
    blob, oc = made(orc, name, po2)[:2]
    seal, _ = rig.host_seal(orc, suite, name, po2)
    assert r0.verify_seal(blob, seal, hashfn=suite) == (0, "ok", po2)
    assert rig.hal[suite].verify_seals(blob, [seal, seal])[0][:3] == (0, "ok", po2)  # the device climbs the Merkle paths
    if suite == "poseidon2":
        assert oc.verify(seal) == (0, "ok")
    else:
        assert r0.verify_seal(blob, seal)[0] != 0  # not a Poseidon2 seal
    bad = seal.copy()
    bad[bad.size - 3] = (int(bad[bad.size - 3]) + 1) % P
    assert rig.hal[suite].verify_seals(blob, [seal, bad])[1][:2] == r0.verify_seal(blob, bad, hashfn=suite)[:2] != (0, "ok")


# ---- d. one cell spoiled
@pytest.mark.parametrize("which", [0, 1], ids=["data-cell", "accum-cell"])
@pytest.mark.parametrize("name,po2", CASES)
def test_a_spoiled_witness_is_named_proved_and_refused(rig, orc, name, po2, which):
    h, fam, n = rig.hal["poseidon2"], tc.FAMILIES[name], 1 << po2
    gc = rig.circuit("poseidon2", name)
    blob, oc, code, data, _, _ = made(orc, name, po2)
    spoiler = fam.spoilers(n)[which]
    table = spoiler[4]
    bad, accum_of = spoiled(fam, n, data, spoiler)
    want = oc.prove(po2, code, bad, fam.glob, accum=accum_of)
    cbuf = rig.witness(orc, "poseidon2", name, po2)[0]
    dbuf = h.copy_from(bad)
    abuf = h.copy_from(accum_of(oc.last_mix))
    try:
        # the device's checker gives the reference's table (which test_tap_shapes holds to the stated one)
        assert check_ref.check(blob, po2, code, bad, fam.glob, accum_of(oc.last_mix), oc.last_mix) == table
        got = {t: (rows, first) for t, rows, first in h.check_witness(gc, po2, cbuf, dbuf, fam.glob, abuf, oc.last_mix)}
        assert got == table
        late = check_ref.Program(blob).late
        early = {t: (rows, first) for t, rows, first in h.check_witness(gc, po2, cbuf, dbuf, fam.glob)}
        assert early == {t: v for t, v in table.items() if not late[t]}
        # the proof completes all the same, and is the oracle's proof of the same spoiled inputs
        seal, mix = rig.prove("poseidon2", name, po2, cbuf, dbuf, accum_of)
        assert np.array_equal(mix, oc.last_mix) and np.array_equal(seal, want)
        assert oc.verify(seal) == MISMATCH and r0.verify_seal(blob, seal)[:2] == MISMATCH
        assert h.verify_seals(blob, [seal])[0][:2] == MISMATCH
        # with the switch on the sequencer refuses, naming the first violated term and its first row as check_ref numbers them
        first = min(table)
        text = "term %d does not vanish on %d of 2^%d rows, first at row %d" % (first, table[first][0], po2, table[first][1])
        h.set_check_witness(True)
        try:
            for finish in (False, True):
                h.set_device_finish(finish)
                with pytest.raises(r0.R0HipError) as e:
                    rig.prove("poseidon2", name, po2, cbuf, dbuf, accum_of)
                assert "the witness violates %d of the circuit's %d constraint terms" % (len(table), len(late)) in str(e.value)
                assert text in str(e.value)
        finally:
            h.set_check_witness(False)
            h.set_device_finish(False)
    finally:
        dbuf.free(), abuf.free()
    # nothing of that is left behind: the honest proof is still the oracle's
    honest = rig.witness(orc, "poseidon2", name, po2)
    assert np.array_equal(rig.prove("poseidon2", name, po2, honest[0], honest[1], lambda m: fam.accum(data, m))[0], made(orc, name, po2)[4])


# ---- e. the openings of the 64-tap column: 32 two-point passes over one column in one call
@pytest.mark.parametrize("kind", ["random", "top"])
@pytest.mark.parametrize("po2", [9, 13])
def test_a_column_opens_at_all_64_backs_in_one_call(hal, orc, po2, kind):
    n = 1 << po2
    rng = np.random.default_rng([64, po2])
    if kind == "random":  # f0 of `wide` as the prover holds it: interpolated, shifted for zero knowledge, in natural order
        f0 = made(orc, "wide", po2)[3][:n]
        coeffs = orc.batch_bit_reverse(orc.zk_shift(orc.batch_interpolate_ntt(f0, 1, po2), 1, po2), 1, po2)
    else:
        coeffs = family(rng, n, kind)
    z = rng.integers(0, P, 4).astype(np.uint32)
    back_one = orc.L.orc_rou_rev(po2)
    xs = np.array([[orc.mul(int(w), orc.L.orc_fp_pow(back_one, b)) for w in z] for b in range(64)], dtype=np.uint32).reshape(-1)
    assert len({tuple(x) for x in xs.reshape(-1, 4)}) == 64
    which = np.zeros(64, dtype=np.uint32)
    want = orc.batch_evaluate_any(coeffs, po2, which, xs)
    cbuf = hal.copy_from(coeffs)
    out = hal.copy_from(np.full(4 * 64 + 4, 0xFFFFFFFF, np.uint32))
    try:
        hal.batch_evaluate_any(cbuf, po2, which, xs, out)
        got = out.to_host()
    finally:
        cbuf.free(), out.free()
    assert np.all(got[-4:] == 0xFFFFFFFF), "the element past the last result was written"
    assert np.array_equal(got[:-4], want)
    # the back-0 opening is the plain evaluation at z: Horner over the extension field, four coefficients of it checked by hand
    if po2 == 9:
        tot = np.zeros(4, np.uint32)
        for k in range(n - 1, -1, -1):
            tot = orc.fp4_mul(tot, z)
            tot[0] = (int(tot[0]) + int(coeffs[k])) % P
        assert np.array_equal(want[:4], tot)
