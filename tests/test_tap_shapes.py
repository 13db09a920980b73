"""Whole proofs of circuits whose tap sets no shipped circuit has (tests/tap_circuits.py: a 64-tap register, registers over backs that
are no prefix of 0, 1, 2, a lone {0, 63} combo created last), without a GPU: the numpy witnesses are clean under check_ref and their
one-cell spoilers give the stated tables; the oracle proves them with the accumulation handed in (orc_prove_segment_with); the
oracle's verifier and the product's (r0h_verify_seal, csrc/verify.cpp and the combo table of csrc/blob.cpp) accept the honest seals,
reject the spoiled ones at the constraint identity, and agree in verdict and reason on every mutation tried -- every word of coeff_u
(the whole interpolant of every register, the 64-tap one included, and CHECK's sixteen openings) and a few hundred seeded positions
elsewhere."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0

import check_ref
import tap_circuits as tc
import verify_mutations

P = tc.P
SIZES = (9, 13)  # the smallest trace the prover accepts, and the smallest with two FRI rounds
CASES = [(name, po2) for name in tc.FAMILIES for po2 in SIZES]
MISMATCH = (4, "constraint check mismatch at z")
_made = {}


def made(orc, name, po2):
    """(blob, oracle circuit, code, data, honest seal, the mix the oracle drew), made once per (family, size) and left unchanged"""
    if (name, po2) not in _made:
        fam = tc.FAMILIES[name]
        blob = fam.blob()
        oc = orc.circuit(blob)
        code, data = fam.witness(1 << po2, np.random.default_rng([77, po2]))
        seal = oc.prove(po2, code, data, fam.glob, accum=lambda mix: fam.accum(data, mix))
        mix = oc.last_mix.copy()
        for a in (blob, code, data, seal, mix):
            a.setflags(write=False)
        _made[name, po2] = (blob, oc, code, data, seal, mix)
    return _made[name, po2]


def spoiled(fam, n, data, spoiler):
    """(data, accum callback) with the spoiler's cell one more than it was"""
    _, group, col, row, _ = spoiler
    if group == tc.G_DATA:
        bad = tc.spoil(data, n, col, row)
        return bad, lambda mix: fam.accum(bad, mix)
    return data, lambda mix: tc.spoil(fam.accum(data, mix), n, col, row)


@pytest.mark.parametrize("name", list(tc.FAMILIES))
def test_the_blobs_hold_the_registers_and_combos_they_are_built_for(orc, name):
    blob = tc.FAMILIES[name].blob()
    regs = tc.registers(blob)
    assert tc.combos(blob) == tc.COMBOS[name]
    oc = orc.circuit(blob)
    assert oc.n_combos == len(tc.COMBOS[name]) and oc.n_taps == sum(len(b) for _, _, b in regs)
    assert (oc.n_global, oc.n_mix) == (2, 2)
    sizes = sorted(len(b) for _, _, b in regs)
    if name == "wide":
        assert sizes[-1] == 64 and [b for _, _, b in regs if len(b) == 64] == [list(range(64))]
    if name == "odd":
        shapes = {g: [b for gg, _, b in regs if gg == g] for g in range(3)}
        assert [0, 31, 32] in shapes[tc.G_ACCUM] and [0, 31, 32] in shapes[tc.G_DATA]  # ACCUM's combo, joined by a later group
        assert [0, 3, 31, 32] in shapes[tc.G_CODE] and [0, 3, 31, 32] not in shapes[tc.G_ACCUM] + shapes[tc.G_DATA]
        assert len({len(c) for c in tc.COMBOS[name]}) == len(tc.COMBOS[name])  # every combo its own number of divisions
    if name == "far":
        assert regs[-1] == (tc.G_DATA, 2, [0, 63]) and all(b == [0] for _, _, b in regs[:-1])
    late = check_ref.Program(blob).late
    assert any(late) and not all(late)


@pytest.mark.parametrize("name,po2", CASES)
def test_the_witness_is_clean_and_each_spoiler_gives_its_table(orc, name, po2):
    fam, n = tc.FAMILIES[name], 1 << po2
    blob, _, code, data, _, mix = made(orc, name, po2)
    assert check_ref.check(blob, po2, code, data, fam.glob, fam.accum(data, mix), mix) == {}
    assert check_ref.check(blob, po2, code, data, fam.glob) == {}
    wrong = fam.glob.copy()
    wrong[0] = (int(wrong[0]) + tc.R) % P  # a term of every family reads the public inputs
    assert check_ref.check(blob, po2, code, data, wrong)
    other = mix.copy()
    for k in range(2):  # and a late term each mix word: an accumulation under another mix is not this one's
        other[:] = mix
        other[k] = (int(other[k]) + tc.R) % P
        assert check_ref.check(blob, po2, code, data, fam.glob, fam.accum(data, mix), other)
    for spoiler in fam.spoilers(n):
        bad, accum = spoiled(fam, n, data, spoiler)
        assert check_ref.check(blob, po2, code, bad, fam.glob, accum(mix), mix) == spoiler[4], spoiler[0]


@pytest.mark.parametrize("name,po2", CASES)
def test_the_oracle_proves_and_both_verifiers_accept_or_name_the_constraint_identity(orc, name, po2):
    fam, n = tc.FAMILIES[name], 1 << po2
    blob, oc, code, data, seal, mix = made(orc, name, po2)
    again = oc.prove(po2, code, data, fam.glob, accum=lambda m: fam.accum(data, m))
    assert np.array_equal(again, seal) and np.array_equal(oc.last_mix, mix)  # deterministic
    assert oc.verify(seal) == (0, "ok")
    assert r0.verify_seal(blob, seal) == (0, "ok", po2)
    assert verify_mutations.regions(blob, seal)["po2"] == po2  # the seal has the length its layout gives
    for spoiler in fam.spoilers(n):
        bad, accum = spoiled(fam, n, data, spoiler)
        forged = oc.prove(po2, code, bad, fam.glob, accum=accum)  # the openings are honest: a seal comes out ...
        assert oc.verify(forged) == MISMATCH, spoiler[0]  # ... that states a witness the constraints refuse
        assert r0.verify_seal(blob, forged)[:2] == MISMATCH, spoiler[0]
    with pytest.raises(AssertionError, match="accum gave"):
        oc.prove(po2, code, data, fam.glob, accum=lambda m: np.zeros(3, np.uint32))


@pytest.mark.parametrize("name,po2", CASES)
def test_the_products_verifier_equals_the_oracles_on_single_word_mutations(orc, name, po2):
    blob, oc, _, _, seal, _ = made(orc, name, po2)
    reg = verify_mutations.regions(blob, seal)
    lo, hi = reg["coeff_u"]
    assert hi - lo == 4 * (oc.n_taps + 16)
    rng = np.random.default_rng([1000, po2, len(name)])
    seen = {}
    # every word of coeff_u, the words before it (public inputs, po2, the four tops), then seeded positions over the rest
    positions = list(range(lo, hi)) + list(range(0, 40)) + [int(p) for p in rng.integers(hi, seal.size, 200)]
    for k, pos in enumerate(positions):
        bad = seal.copy()
        kind = k % 3 if lo <= pos < hi else int(rng.integers(0, 3))  # the three kinds of test_verify.py
        if kind == 0:
            bad[pos] = (int(bad[pos]) + 1) % P
        elif kind == 1:
            bad[pos] = int(rng.integers(0, P))
        else:
            bad[pos] = int(rng.integers(P, 1 << 32))  # a non-canonical word
        if bad[pos] == seal[pos]:
            continue
        want = oc.verify(bad)
        got = r0.verify_seal(blob, bad)
        assert got[:2] == want, "word %d: product says %r, oracle says %r" % (pos, got, want)
        assert got[0] != 0
        seen[got[0]] = seen.get(got[0], 0) + 1
        if lo <= pos < hi:
            assert got[0] == (9 if kind == 2 else 4), pos  # an opening that is not the committed column's: the identity at z fails
    for cut in (0, 1, 7, lo, lo + 5, hi - 1, hi, seal.size // 3, seal.size - 1):
        got = r0.verify_seal(blob, seal[:cut])
        assert got[:2] == oc.verify(seal[:cut]) == (1, "seal truncated"), cut
    for extra in (1, 3):
        longer = np.concatenate([seal, np.zeros(extra, np.uint32)])
        assert r0.verify_seal(blob, longer)[:2] == oc.verify(longer) == (8, "trailing words in seal")
    assert {3, 4, 5}.issubset(seen), seen  # group paths, the identity at z, FRI paths


def test_a_seal_of_one_family_is_no_seal_of_another(orc):
    seal = made(orc, "odd", 9)[4]
    other = made(orc, "wide", 9)[0]
    got = r0.verify_seal(other, seal)
    assert got[0] != 0 and got[:2] == made(orc, "wide", 9)[1].verify(seal)


def test_interpolation_through_64_and_65_points_is_the_polynomial(orc):
    """orc_poly_interpolate at the format's bound and one past it, against Horner at every point (it kept 16 slots before)"""
    from orc_binding import _ptr
    rng = np.random.default_rng(64)
    for n in (1, 16, 17, 64, 65):
        xs, ys = rng.integers(0, P, 4 * n).astype(np.uint32), rng.integers(0, P, 4 * n).astype(np.uint32)
        out = np.zeros(4 * n, np.uint32)
        orc.L.orc_poly_interpolate(_ptr(out), _ptr(xs), _ptr(ys), n)
        coeffs = out.reshape(n, 4)
        for i in range(n):
            x, tot = xs[4 * i:4 * i + 4], np.zeros(4, np.uint32)
            for k in range(n - 1, -1, -1):
                tot = orc.fp4_mul(tot, x)
                tot = ((tot.astype(np.uint64) + coeffs[k]) % np.uint64(P)).astype(np.uint32)
            assert np.array_equal(tot, ys[4 * i:4 * i + 4]), (n, i)
