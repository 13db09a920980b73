"""The cheating prover's seals (tests/cheats.py, tests/test_cheating_prover.py) through the collecting verifier with the device
hashing the openings (r0h_verify_seals_on: verify<true> of csrc/verify.cpp, merkle_climb_kernel, settle).  Every Merkle path of these
seals is valid -- the trees are built over the lies -- so every opening reaches its node and each verdict is one that settle's second
rule hands on, "the verdict of the first query whose walk failed": the walk's own algebra, with nothing of the immediate verifier's
hashing in between.  Verdict, reason and po2 must be r0h_verify_seal's for every seal, the honest ones in among the cheats.

All the proving is the oracle's, on the CPU; the device sees one upload and one launch per batch."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0

import cheats

pytestmark = pytest.mark.gpu


def _one_batch(hal, orc, name, sweeps, seed):
    """the sweeps' seals and their honest ones, shuffled, as ONE batch -> [(label, host verdict, device verdict)], launches"""
    cases = []
    for po2, which in sweeps:
        cases += cheats.every_cheating_seal(orc, name, po2, which)
    cases += [("honest, po2 %d" % po2, None, cheats.subject(orc, name, po2).honest) for po2 in sorted({p for p, _ in sweeps})]
    cases = [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]
    blob = cheats.subject(orc, name, sweeps[0][0]).blob
    hal.kernel_timing(True)
    before = hal.kernel_stats().get("merkle_climb_kernel", {"launches": 0})["launches"]
    got = hal.verify_seals(blob, [seal for _, _, seal in cases])
    launches = hal.kernel_stats()["merkle_climb_kernel"]["launches"] - before
    hal.kernel_timing(False)
    assert launches == 1
    return blob, cases, got


def _held_to_the_host(blob, cases, got):
    seen = {}
    for (label, cheat, seal), g in zip(cases, got):
        want = cheats.product_verdict(blob, seal)
        assert g[:3] == want, "%s: device-hashed %r, host %r" % (label, g[:3], want)
        if cheat is None:
            assert g[0] == 0, label
        else:
            assert g[0] in cheats.ALLOWED[cheat[0]] and g[1] == cheats.REASON[g[0]], (label, g[:3])
        seen.setdefault(cheat and cheat[0], set()).add(g[0])
    return seen


def test_every_cheat_of_tiny_with_the_two_round_sample_is_one_batch(hal, orc):
    """tiny: the five sweeps at po2 9 (484 seals), the sample at po2 13 (36) and the two honest seals, shuffled, in ONE batch of mixed
    po2: one launch, every verdict the host's and its kind's.  On the build machine's CPU the proofs take 7.2 s (po2 9) and 8.2 s (the
    sample) and the host's verdicts 0.7 s, where no earlier test of the run has made them; the batch is one upload of 37 MB."""
    blob, cases, got = _one_batch(hal, orc, "tiny", [(9, cheats.SWEEPS), (13, cheats.SAMPLE)], 5)
    assert len(cases) == 484 + 36 + 2
    seen = _held_to_the_host(blob, cases, got)
    assert seen == {None: {0}, "committed": {6}, "flowing": {4}, "coeff_u": {4}, "fri": {6, 7}, "final": {7}}
    assert sorted(g[2] for g in got if g[0] == 0) == [9, 13]


def test_every_cheat_of_small_is_a_second_batch(hal, orc):
    """small at po2 9: 864 cheats and the honest seal.  On the build machine's CPU the proofs take 16.9 s and the host's verdicts
    1.2 s, where no earlier test of the run has made them; one upload of 68 MB, one launch."""
    blob, cases, got = _one_batch(hal, orc, "small", [(9, cheats.SWEEPS)], 6)
    assert len(cases) == 864 + 1
    seen = _held_to_the_host(blob, cases, got)
    assert seen == {None: {0}, "committed": {6}, "flowing": {4}, "coeff_u": {4}, "fri": {6, 7}, "final": {7}}


TRACE_HANDFUL = 8


@pytest.mark.parametrize("k", range(TRACE_HANDFUL))
def test_the_trace_circuit_at_its_smallest_size(hal, orc, k):
    """The trace circuit at TRACE_MIN_PO2 (2^16 rows: late public inputs and the 40-column ACCUM enter only here), an executor's run
    proved by the oracle.  An oracle proof of it takes 4.6 s to 5.6 s on the build machine (8 threads), so the handful is ONE column
    per group, the last (not the first and the last), and four coeff_u words -- of an ACCUM register a term reads together with a
    late public input, its constant coefficient (a running sum read through a(0) - a(1): the identity does not see the shift, the DEEP
    comparison does, 6) and its linear one (4), of a register no term reads (6) and CHECK's last (4) -- one cheat to a test: 5 s to
    8 s each, and 9 s once for the witness and the honest seal.  Host and device agree, with and without the control root."""
    s = cheats.subject(orc, "trace", r0.TRACE_MIN_PO2)
    handful = cheats.trace_handful(s.blob)
    assert len(handful) == TRACE_HANDFUL and [v for _, _, v in handful] == [6, 6, 6, 6, 6, 4, 6, 4]
    label, cheat, verdict = handful[k]
    seal = s.prove(cheat)
    assert seal.size == s.honest.size and not np.array_equal(seal, s.honest)
    assert s.oc.verify(seal) == (verdict, cheats.REASON[verdict]), label
    root = s.code_root()
    for roots in (None, [root, root]):
        want = [r0.verify_seal(s.blob, x, code_root=None if roots is None else root) for x in (seal, s.honest)]
        got = hal.verify_seals(s.blob, [seal, s.honest], roots)
        assert [g[:3] for g in got] == want, label
        assert want[1] == (0, "ok", s.po2)
        code_lie = roots is not None and cheat[0] == "committed" and cheat[1] == cheats.GROUP_NAMES.index("code")
        code = cheats.CODE_ROOT if code_lie else verdict
        assert want[0] == (code, cheats.REASON[code], s.po2), label
