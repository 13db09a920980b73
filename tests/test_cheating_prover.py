"""What the algebraic half of verification covers, without a GPU: seals of a cheating prover (tests/cheats.py; the oracle's sequencer
with one lie, orc_prove_segment_cheat) whose transcript and Merkle trees are valid, so that only the check that binds the lied-about
words can refuse them.  One sweep per kind of lie and circuit -- circuits/tiny.r0c and circuits/small.r0c at po2 9 and the three
families of tap_circuits.py (the 64-tap register, backs that are no prefix of 0, 1, 2, the lone {0, 63} combo) at their smallest
po2 -- over EVERY column of every group (committed; CODE, DATA and ACCUM also flowing into eval_check), every word of coeff_u, all 64
columns of the FRI round and every word of the final polynomial; at po2 13, where a proof has two FRI rounds and costs a quarter of a
second, a sample.  For every cheat: the seal is another seal of the honest one's length, the oracle's verifier and the product's
(r0h_verify_seal, csrc/verify.cpp) give the same verdict and reason, and the verdict is the one cheats.py derives for the kind from
the order of the checks -- never 0, and never a code of the transcript or of a Merkle path.

The times in the docstrings are a whole sweep's on the build machine (8 oracle threads), proofs and both verifications: at po2 9 a
proof takes 17 ms (tiny) to 22 ms (small), the oracle's verdict 1.4 ms and the product's 3 ms; at po2 13 a proof takes 0.24 s."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0

import cheats
from conftest import circuit_path

PO2 = 9
CIRCUITS = ("tiny", "small", "wide", "odd", "far")
COEFF_U_PARTS = cheats.COEFF_U_PARTS


def held(orc, name, po2, which, part=None, want=None):
    """every cheat of the sweep against both verifiers -> [(cheat, verdict)]; want: cheat -> the verdict it must get, where the kind
    allows more than one and the circuit says which"""
    s = cheats.subject(orc, name, po2)
    assert r0.verify_seal(s.blob, s.honest) == (0, "ok", po2)
    out = []
    for label, cheat, seal in cheats.cheating_seals(orc, name, po2, which, part):
        assert seal.size == s.honest.size and not np.array_equal(seal, s.honest), label
        oracle, product = s.oc.verify(seal), cheats.product_verdict(s.blob, seal)
        assert product == oracle + (po2,), "%s: the product says %r, the oracle %r" % (label, product, oracle)
        assert oracle[0] in cheats.ALLOWED[cheat[0]], "%s: %r" % (label, oracle)
        assert oracle[1] == cheats.REASON[oracle[0]], label
        if want is not None:
            assert oracle[0] == want(cheat), "%s: %r, the order of the checks gives %d" % (label, oracle, want(cheat))
        out.append((cheat, oracle[0]))
    assert out
    return out


@pytest.mark.parametrize("name", CIRCUITS)
def test_every_committed_column_of_every_group_is_bound_by_the_deep_comparison(orc, name):
    """CODE, DATA, ACCUM and CHECK, every column: the tree holds the lie, coeff_u and FRI are honest -- nothing but the DEEP value
    against FRI's first matrix can refuse, and it does (6).  0.4 s (far: 21 columns) to 2.1 s (small: 80)."""
    got = held(orc, name, PO2, "committed")
    assert len(got) == sum(cheats.group_sizes(cheats.subject(orc, name, PO2).blob))


@pytest.mark.parametrize("name", CIRCUITS)
def test_a_lie_that_flows_into_eval_check_fails_the_identity_at_z(orc, name):
    """CODE, DATA and ACCUM, every column: CHECK is made from the lying evaluations and the coefficients are not -- the constraint
    identity compares the two (4) before the DEEP comparison is reached.  0.1 s (far: 5 columns) to 1.4 s (small: 64)."""
    got = held(orc, name, PO2, "flowing")
    assert len(got) == sum(cheats.group_sizes(cheats.subject(orc, name, PO2).blob)[:3])


@pytest.mark.parametrize("part", range(COEFF_U_PARTS))
@pytest.mark.parametrize("name", CIRCUITS)
def test_every_word_of_coeff_u_is_bound(orc, name, part):
    """every word of every register's interpolant (the 64-tap one included) and of CHECK's sixteen openings, the prover's DEEP
    quotients following the lie: 4 where a term reads the register or the word is CHECK's, 6 (the dropped remainder) where none
    does -- cheats.coeff_u_verdict says which.  A third of the words to a test: 0.5 s (far: 88 words) to 3.8 s (small: 528)."""
    verdict = cheats.coeff_u_verdict(cheats.subject(orc, name, PO2).blob)
    got = held(orc, name, PO2, "coeff_u", (part, None, COEFF_U_PARTS), want=lambda cheat: verdict[cheat[1]])
    assert [c[1] for c, _ in got] == list(range(len(verdict)))[part::COEFF_U_PARTS]


@pytest.mark.parametrize("name", CIRCUITS)
def test_every_column_of_the_fri_round_is_bound_by_the_goal_or_by_the_fold(orc, name):
    """all 64 columns (4 components of 16 coset members) of the one round of a po2 9 proof: query 0 takes the goal comparison for the
    member its position picks (6) and the fold for the fifteen others (7, the final polynomial) -- a sweep sees both, so no member
    and no component is left out of either.  1.1 s to 2.1 s."""
    got = held(orc, name, PO2, "fri")
    assert len(got) == cheats.FRI_COLUMNS and {v for _, v in got} == {6, 7}, got
    members = {6: set(), 7: set()}
    for cheat, v in got:
        members[v].add(cheat[2] % 16)
    assert len(members[7]) == 16  # (a member takes the goal comparison only where query 0 picks it: which ones is the transcript's)


@pytest.mark.parametrize("name", CIRCUITS)
def test_every_word_of_the_final_polynomial_is_bound(orc, name):
    """all 128 words (4 components of 32 coefficients) of a po2 9 proof: 7 at query 0.  2.1 s to 3.8 s."""
    got = held(orc, name, PO2, "final")
    assert len(got) == 128


@pytest.mark.parametrize("which,part", zip(("round 0", "round 1", "committed"), (part for _, part in cheats.SAMPLE)))
def test_two_fri_rounds_at_po2_13(orc, which, part):
    """tiny at po2 13, the smallest proof with two rounds: one column per coset member of each round, the component rotating, and the
    first column of each group.  A lie in round 0 is caught by a goal comparison -- round 0's or, through the fold, round 1's (6) --
    and one in round 1 by its goal comparison or the final polynomial (6 or 7).  16 proofs: 4 s; the four columns: 1 s."""
    s = cheats.subject(orc, "tiny", 13)
    sample = cheats.sample_two_rounds(s.blob)
    assert [c[1:3] for _, c in sample[:32]] == [(rd, 16 * (i % 4) + i) for rd in (0, 1) for i in range(16)] and len(sample) == 36
    got = held(orc, "tiny", 13, "sample", part)
    assert len(got) == part[1] - part[0]
    if which == "round 0":
        assert {v for _, v in got} == {6}, got


def test_with_the_control_root_a_lie_about_a_code_column_is_another_program(orc):
    """tiny, every CODE column, committed and flowing: the CODE commitment is not the control root (10) in both verifiers before any
    algebra; without the root the kind's own verdict, as above.  0.2 s on top of the sweeps."""
    s = cheats.subject(orc, "tiny", PO2)
    root = s.code_root()
    assert s.oc.verify(s.honest, code_root=root) == (0, "ok") and r0.verify_seal(s.blob, s.honest, code_root=root) == (0, "ok", PO2)
    n = 0
    for kind in ("committed", "flowing"):
        for label, cheat, seal in cheats.cheating_seals(orc, "tiny", PO2, kind):
            bound = s.oc.verify(seal, code_root=root)
            assert r0.verify_seal(s.blob, seal, code_root=root)[:2] == bound, label
            if cheat[1] == cheats.GROUP_NAMES.index("code"):
                assert bound == (cheats.CODE_ROOT, cheats.REASON[cheats.CODE_ROOT]), label
                assert s.oc.verify(seal)[0] in cheats.ALLOWED[kind] and r0.verify_seal(s.blob, seal)[0] in cheats.ALLOWED[kind], label
                n += 1
            else:
                assert bound[0] in cheats.ALLOWED[kind], label
    assert n == 2 * cheats.group_sizes(s.blob)[1]


@pytest.mark.parametrize("name", cheats.KEPT)
def test_the_collecting_verifier_settles_on_the_same_query_without_a_device(orc, name):
    """every cheat of tiny and small, the honest seal among them, as one batch through r0h_verify_seals_on with no context: the walk of
    verify<true>, the openings hashed on the host, settle.  Every opening reaches its node, so each verdict is the first failing
    walk's, and must be the immediate verifier's.  2.2 s (tiny: 485 seals) and 2.8 s (small: 865) once the sweeps above have run."""
    s = cheats.subject(orc, name, PO2)
    cases = [("honest", None, s.honest)] + cheats.every_cheating_seal(orc, name, PO2)
    got = r0.verify_seals(s.blob, [seal for _, _, seal in cases])
    assert got[0][:3] == (0, "ok", PO2)
    for (label, _, seal), g in zip(cases, got):
        assert g[:3] == cheats.product_verdict(s.blob, seal), label


@pytest.mark.parametrize("name", ("tiny", "small", "bench", "recursion", "trace", "image") + tuple(cheats.tc.FAMILIES))
def test_every_column_belongs_to_a_register(name):
    """a column without a register is in no DEEP combination: nothing would bind what the prover commits for it.  Every shipped
    circuit and every family.  Milliseconds."""
    blob = cheats.tc.FAMILIES[name].blob() if name in cheats.tc.FAMILIES else np.fromfile(circuit_path(name), dtype=np.uint32)
    assert cheats.unregistered(blob) == []


def test_a_descriptor_that_names_no_word_of_the_proof_gives_no_seal(orc):
    """the hook's own bounds: a column, word or round past the end, a zero or non-canonical delta.  0.1 s."""
    s = cheats.subject(orc, "tiny", PO2)
    sizes = cheats.group_sizes(s.blob)
    words = 4 * (s.oc.n_taps + cheats.CHECK_SIZE)
    for cheat in [("committed", 4, 0, 1), ("committed", 3, 16, 1), ("committed", 1, sizes[1], 1), ("flowing", 3, 0, 1), ("flowing", 2, sizes[2], 1),
                  ("coeff_u", words, 0, 1), ("fri", 1, 0, 1), ("fri", 0, 64, 1), ("final", 128, 0, 1), ("final", 0, 0, 0), ("final", 0, 0, cheats.tc.P)]:
        with pytest.raises(AssertionError, match="names no word"):
            s.prove(cheat)
    assert np.array_equal(s.prove(None), s.honest)
