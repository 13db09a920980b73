"""CPU side of the generator's structural rules (csrc/evalcheck_emit.cpp) on the hand-built circuits of evalcheck_circuits.py:
the plain reference (evalcheck_ref.py) against the oracle, and the emitted text, interpreted on exact-width integers
(evalcheck_text.py), against the oracle on a few lanes with no unsigned sum wrapping -- under every operand family, every cut
variant, and for the six committed circuits.  The device's side is tests/test_gpu_evalcheck_rules.py."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import circuit_path

import check_ref
import evalcheck_circuits as hand
import evalcheck_ref
import evalcheck_text
import field_words

P = field_words.P
COMMITTED = ("tiny", "small", "bench", "recursion", "trace", "image")
# poly_mix words (Montgomery form) at which a looser cadence of the running sums wraps on nine bare terms at p - 1 while the
# generator's does not: evalcheck_text.find_sharp_poly_mix(seed, first, every, 9), the first hit among 2^20 candidates
SHARP_SEED = 20240611
SHARP_FIRST_AT_6 = (1096638445, 1584394041, 609149216, 294507771)  # cadence (6, 2): the first correction before product 6 instead of 4
SHARP_EVERY_THIRD = (872365935, 1736690956, 1836686585, 1188979332)  # cadence (4, 3): a correction before every third product
SHARP = {"first_at_6": (SHARP_FIRST_AT_6, 6, 2), "every_third": (SHARP_EVERY_THIRD, 4, 3)}


def hand_blob(case, monkeypatch):
    """the blob of a hand circuit with R0H_EC_BUDGET set as the case asks (the emitter and r0h_circuit_load read it per call)"""
    name, budget = case
    if budget is None:
        monkeypatch.delenv("R0H_EC_BUDGET", raising=False)
    else:
        monkeypatch.setenv("R0H_EC_BUDGET", str(budget))
    return hand.FAMILIES[name]()


def lanes_of(po2):
    domain = 4 << po2
    return [0, 1, 2, 3, domain // 2 + 5, domain - 1]


def poly_mix_of(kind, seed):
    return field_words.point(np.random.default_rng(seed), "top" if kind == "top" else "random")


@pytest.mark.parametrize("case", hand.cases(), ids=hand.case_id)
def test_every_cut_variant_has_the_kernels_it_claims(case, monkeypatch):
    blob = hand_blob(case, monkeypatch)
    pr = check_ref.Program(blob)
    want = 1 if case[1] is None else hand.CUTS[case]
    src, chk = r0.emit_eval_check_source(blob), r0.emit_check_witness_source(blob)
    assert hand.kernels_in(src) == hand.kernels_in(chk) == want
    assert src.count("void eval_check_") == chk.count("void check_witness_") == want
    if case[1] == 1:
        assert want == len(pr.terms)  # every term its own kernel
    text = evalcheck_text.Text(src)
    assert text.powers_used() == {t: t for t in range(len(pr.terms))}  # an empty inner chain takes no power
    # the terms that wait for the accumulation sit under the switch of the kernel they were cut into, after its early terms
    home = {}
    for k, part in enumerate(chk.split("void check_witness_")[1:]):
        early, _, late = part.partition("  if (with_accum) {\n")
        home.update({int(x.split("u,")[0]): (k, False) for x in early.split("  tally(table, ")[1:]})
        home.update({int(x.split("u,")[0]): (k, True) for x in late.split("  tally(table, ")[1:]})
    assert [home[t][1] for t in range(len(pr.terms))] == pr.late
    assert [home[t][0] for t in range(len(pr.terms))] == [k for k, kernel in enumerate(text.kernels) for st in kernel if st[0] == "term"]
    if case[1] is not None and case[0] in ("gates", "taps"):
        assert len({home[t][0] for t in range(len(pr.terms)) if pr.late[t]}) >= 2  # late terms in at least two kernels


def test_the_cut_variants_cut_between_two_readers_of_one_sub_expression(monkeypatch):
    """lazy's terms 3 and 4 read one sum: under every cut budget they lie in different kernels, and both kernels define it"""
    for case in sorted(c for c in hand.CUTS if c[0] == "lazy"):
        text = evalcheck_text.Text(r0.emit_eval_check_source(hand_blob(case, monkeypatch)))
        home = {st[1]: k for k, kernel in enumerate(text.kernels) for st in kernel if st[0] == "term"}
        assert home[3] != home[4]
        value = {st[1]: st[3] for kernel in text.kernels for st in kernel if st[0] == "term"}[4]
        for k in (home[3], home[4]):
            assert any(st[0] == "var" and st[1] == value for st in text.kernels[k])


@pytest.mark.parametrize("kind", hand.KINDS)
@pytest.mark.parametrize("po2", [6, 7])
@pytest.mark.parametrize("name", sorted(hand.FAMILIES) + ["tiny", "small"])
def test_the_plain_reference_is_the_oracles_eval_check(orc, name, po2, kind):
    blob = hand.FAMILIES[name]() if name in hand.FAMILIES else np.fromfile(circuit_path(name), dtype=np.uint32)
    oc = orc.circuit(blob)
    rng = np.random.default_rng([7, po2, len(kind)])
    ea, ec, ed = (hand.words(rng, size * (4 << po2), kind) for size in oc.group_size)
    glob, mix = hand.words(rng, max(oc.n_global, 1), kind), hand.words(rng, max(oc.n_mix, 1), kind)
    pm = poly_mix_of(kind, po2)
    assert np.array_equal(evalcheck_ref.eval_check(blob, po2, ea, ec, ed, glob, mix, pm), oc.eval_check(po2, ea, ec, ed, glob, mix, pm))


def interpret_against_the_oracle(orc, blob, po2, kind, pm, seed=11):
    oc = orc.circuit(blob)
    domain = 4 << po2
    rng = np.random.default_rng([seed, po2, len(kind)])
    ea, ec, ed = (hand.words(rng, size * domain, kind) for size in oc.group_size)
    glob, mix = hand.words(rng, max(oc.n_global, 1), kind), hand.words(rng, max(oc.n_mix, 1), kind)
    want = oc.eval_check(po2, ea, ec, ed, glob, mix, pm).reshape(4, domain)
    text = evalcheck_text.Text(r0.emit_eval_check_source(blob))
    got = evalcheck_text.run(text, po2, lanes_of(po2), ea, ec, ed, glob, mix, pm)  # raises if a sum wraps
    for i, words in got.items():
        assert words == [int(x) for x in want[:, i]], (i, kind)


@pytest.mark.parametrize("kind", hand.KINDS)
@pytest.mark.parametrize("case", hand.cases(), ids=hand.case_id)
def test_the_emitted_text_computes_the_oracles_eval_check_and_nothing_wraps(orc, case, kind, monkeypatch):
    blob = hand_blob(case, monkeypatch)
    for po2 in (6, 7):
        interpret_against_the_oracle(orc, blob, po2, kind, poly_mix_of(kind, po2))


@pytest.mark.parametrize("name", COMMITTED)
def test_the_emitted_text_of_the_committed_circuits(orc, name, monkeypatch):
    monkeypatch.delenv("R0H_EC_BUDGET", raising=False)
    blob = np.fromfile(circuit_path(name), dtype=np.uint32)
    for kind in hand.KINDS:
        interpret_against_the_oracle(orc, blob, 6, kind, poly_mix_of(kind, 3))


@pytest.mark.parametrize("which", sorted(SHARP))
@pytest.mark.parametrize("case", [("bare9", None), ("bare9", 30)], ids=hand.case_id)
def test_sharp_poly_mix_for_the_cadence_of_the_running_sums(orc, which, case, monkeypatch):
    """Under the committed poly_mix a looser cadence would wrap a running sum (the model in evalcheck_text.cadence_wraps says so),
    the generator's does not, and its text, all operands p - 1, gives the oracle's words"""
    pm, first, every = SHARP[which]
    assert pm is not None, "no sharp poly_mix was found for this cadence"
    pm = np.array(pm, dtype=np.uint32)
    m = np.array(evalcheck_text.mix_powers(pm, 9), dtype=np.uint64).reshape(1, 9, 4)
    assert evalcheck_text.cadence_wraps(m, first, every, 9)[0] and not evalcheck_text.cadence_wraps(m, 4, 2, 9)[0]
    blob = hand_blob(case, monkeypatch)
    for po2 in (6, 7):
        interpret_against_the_oracle(orc, blob, po2, "top", pm)


@pytest.mark.parametrize("which", sorted(SHARP))
def test_the_sharp_poly_mix_is_what_the_seeded_search_finds(which):
    pm, first, every = SHARP[which]
    assert evalcheck_text.find_sharp_poly_mix(SHARP_SEED, first, every, 9) == list(pm)


def test_the_interpreter_notices_a_wrap_and_an_unknown_line():
    """the checks the tests above lean on, shown to bite: two uncorrected sums in one product, products with no correction"""
    with pytest.raises(evalcheck_text.Wrap):
        evalcheck_text.fmul(2 * P - 2, 2 * P - 3)
    assert evalcheck_text.fmul(2 * P - 2, P - 1) < P
    src = r0.emit_eval_check_source(hand.bare(33))
    with pytest.raises(evalcheck_text.Unknown):
        evalcheck_text.Text(src.replace("4u * (back)", "4u + (back)"))
    assert evalcheck_text.Text(src.replace("4u * (back)", "(back)")).stride == 1
    text = evalcheck_text.Text(src.replace("  T0 = dfix(T0); T1 = dfix(T1); T2 = dfix(T2); T3 = dfix(T3);\n", ""))
    top = np.full(33 * 256, P - 1, dtype=np.uint32)
    one = np.zeros(256, dtype=np.uint32)
    with pytest.raises(evalcheck_text.Wrap):
        evalcheck_text.run(text, 6, [0], one, one, top, [0, 0], [0, 0], [P - 1] * 4)


def lazy_sums(blob):
    """{variable: emitted uncorrected?} over the ADD steps, read from the text (every kernel must agree)"""
    text = evalcheck_text.Text(r0.emit_eval_check_source(blob))
    out = {}
    for kernel in text.kernels:
        for st in kernel:
            if st[0] == "var" and st[2][0] in ("lazy", "fadd"):
                assert out.setdefault(st[1], st[2][0] == "lazy") == (st[2][0] == "lazy")
    return out


@pytest.mark.parametrize("name", sorted(hand.FAMILIES) + list(COMMITTED))
def test_which_sums_stay_uncorrected(name, monkeypatch):
    """The rules of lazy_additions, stated on the program and checked on the text.  Some of them are stricter than today's
    arithmetic needs (a gate is only ever multiplied by a corrected value), so no operand can tell them from their absence: the
    text can.  An uncorrected sum is read by products only -- it is no term's value, no gate, no operand of ADD or SUB; and no
    product reads two of them, a square counting twice."""
    monkeypatch.delenv("R0H_EC_BUDGET", raising=False)
    blob = hand.FAMILIES[name]() if name in hand.FAMILIES else np.fromfile(circuit_path(name), dtype=np.uint32)
    pr = check_ref.Program(blob)
    lazy = lazy_sums(blob)
    is_lazy = lambda v: lazy.get(v, False)
    for v, (op, a, b, _) in enumerate(pr.fp):
        if op in (check_ref.OP_ADD, check_ref.OP_SUB):
            assert not is_lazy(a) and not is_lazy(b), "v%d: an uncorrected operand of ADD/SUB" % v
        if op == check_ref.OP_MUL:
            assert is_lazy(a) + is_lazy(b) <= 1 and not (a == b and is_lazy(a)), "v%d: two uncorrected operands" % v
    for t, (v, gates) in enumerate(pr.terms):
        assert not is_lazy(v) and not any(is_lazy(g) for g in gates), "term %d: an uncorrected value or gate" % t
    if name == "lazy":
        # and the sums that may stay uncorrected do.  In creation order: one of term 0's two; not the squared one, nor the one a
        # SUB reads, nor the term's value, nor the gate; the one of (s x) s; neither operand of the sum of two sums, but that sum;
        # the sums times a constant, a public input, a mix word
        flags = [lazy[v] for v in sorted(lazy)]
        assert sorted(flags[:2]) == [False, True]
        assert flags[2:] == [False, False, False, False, True, False, False, True, True, True, True]
    if name in COMMITTED:
        assert any(lazy.values())  # the rule is in use on every committed circuit


@pytest.mark.parametrize("po2", [6, 8, 9])
@pytest.mark.parametrize("case", [c for c in hand.cases() if c[0] in ("gates", "taps")], ids=hand.case_id)
def test_the_checkers_text_tallies_what_the_reference_does(case, po2, monkeypatch):
    """the witness checker's text on the planted witnesses the device gets: taps at row (i - back) mod N, every term under its own
    number, the late terms under the switch and only there"""
    text = evalcheck_text.CheckText(r0.emit_check_witness_source(hand_blob(case, monkeypatch)))
    assert text.stride == 1
    cases = hand.planted_cases(case[0], po2)
    if po2 > 6 and case[1] is not None:
        cases = cases[:2]  # every row is interpreted in Python: the cut variants get all row sets at 64 rows, two of them above
    for rows, (accum, code, data, glob, mix), want, early in cases:
        assert evalcheck_text.run_check(text, po2, code, data, glob, accum, mix) == want, rows
        assert evalcheck_text.run_check(text, po2, code, data, glob) == early, rows
