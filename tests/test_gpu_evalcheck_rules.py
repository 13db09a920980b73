"""The generated kernels on the device against the structural rules of their generator (csrc/evalcheck_emit.cpp): r0h_eval_check
on the hand-built circuits of evalcheck_circuits.py and their cut variants, bit-equal to the oracle and to the plain reference
(evalcheck_ref.py) under the corner, all-(p - 1), near-p and random operand families; the code objects the build ships against the oracle
at kernel level (the first comparison of the multi-kernel accumulate path); and r0h_check_witness on planted witnesses against
check_ref.  The CPU side -- the same circuits through an exact-width interpretation of the text -- is tests/test_evalcheck_rules.py."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from conftest import circuit_path

import evalcheck_circuits as hand
import evalcheck_ref
import field_words
from test_evalcheck_rules import SHARP, poly_mix_of

pytestmark = pytest.mark.gpu
P = field_words.P
FILL = 0xA5A5A5A5  # no field word: a kernel that adds into the buffer instead of overwriting it cannot hide
GUARD = 4


@pytest.fixture(scope="module")
def circuits(hal):
    """(family, budget) -> the circuit loaded under that R0H_EC_BUDGET, compiled in-process, once per module"""
    held = {}
    yield held
    for gc in held.values():
        gc.free()


def loaded(hal, circuits, case, monkeypatch):
    if case not in circuits:
        name, budget = case
        if budget is None:
            monkeypatch.delenv("R0H_EC_BUDGET", raising=False)
        else:
            monkeypatch.setenv("R0H_EC_BUDGET", str(budget))  # read when the circuit is loaded
        blob = hand.FAMILIES[name]()
        assert hand.kernels_in(r0.emit_eval_check_source(blob)) == (1 if budget is None else hand.CUTS[case])
        circuits[case] = hal.load_circuit(blob)
    return circuits[case]


def device_eval_check(hal, gc, po2, ea, ec, ed, glob, mix, pm):
    """r0h_eval_check into a buffer pre-filled with FILL and followed by GUARD words: the 4 x 4N result words, all below p, with
    the guard intact"""
    words = 16 << po2
    check = hal.copy_from(np.full(words + GUARD, FILL, dtype=np.uint32))
    bufs = [hal.copy_from(x) for x in (ea, ec, ed)]
    (_, pg), (_, pmx), (_, pq) = r0._u32arr(glob), r0._u32arr(mix), r0._u32arr(pm)
    r0._check(r0.lib().r0h_eval_check(hal.ctx, gc.handle, po2, bufs[0].handle, bufs[1].handle, bufs[2].handle, pg, pmx, pq, check.handle))
    out = check.to_host()
    for b in bufs + [check]:
        b.free()
    assert np.all(out[words:] == FILL), "eval_check wrote past the end of check"
    assert np.all(out[:words] < P), "a result word is not canonical"
    return out[:words]


_WANT = {}  # (family, po2, operand kind) -> (operands, poly_mix, the oracle's check): computed once, shared by the cut variants


def expected(orc, name, po2, kind):
    key = (name, po2, kind)
    if key not in _WANT:
        blob = hand.FAMILIES[name]()
        words = "top" if kind in SHARP else kind
        rng = np.random.default_rng([13, po2, len(kind)])
        oc = orc.circuit(blob)
        ops = [hand.words(rng, size * (4 << po2), words) for size in oc.group_size]
        ops += [hand.words(rng, hand.N_GLOBAL, words), hand.words(rng, hand.N_MIX, words)]
        pm = np.array(SHARP[kind][0], dtype=np.uint32) if kind in SHARP else poly_mix_of(kind, po2)
        want = oc.eval_check(po2, *ops, pm)
        assert np.array_equal(want, evalcheck_ref.eval_check(blob, po2, *ops, pm))  # the second witness
        for a in ops + [want]:
            a.setflags(write=False)
        _WANT[key] = (ops, pm, want)
    return _WANT[key]


# ---- a. the hand circuits and their cut variants
@pytest.mark.parametrize("po2", [6, 7])  # the 4N domain is exactly one block, and two
@pytest.mark.parametrize("case", hand.cases(), ids=hand.case_id)
def test_eval_check_on_the_hand_circuits(hal, orc, circuits, case, po2, monkeypatch):
    gc = loaded(hal, circuits, case, monkeypatch)
    kinds = list(hand.KINDS) + (sorted(SHARP) if case[0] == "bare9" else [])
    for kind in kinds:
        ops, pm, want = expected(orc, case[0], po2, kind)
        got = device_eval_check(hal, gc, po2, *ops, pm)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d words differ, first at component %d, point %d" % (kind, bad.size, bad[0] // (4 << po2), bad[0] % (4 << po2))


# ---- b. the code objects the build ships
@pytest.mark.parametrize("name", ["small", "bench", "recursion", "trace", "image"])
def test_eval_check_of_the_shipped_code_objects_is_the_oracles(hal, orc, name):
    po2 = 6
    blob = np.fromfile(circuit_path(name), dtype=np.uint32)
    oc = orc.circuit(blob)
    gc = hal.load_circuit(blob, entry.code_object_path(name))
    assert hand.kernels_in(r0.emit_eval_check_source(blob)) == {"small": 1, "bench": 3, "recursion": 2, "trace": 1, "image": 1}[name]
    for kind in ("pool", "top", "near"):
        rng = np.random.default_rng([17, len(name), len(kind)])
        ops = [hand.words(rng, size * (4 << po2), kind) for size in oc.group_size]
        ops += [hand.words(rng, max(oc.n_global, 1), kind), hand.words(rng, max(oc.n_mix, 1), kind)]
        pm = poly_mix_of(kind, 5)
        assert np.array_equal(device_eval_check(hal, gc, po2, *ops, pm), oc.eval_check(po2, *ops, pm)), kind
    gc.free()


# ---- c. the witness checker on planted witnesses
@pytest.mark.parametrize("po2", [6, 8, 9])
@pytest.mark.parametrize("case", [c for c in hand.cases() if c[0] in ("gates", "taps")], ids=hand.case_id)
def test_check_witness_on_planted_witnesses(hal, circuits, case, po2, monkeypatch):
    gc = loaded(hal, circuits, case, monkeypatch)
    for rows, (accum, code, data, glob, mix), want, early in hand.planted_cases(case[0], po2):
        bufs = [hal.copy_from(x) for x in (accum, code, data)]
        got = {t: (cnt, first) for t, cnt, first in hal.check_witness(gc, po2, bufs[1], bufs[2], glob, bufs[0], mix)}
        got_early = {t: (cnt, first) for t, cnt, first in hal.check_witness(gc, po2, bufs[1], bufs[2], glob)}
        for b in bufs:
            b.free()
        assert got == want, (rows, got, want)
        assert got_early == early, (rows, got_early, early)
