"""The log-derivative argument on the host: the exact reference (logup_ref.py) against the oracle and r0h_logup_multiplicities_host on
generated LOGUP circuits (logup_circuits.py), on the trace circuit's corner programs and on the image circuit; and the argument's
contract (include/r0hip_circuit.h, LOGUP) refused by both parsers and both host-side multiplicity counts.  The device gets the same
circuits in test_gpu_logup.py."""
import copy
import ctypes
import os
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import logup_circuits as lc
import logup_ref as ref
from trace_circuit import G_CODE, LF, ONE, Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = [0, 3, 5, 6, 7, 9]          # R16 gated / no table, a public total / R16 + AND x2 / R16, three public totals / ...
_vp = ctypes.c_void_p


def host_multiplicities(blob, po2, data, glob):
    blob, data = np.ascontiguousarray(blob, dtype=np.uint32), np.array(data, dtype=np.uint32)
    g = np.ascontiguousarray(glob if len(glob) else [0], dtype=np.uint32)
    r0._check(r0.lib().r0h_logup_multiplicities_host(blob.ctypes.data_as(_vp), blob.size, po2, data.ctypes.data_as(_vp), g.ctypes.data_as(_vp)))
    return data


def oracle_multiplicities_rc(orc, blob, po2, data, glob):
    """the oracle's return code (0 or -1), data left as it was"""
    oc = orc.circuit(blob)
    d = np.array(data, dtype=np.uint32)
    g = np.ascontiguousarray(glob if len(glob) else [0], dtype=np.uint32)
    return orc.L.orc_logup_multiplicities(oc.h, po2, d.ctypes.data_as(_vp), g.ctypes.data_as(_vp))


def oracle_parses(orc, blob):
    b = np.ascontiguousarray(blob, dtype=np.uint32)
    h = orc.L.orc_circuit_parse(b.ctypes.data_as(_vp), b.size)
    if h:
        orc.L.orc_circuit_free(h)
    return bool(h)


def library_parses(blob):
    try:
        r0.emit_eval_check_source(np.ascontiguousarray(blob, dtype=np.uint32))
    except r0.R0HipError:
        return False
    return True


def check_against_oracle(orc, blob, po2, code, data, glob, mix):
    """reference == oracle (== host) on multiplicities, ACCUM and the public totals; -> the witness with its multiplicities"""
    oc = orc.circuit(blob)
    want = ref.multiplicities(blob, data, glob, po2)
    if ref.parse(blob)["tables"]:
        assert np.array_equal(oc.logup_multiplicities(po2, data, glob), want)
        assert np.array_equal(host_multiplicities(blob, po2, data, glob), want)
    assert np.array_equal(ref.totals(blob, po2, code, want, glob), oc.logup_totals(po2, code, want, glob))
    assert np.array_equal(ref.accum(blob, po2, code, want, glob, mix), oc.accum_public(po2, code, want, glob, mix))
    return want


def test_the_generated_circuits_cover_what_the_committed_ones_do_not():
    cs = [lc.generate(s) for s in SEEDS]
    assert {tuple(c.kinds) for c in cs} == {(), (1,), (1, 2)}
    assert any(c.n_public for c in cs) and any(c.n_chain >= 3 for c in cs)
    gates = [g for c in cs for _, g, _ in c.lookups]
    assert None in gates and any(g and g[0] == "sel" for g in gates) and any(g and g[0] == "not" for g in gates)
    assert any(k == 2 for c in cs for k, _, _ in c.lookups)


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_equals_oracle_and_host_on_a_generated_circuit(orc, seed):
    c = lc.generate(seed)
    po2 = 16
    data, glob, mix = c.witness(po2, seed=1)
    code = orc.circuit(c.words).witgen(po2, 0)[0]
    want = check_against_oracle(orc, c.words, po2, code, data, glob, mix)
    # gated-off rows look up values outside the table and are not counted; a count is the rows whose numerator is 1
    for k in c.kinds:
        m = ref.dec(want.reshape(-1, 1 << po2)[c.mult[k]])
        on = sum(int((num == 1).sum()) for kind, num, _ in ref.lookups(c.words, po2, data, glob) if kind == k)
        assert int(m.sum()) == on


@pytest.mark.parametrize("name", ["mext", "alu", "memory", "control", "ecall"])
def test_reference_equals_oracle_and_host_on_the_trace_circuit(orc, name):
    import trace_corners as tcr
    blob = np.fromfile(os.path.join(ROOT, "circuits", "trace.r0c"), dtype=np.uint32)
    po2 = r0.TRACE_MIN_PO2
    vm = tcr.run(tcr.PROGRAMS[name](), expect=(0, 0x00050003) if name == "ecall" else (0, 0))
    data, glob = vm.trace_witness(0, po2)          # multiplicities counted by r0h_logup_multiplicities_host
    rng = np.random.default_rng(len(name))
    glob = np.array(glob, dtype=np.uint32)
    glob[r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS:] = rng.integers(0, ref.P, size=r0.TRACE_LATE_GLOBALS)
    mix = rng.integers(0, ref.P, size=orc.circuit(blob).n_mix).astype(np.uint32)
    code = orc.circuit(blob).witgen(po2, 0)[0]
    zeroed = data.reshape(-1, 1 << po2).copy()
    tables = ref.parse(blob)["tables"]
    for col, _ in tables:
        zeroed[col] = 0
    want = check_against_oracle(orc, blob, po2, code, zeroed.reshape(-1), glob, mix)
    assert np.array_equal(want, data.reshape(-1))


def test_reference_equals_oracle_on_the_image_circuit(orc):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    blob = np.fromfile(os.path.join(ROOT, "circuits", "image.r0c"), dtype=np.uint32)
    elf = elf_of(_guest(40), 0x400)
    po2 = r0.image_po2(elf)
    data, glob = r0.image_witness(elf, po2)
    glob[r0.IMAGE_GAMMA:r0.IMAGE_GAMMA + 16] = np.random.default_rng(5).integers(0, ref.P, size=16)
    oc = orc.circuit(blob)
    code = oc.witgen(po2, 0)[0]
    mix = np.random.default_rng(6).integers(0, ref.P, size=oc.n_mix).astype(np.uint32)
    check_against_oracle(orc, blob, po2, code, data.reshape(-1), glob, mix)
    assert ref.totals(blob, po2, code, data.reshape(-1), glob)[r0.IMAGE_GAMMA + 16:].any()


# ---- the contract: one rule broken at a time
def _tables(c):
    return [(c.mult[k], k) for k in c.kinds]


def _break(rule):
    """-> the blob of a generated circuit (R16 + AND, a public total) with exactly one rule of the contract broken"""
    c = lc.generate(5)
    assert c.kinds == [1, 2] and c.n_public >= 1
    accs, tables = copy.deepcopy(c.accs), _tables(c)
    looks = [(j, i) for j, (frs, fin) in enumerate(accs) for i, f in enumerate(frs) if f.table]
    j, i = looks[0]
    f = accs[j][0][i]
    if rule == "three fractions":
        accs[-1] = (accs[-1][0][:3], accs[-1][1])
    elif rule == "table kind":         # the AND table alone, as table 1
        tables = [(c.mult[2], 2)]
        for frs, _ in accs:
            for g in frs:
                if g.table == 1:
                    g.table = 0
                    g.num = LF()
                elif g.table == 2:
                    g.table = 1
    elif rule == "table index":        # a lookup names table 2 of 1
        tables = [(c.mult[1], 1)]
        for frs, _ in accs:
            for g in frs:
                if g.table == 2:
                    g.num = LF()
                    g.parts = [(("mix", 0), ONE), (("one",), -LF.col(c.free[0]))]
    elif rule == "public lookup":      # a lookup in the accumulator with a public total
        pub = accs[-1][0]
        pub[0], accs[j][0][i] = accs[j][0][i], pub[0]
    elif rule == "numerator reads CODE":
        f.num = LF.col(lc.CODE_RANDOM, G_CODE)
    elif rule == "value reads CODE":
        f.parts[1] = (f.parts[1][0], f.parts[1][1] + LF.col(lc.CODE_RANDOM, G_CODE))
    return lc.replace_logup(c.words, lc.logup_words(accs, tables))


RULES = ["three fractions", "table kind", "table index", "public lookup", "numerator reads CODE", "value reads CODE"]


def test_the_unbroken_circuit_parses(orc):
    assert library_parses(_break(None)) and oracle_parses(orc, _break(None))


@pytest.mark.parametrize("rule", RULES)
def test_both_parsers_refuse_a_circuit_that_breaks_the_contract(orc, rule):
    blob = _break(rule)
    assert not library_parses(blob), rule
    assert not oracle_parses(orc, blob), rule


def _error_cases(c, po2, seed=1):
    """-> {name: (data, glob)}: witnesses that break the contract at one row"""
    data, glob, _ = c.witness(po2, seed)
    n = 1 << po2
    out = {}
    d = data.reshape(-1, n).copy()
    for s in c.sel:
        d[s, 5] = ref.enc(2)
    out["numerator 2"] = (d.reshape(-1), glob)
    kind, gate, cols = next(x for x in c.lookups if x[1] is None and x[0] == 1)
    d = data.reshape(-1, n).copy()
    k_p = cols[1]
    d[cols[0], 7] = ref.enc((int(ref.dec(d[cols[0], 7])) + 65536 * pow(k_p, ref.P - 2, ref.P)) % ref.P)   # value + 65536
    out["outside R16"] = (d.reshape(-1), glob)
    kind, gate, cols = next(x for x in c.lookups if x[1] is None and x[0] == 2)
    d = data.reshape(-1, n).copy()
    d[cols[2], 9] = ref.enc(int(ref.dec(d[cols[2], 9])) ^ 1)                                              # r != a & b
    out["outside AND"] = (d.reshape(-1), glob)
    return out


ERROR_SEED = 17


def test_error_circuit_has_what_the_error_cases_need():
    c = lc.generate(ERROR_SEED, tables=[1, 2], n_chain=4)
    assert any(g for _, g, _ in c.lookups) and any(k == 1 and g is None for k, g, _ in c.lookups) and any(k == 2 and g is None for k, g, _ in c.lookups)


@pytest.mark.parametrize("case", ["numerator 2", "outside R16", "outside AND"])
def test_host_and_oracle_refuse_a_witness_that_breaks_the_contract(orc, case):
    c = lc.generate(ERROR_SEED, tables=[1, 2], n_chain=4)
    data, glob = _error_cases(c, 16)[case]
    with pytest.raises(ref.LogupError):
        ref.multiplicities(c.words, data, glob, 16)
    with pytest.raises(r0.R0HipError):
        host_multiplicities(c.words, 16, data, glob)
    assert oracle_multiplicities_rc(orc, c.words, 16, data, glob) == -1


def many_lookups_blob(n_acc):
    """one R16 table and 4 n_acc - 1 ungated lookups of DATA column 1: 123 of them at 2^24 rows are more than p - 1"""
    look = Fraction("l", ONE, [(("mix", 0), ONE), (("one",), -LF.col(1))], 1)
    table = Fraction("t", -LF.col(0), [(("mix", 0), ONE), (("one",), -LF.col(3, G_CODE))])
    frs = [table] + [look] * (4 * n_acc - 1)
    accs = [(frs[4 * j:4 * j + 4], None) for j in range(n_acc)]
    code_cols = [(0, 0), (1, 0), (3, 7), (4, 0)]
    taps = sorted([(0, c, 0) for c in range(4 * n_acc)] + [(1, c, 0) for c in range(4)] + [(2, c, 0) for c in range(2)])
    return lc.blob(n_acc, 4, 2, taps, 0, 4, 0, [(7, 0, 0, 0)], code_cols, lc.logup_words(accs, [(0, 1)]))


def test_more_than_p_minus_1_lookups_of_a_table_are_refused(orc):
    blob = many_lookups_blob(31)
    assert library_parses(blob) and oracle_parses(orc, blob)
    data = np.zeros(2 << 16, dtype=np.uint32)
    data[(1 << 16) + 5] = ref.enc(4096)
    m = host_multiplicities(blob, 16, data, [])
    assert np.array_equal(m, ref.multiplicities(blob, data, [], 16))
    assert int(ref.dec(m[4096])) == 123 and int(ref.dec(m[0])) == 123 * ((1 << 16) - 1)
    data = np.zeros(2 << 24, dtype=np.uint32)
    with pytest.raises(ref.LogupError):
        ref.multiplicities(blob, data, [], 24)
    with pytest.raises(r0.R0HipError, match="p - 1"):
        host_multiplicities(blob, 24, data, [])
    assert oracle_multiplicities_rc(orc, blob, 24, data, []) == -1
