"""CPU side of the balance check (r0h_logup_check_balance): the host function against the numpy restatement (tests/balance_ref.py) on
tuple circuits (tests/balance_circuits.py) and generated LOGUP circuits, and on the trace circuit at 2^16 rows -- silent on an honest
witness, and naming the fractions and rows tools/trace_circuit.check_fractions names on three single-cell alterations; the fraction
names; the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_circuit  # noqa: E402
import trace_circuit as tc  # noqa: E402
import trace_corners as corners  # noqa: E402
from trace_corners import COL, P, R_INV, canonical  # noqa: E402

import balance_circuits as bc  # noqa: E402
import balance_ref as br  # noqa: E402
import logup_circuits as lc  # noqa: E402
import logup_ref as ref  # noqa: E402

PO2 = r0.TRACE_MIN_PO2
N = 1 << PO2


def host(blob, po2, code, data, glob):
    return r0.logup_check_balance_host(blob, po2, code, data, glob)


@pytest.mark.parametrize("po2", [4, 9])
@pytest.mark.parametrize("name", bc.SCENARIOS)
def test_host_equals_the_reference_on_tuple_circuits(name, po2):
    c, data, glob = bc.scenario(name, po2)
    want = br.check(c.words, po2, None, data, glob)
    assert want == br.check(c.words, po2, None, data, glob, whole_vectors=True)
    assert host(c.words, po2, None, data, glob) == want
    assert (want == []) == (name in bc.BALANCED)
    n = 1 << po2
    if name == "surplus":
        assert want == [(0, 0, 1, 2 * n + 1)]
    if name == "own class":
        assert len(want) == 8 * n and want[:9] == [(f, 0, 1, 1) for f in range(8)] + [(0, 1, 1, 1)]
        few, total = r0.logup_check_balance_host(c.words, po2, None, data, glob, capacity=8)
        assert total == 8 * n and few == want[:8]
    if name == "permutation":  # one consumed value altered: the tuple nobody produced, and the one nobody consumes any more
        bad = data.copy()
        row = n // 2
        bad[2 * n + row] = ref.enc((int(ref.dec(bad[2 * n + row])) + 1) % P)
        want = br.check(c.words, po2, None, bad, glob)
        produced = int(np.nonzero(ref.dec(data[n:2 * n]) == ref.dec(data[3 * n + row]))[0][0])   # (the second coordinate is the producer's row)
        assert sorted(want) == sorted([(1, row, P - 1, 1), (0, produced, 1, 1)])
        assert host(c.words, po2, None, bad, glob) == want


@pytest.mark.parametrize("po2", [4, 9])
def test_more_identities_than_a_session_has_room_for(po2):
    """eleven challenge identities under the chain: the host's walk has no limit of eight"""
    c, data, glob = bc.scenario("many identities", po2)
    assert len({(kind, idx if kind else 0) for _, f in br.chain_fractions(ref.parse(c.words)) for kind, idx, _ in f["parts"]}) == 11
    assert br.check(c.words, po2, None, data, glob) == []
    n = 1 << po2
    for column, row in ((6, n // 2), (0, n - 1)):   # a consumed value of the second pair, a produced one of the first
        bad = bc.altered(data, po2, column, row)
        want = br.check(c.words, po2, None, bad, glob)
        assert len(want) == 2 and sorted(net for _, _, net, _ in want) == [1, P - 1] and row in [r for _, r, _, _ in want]
        assert host(c.words, po2, None, bad, glob) == want


@pytest.mark.parametrize("tables", [[1], [1, 2]])
def test_host_equals_the_reference_on_generated_lookup_circuits(orc, tables):
    c = lc.generate(7, tables=tables, n_chain=3, n_public=1)
    code = orc.circuit(c.words).witgen(16, 0)[0]
    data, glob, _ = c.witness(16, seed=2)
    want = br.check(c.words, 16, code, data, glob)           # multiplicities left zero: every looked-up value's class is reported
    assert want and host(c.words, 16, code, data, glob) == want
    assert all(net == members for _, _, net, members in want)  # (lookups alone, numerator 1 each)
    full = ref.multiplicities(c.words, data, glob, 16)
    assert br.check(c.words, 16, code, full, glob) == [] == host(c.words, 16, code, full, glob)


@pytest.fixture(scope="module")
def trace():
    """the host witness of a corner program at 2^16 rows, multiplicities filled (r0h_vm_trace_witness, r0h_logup_multiplicities_host)"""
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    vm = corners.run(corners.PROGRAMS["alu"]())
    data, glob = vm.trace_witness(0, PO2)
    code = ref.enc(np.array(tc.code_columns(N), dtype=np.int64)).reshape(-1)
    return blob, code, data, glob, len(vm.preflight(0))


ALTERATIONS = ("register read", "multiplicity + 1", "multiplicity - 1", "boundary value")


def trace_alteration(what, m, n_rows):
    """(column, row, new canonical value) on the canonical witness m [column, row]: one register-read value cell of one cycle (memory
    tuples alone move), one multiplicity entry + 1 or - 1 (a value few lookups ask for: check_fractions names four fractions and eight
    rows of a class at the most), one boundary row's value"""
    mid = n_rows // 2
    first_boundary = int(np.nonzero(m[COL["bnd"]])[0][0])
    column, row, step = {"register read": ("rs1_lo", mid, 1), "multiplicity + 1": ("m16", 5, 1), "multiplicity - 1": ("m16", 5, -1),
                         "boundary value": ("after_lo", first_boundary, 1)}[what]
    return column, row, (int(m[COL[column], row]) + step) % P


def chained(bad):
    """check_fractions' findings among the chain links (the session sum closes across segments: not this check's)"""
    return [(nm, rows) for nm, rows, _ in bad if not nm.startswith("session:")]


def test_the_trace_circuit_balances_on_an_honest_witness(trace):
    blob, code, data, glob, n_rows = trace
    assert host(blob, PO2, code, data, glob) == [] == br.check(blob, PO2, code, data, glob)
    assert chained(tc.check_fractions(canonical(data, PO2).astype(np.int64), [int(x) * R_INV % P for x in glob])) == []


@pytest.mark.parametrize("what", ALTERATIONS)
def test_an_altered_trace_witness_names_what_check_fractions_names(trace, what):
    blob, code, data, glob, n_rows = trace
    names = gen_circuit.fraction_names("trace")
    m = canonical(data, PO2).astype(np.int64)
    column, row, value = trace_alteration(what, m, n_rows)
    bad = data.copy()
    bad[COL[column] * N + row] = ref.enc(value)
    got = host(blob, PO2, code, bad, glob)
    print(what, [(names[f], r, net, members) for f, r, net, members in got])
    assert got and got == br.check(blob, PO2, code, bad, glob)
    m[COL[column], row] = value
    theirs = chained(tc.check_fractions(m, [int(x) * R_INV % P for x in glob]))
    assert len(theirs) == len(got) < 64
    assert sorted(r for _, r, _, _ in got) == sorted(rows[0] for _, rows in theirs)
    for f, r, _, members in got:
        rows = next(rows for nm, rows in theirs if rows[0] == r and names[f] in nm.split("|"))
        assert len(rows) <= min(members, 8)
    if what == "register read":
        assert {names[f].split(":")[0] for f, _, _, _ in got} == {"rs1"} and all(members == 1 for _, _, _, members in got)
    if what.startswith("multiplicity"):
        assert len(got) == 1 and got[0][2] == (P - 1 if what.endswith("+ 1") else 1) and names[got[0][0]].startswith("dl")
    if what == "boundary value":
        assert (names.index("mem:write"), row, P - 1, 1) in got


def test_fraction_names_cover_the_chain_fractions():
    names = gen_circuit.fraction_names("trace")
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    assert len(names) == 4 * ref.n_chain(ref.parse(blob)) == 36 and names[0] == "rs1:read" and names[-1] == "table:and"
    assert "r0h_circuit_n_chain_fractions" in r0.EXPORTED_SYMBOLS and "r0h_logup_check_balance" in r0.EXPORTED_SYMBOLS
    image = np.fromfile(circuit_path("image"), dtype=np.uint32)
    assert gen_circuit.fraction_names("image") == ["fraction:%d" % f for f in range(4 * ref.n_chain(ref.parse(image)))]
    assert gen_circuit.fraction_names("tiny") == []


def test_the_host_function_refuses_bad_arguments():
    c, data, glob = bc.scenario("order", 4)
    with pytest.raises(r0.R0HipError, match="po2 3 outside"):
        host(c.words, 3, None, data, glob)
    with pytest.raises(r0.R0HipError, match=r"global\[0\] not canonical"):
        r0.logup_check_balance_host(c.words, 4, None, data, np.array([P, 0, 0, 0], dtype=np.uint32))
    lookups = lc.generate(7, tables=[1], n_chain=1, n_public=0)
    with pytest.raises(r0.R0HipError, match="CODE group"):
        host(lookups.words, 16, None, lookups.witness(16)[0], lookups.witness(16)[1])
    assert host(np.fromfile(circuit_path("tiny"), dtype=np.uint32), 9, None, np.zeros(12 << 9, dtype=np.uint32), None) == []   # no LOGUP section: nothing to check


def test_the_command_line_documents_the_switch_and_wants_its_value():
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    out = subprocess.run([prove, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--check-balance 1" in out.stdout and "--fraction-names" in out.stdout
    out = subprocess.run([prove, circuit_path("tiny"), "--check-balance"], capture_output=True, text=True)
    assert out.returncode == 1 and "--check-balance needs a value" in out.stderr
    out = subprocess.run([prove, circuit_path("tiny"), "--check-witness"], capture_output=True, text=True)
    assert out.returncode == 1 and "--check-witness needs a value" in out.stderr
