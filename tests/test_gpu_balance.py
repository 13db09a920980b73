"""r0h_logup_check_balance on the device against the host function and the numpy restatement (tests/balance_ref.py): every case asserts
device == host == reference.  Tuple circuits (tests/balance_circuits.py) at fewer rows than a workgroup, one workgroup's and several,
through every path of the insert kernel; generated lookup circuits with and without their multiplicities; the trace circuit's device
witness with three single-word alterations; the sequencer's switch; the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_circuit  # noqa: E402
import trace_corners as tcr  # noqa: E402
from trace_corners import COL, P  # noqa: E402

import balance_circuits as bc  # noqa: E402
import balance_ref as br  # noqa: E402
import logup_circuits as lc  # noqa: E402
import logup_ref as ref  # noqa: E402
from test_balance import ALTERATIONS, trace_alteration  # noqa: E402

pytestmark = pytest.mark.gpu
PO2 = r0.TRACE_MIN_PO2
N = 1 << PO2


def three_ways(hal, gc, po2, code, data, glob, capacity=None):
    """device, host and reference on one witness (code: a Buf or None; data: host words) -> the reference's full list"""
    code_words = code.to_host() if code is not None else None
    want = br.check(gc.blob, po2, code_words, data, glob)
    assert r0.logup_check_balance_host(gc.blob, po2, code_words, data, glob) == want
    buf = hal.copy_from(data)
    try:
        assert hal.logup_check_balance(gc, po2, code, buf, glob) == want
        if capacity is not None:
            assert hal.logup_check_balance(gc, po2, code, buf, glob, capacity=capacity) == (want[:capacity], len(want))
            assert r0.logup_check_balance_host(gc.blob, po2, code_words, data, glob, capacity=capacity) == (want[:capacity], len(want))
    finally:
        buf.free()
    return want


@pytest.mark.parametrize("po2", [4, 8, 12])
def test_a_permutation_balances_and_one_altered_cell_does_not(hal, po2):
    c, data, glob = bc.scenario("permutation", po2)
    gc = hal.load_circuit(c.words)
    assert gc.n_chain_fractions == 4
    assert three_ways(hal, gc, po2, None, data, glob) == []
    n = 1 << po2
    for column, row in ((2, n // 2), (0, 0), (3, n - 1)):
        bad = data.copy()
        bad[column * n + row] = ref.enc((int(ref.dec(bad[column * n + row])) + 1) % P)
        want = three_ways(hal, gc, po2, None, bad, glob, capacity=1)
        assert len(want) == 2 and sorted(net for _, _, net, _ in want) == [1, P - 1] and all(members == 1 for _, _, _, members in want)
        assert row in [r for _, r, _, _ in want]
    gc.free()


@pytest.mark.parametrize("name", ["order", "zero part", "weights", "minus ones", "hot", "surplus", "many identities"])
def test_kernel_paths_on_tuple_circuits(hal, name):
    po2 = 12
    c, data, glob = bc.scenario(name, po2)
    gc = hal.load_circuit(c.words)
    want = three_ways(hal, gc, po2, None, data, glob, capacity=1)
    assert (want == []) == (name in bc.BALANCED)
    if name == "surplus":
        assert want == [(0, 0, 1, 2 * (1 << po2) + 1)]
    if name == "order":  # and a class that does NOT close is told from its neighbours through either path
        bad = data.copy()
        bad[4 << po2] = ref.enc((int(ref.dec(bad[4 << po2])) + 1) % P)   # one half of a split coordinate, row 0
        assert len(three_ways(hal, gc, po2, None, bad, glob)) == 2
    if name == "many identities":  # eleven challenge identities; one consumed value of the second pair altered
        want = three_ways(hal, gc, po2, None, bc.altered(data, po2, 6, 1 << (po2 - 1)), glob, capacity=1)
        assert len(want) == 2 and sorted(net for _, _, net, _ in want) == [1, P - 1]
    gc.free()


def test_every_tuple_in_a_class_of_its_own(hal):
    """32 K classes: more than a workgroup's LDS table holds, and more than the caller has room for"""
    po2 = 12
    c, data, glob = bc.scenario("own class", po2)
    gc = hal.load_circuit(c.words)
    want = three_ways(hal, gc, po2, None, data, glob, capacity=8)
    assert len(want) == 8 << po2 and want[:8] == [(f, 0, 1, 1) for f in range(8)]
    tuples, sent, slots = hal.logup_check_balance_stats()
    assert tuples == 8 << po2 == sent and slots == 16 << po2   # nothing to merge; a load of 1/2
    gc.free()


def test_the_hot_class_is_merged_in_lds(hal):
    po2 = 12
    c, data, glob = bc.scenario("hot", po2)
    gc = hal.load_circuit(c.words)
    buf = hal.copy_from(data)
    assert hal.logup_check_balance(gc, po2, None, buf, glob) == []
    tuples, sent, slots = hal.logup_check_balance_stats()
    assert tuples == 2 << po2 and 1 <= sent <= (1 << po2) // 1024 and slots == 4 << po2   # one flush a workgroup
    buf.free()
    gc.free()


@pytest.mark.parametrize("tables", [[1], [1, 2]])
@pytest.mark.parametrize("seed", [7, 11])
def test_generated_lookup_circuits_with_and_without_multiplicities(hal, seed, tables):
    c = lc.generate(seed, tables=tables, n_chain=3, n_public=1)
    gc = hal.load_circuit(c.words)
    code, unused, _ = hal.witgen(gc, 16, 0)
    unused.free()
    data, glob, _ = c.witness(16, seed=seed)
    assert three_ways(hal, gc, 16, code, ref.multiplicities(c.words, data, glob, 16), glob) == []
    want = three_ways(hal, gc, 16, code, data, glob, capacity=5)    # multiplicities left zero: every looked-up value's class
    assert len(want) > 5 and all(net == members for _, _, net, members in want)
    code.free()
    gc.free()


@pytest.fixture(scope="module")
def trace(hal):
    """the trace circuit and the device witness of a corner program at 2^16 rows, multiplicities filled"""
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    vm = tcr.run(tcr.PROGRAMS["alu"]())
    rows, bounds = vm.preflight_arrays(0)
    data, glob = hal.trace_witgen(rows, bounds, PO2, circuit=gc)
    code, unused, _ = hal.witgen(gc, PO2, 0)
    unused.free()
    yield gc, code, data, glob, len(rows)
    gc.free()


def trace_three_ways(hal, gc, code, data, glob):
    words, code_words = data.to_host(), code.to_host()
    want = br.check(gc.blob, PO2, code_words, words, glob)
    assert r0.logup_check_balance_host(gc.blob, PO2, code_words, words, glob) == want
    assert hal.logup_check_balance(gc, PO2, code, data, glob) == want
    return want


def test_an_honest_trace_witness_balances(hal, trace):
    gc, code, data, glob, _ = trace
    assert gc.n_chain_fractions == 36 == len(gen_circuit.fraction_names("trace"))
    assert trace_three_ways(hal, gc, code, data, glob) == []


@pytest.mark.parametrize("what", ALTERATIONS)
def test_an_altered_trace_witness_names_its_fractions(hal, trace, what):
    gc, code, data, glob, n_rows = trace
    column, row, value = trace_alteration(what, tcr.canonical(data.to_host(), PO2).astype(np.int64), n_rows)
    at = COL[column] * N + row
    old = data.to_host(at, 1)
    data.upload(ref.enc([value]), at)
    try:
        want = trace_three_ways(hal, gc, code, data, glob)
        names = gen_circuit.fraction_names("trace")
        print(what, [(names[f], r, net, members) for f, r, net, members in want])
        assert want and len(want) <= 4
    finally:
        data.upload(old, at)


def test_the_sequencers_switch(hal, trace):
    gc, code, data, glob, n_rows = trace
    glob = glob.copy()
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = np.random.default_rng(4).integers(0, P, 16).astype(np.uint32)
    full = hal.logup_totals(gc, PO2, code, data, glob)
    cc = hal.code_commit(gc, PO2, code)
    column, row, value = trace_alteration("multiplicity + 1", tcr.canonical(data.to_host(), PO2).astype(np.int64), n_rows)
    at = COL[column] * N + row
    old = data.to_host(at, 1)
    try:
        seal = hal.prove_segment(gc, PO2, cc, data, full)   # off by default: nothing is checked
        assert "check_balance" not in [n for n, _ in hal.last_profile()]
        hal.set_check_balance(True)
        assert np.array_equal(hal.prove_segment(gc, PO2, cc, data, full), seal)   # on, honest: the same seal, word for word
        assert "check_balance" in [n for n, _ in hal.last_profile()]
        assert np.array_equal(hal.prove_segment(gc, PO2, code, data, full), seal)  # ... and from the CODE columns themselves
        data.upload(ref.enc([value]), at)
        want = br.check(gc.blob, PO2, code.to_host(), data.to_host(), full)
        f, r, net, members = want[0]
        message = "prove_segment: fraction %d does not balance: net %d over %d tuples, first at row %d; %d classes in all" % (f, net, members, r, len(want))
        for how in (cc, code):
            with pytest.raises(r0.R0HipError) as e:
                hal.prove_segment(gc, PO2, how, data, full)
            assert str(e.value) == message
        with pytest.raises(r0.R0HipError) as e:
            hal.proof_begin(gc, PO2, cc, data, full)      # what sessions go through (r0h_proof_begin_committed)
        assert str(e.value) == message
        # the witness checker's switch alone: its message for the same witness, exactly as the checker states it
        hal.set_check_balance(False)
        hal.set_check_witness(True)
        h, _ = hal.proof_begin(gc, PO2, cc, data, full)
        mix = np.zeros(gc.n_mix, dtype=np.uint32)
        r0._check(r0.lib().r0h_proof_late(h, full[r0.TRACE_GLOBALS - r0.TRACE_LATE_GLOBALS:].ctypes.data_as(r0._vp), mix.ctypes.data_as(r0._vp)))
        accum = hal.accum_public(gc, PO2, code, data, full, mix)
        table = hal.check_witness(gc, PO2, code, data, full, accum, mix)
        assert table
        with pytest.raises(r0.R0HipError) as e:
            hal.proof_finish(h, accum)
        assert str(e.value) == "prove_segment: the witness violates %d of the circuit's %d constraint terms: term %d does not vanish on %d of 2^%d rows, first at row %d" % (
            len(table), gc.n_terms, table[0][0], table[0][1], PO2, table[0][2])
        accum.free()
    finally:
        hal.set_check_balance(False)
        hal.set_check_witness(False)
        data.upload(old, at)
        cc.free()


def test_argument_errors(hal):
    c, data, glob = bc.scenario("order", 4)
    gc = hal.load_circuit(c.words)
    buf = hal.copy_from(data)
    for po2 in (3, 25):
        with pytest.raises(r0.R0HipError, match="r0h_logup_check_balance: po2 %d outside" % po2):
            hal.logup_check_balance(gc, po2, None, buf, glob)
    with pytest.raises(r0.R0HipError, match="buffers too small"):
        hal.logup_check_balance(gc, 5, None, buf, glob)
    with pytest.raises(r0.R0HipError, match=r"global\[0\] not canonical"):
        hal.logup_check_balance(gc, 4, None, buf, np.array([P, 0, 0, 0], dtype=np.uint32))
    assert hal.logup_check_balance(gc, 4, None, buf, glob) == []   # the context goes on working
    buf.free()
    gc.free()
    tiny = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
    code, data, glob = hal.witgen(tiny, 9, 1)
    assert tiny.n_chain_fractions == 0 and hal.logup_check_balance(tiny, 9, code, data, glob) == []   # no LOGUP section: nothing to check
    tiny.free()


def test_cli_round_trip():
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    runs = []
    for extra in ([], ["--check-balance", "1"]):
        out = subprocess.run([prove, circuit_path("tiny"), "--po2", "9", "--seed", "3", "--verify", "1"] + extra, capture_output=True, text=True)
        assert out.returncode == 0 and "seals verified" in out.stderr, out.stdout + out.stderr
        runs.append(json.loads(out.stdout.splitlines()[0])["seal_fnv1a"])
    assert runs[0] == runs[1]
