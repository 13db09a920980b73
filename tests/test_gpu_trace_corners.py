"""The device witness of the trace circuit (trace_witgen_kernel, csrc/trace.hip; the multiplicities: logup_count_kernel /
logup_mult_kernel, csrc/logup.hip) on the corner programs of trace_corners.py and at the edges of the segment shape: the largest
segment the API accepts, one without blank rows, one of a single cycle, and the segment numbers at the top of the accepted range.
The host witness compiles the same csrc/trace.hpp, so equality with it says nothing about the code hipcc emits for gfx950 on its
own: every device witness is also checked against the references that do not share that code -- the numpy restatement of the
columns that come straight from the rows, every constraint and fraction evaluated in Python, the exact-integer decode, and the
multiplicities counted in Python."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import trace_corners as tcr
from conftest import circuit_path
from trace_corners import COL, F, P, PRIMARY, canonical, canonical_globals, decode, expand
from gen_circuit import check_trace_rows
import trace_circuit as tc

pytestmark = pytest.mark.gpu
PO2 = r0.TRACE_MIN_PO2
MULT = [COL["m16"], COL["mand"]]


@pytest.fixture(scope="module")
def circ(hal, orc):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob)
    yield blob, gc, orc.circuit(blob)
    gc.free()


def host_multiplicities(words, glob, po2):
    """the multiplicity columns r0h_logup_multiplicities_host counts on these words (its own columns cleared first)"""
    blob = r0.trace_blob()
    d = words.copy().reshape(r0.TRACE_COLUMNS, -1)
    d[MULT] = 0
    d = d.reshape(-1)
    g = glob.copy()
    r0._check(r0.lib().r0h_logup_multiplicities_host(blob.ctypes.data_as(r0._vp), blob.size, po2, d.ctypes.data_as(r0._vp), g.ctypes.data_as(r0._vp)))
    return d.reshape(r0.TRACE_COLUMNS, -1)[MULT]


def device_checks(hal, gc, rows, bounds, po2, number=1, closing=True, host=None):
    """the device witness of these rows against everything that does not share its code; with `host` (the host witness and its
    globals) word for word against that too.  -> (device Buf, its globals, canonical witness)"""
    dev, dglob = hal.trace_witgen(rows, bounds, po2, number=number, closing=closing, circuit=gc)
    got = dev.to_host()
    if host is not None:
        assert np.array_equal(dglob, host[1])
        if not np.array_equal(got, host[0]):
            diff = np.nonzero((got != host[0]).reshape(r0.TRACE_COLUMNS, -1))
            raise AssertionError("device != host at (column, row) %s" % [(tcr.TRACE_COLUMNS[c], int(r)) for c, r in zip(*diff)][:12])
    m, g = canonical(got, po2), canonical_globals(dglob)
    primary = [COL[c] for c in PRIMARY]
    want = expand(rows, bounds, po2, number, closing)[primary]
    if not np.array_equal(m[primary], want):
        bad = [PRIMARY[i] for i in range(len(primary)) if not np.array_equal(m[primary[i]], want[i])]
        raise AssertionError("device columns unlike the numpy restatement: %s" % bad)
    assert check_trace_rows(m, g) == []
    assert decode(rows, m) == []
    assert np.array_equal(got.reshape(r0.TRACE_COLUMNS, -1)[MULT], host_multiplicities(got, dglob, po2))
    recount = m.copy()
    tc.multiplicities(recount, g)
    assert np.array_equal(recount[MULT], m[MULT])
    return dev, dglob, m


def seal_of(hal, orc, circ, po2, dev, glob, seed, oracle=None):
    """the device seal of this witness under a random challenge, checked by both verifiers; with `oracle` (the host words) the
    totals, the accumulation and the seal equal the oracle's.  -> the verifiers' verdict"""
    blob, gc, c = circ
    code, synthetic, _ = hal.witgen(gc, po2, 0)
    synthetic.free()
    rng = np.random.default_rng(seed)
    glob = glob.copy()
    glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = [orc.enc(int(v)) for v in rng.integers(0, P, 16)]
    full = hal.logup_totals(gc, po2, code, dev, glob)
    cc = hal.code_commit(gc, po2, code)
    try:
        if oracle is not None:
            ocode = c.witgen(po2, 0)[0]
            assert np.array_equal(full, c.logup_totals(po2, ocode, oracle, glob))
            mix = np.array([orc.enc(int(v)) for v in rng.integers(0, P, c.n_mix)], dtype=np.uint32)
            acc = hal.accum_public(gc, po2, code, dev, full, mix)
            assert np.array_equal(acc.to_host(), c.accum_public(po2, ocode, oracle, full, mix))
            acc.free()
        seal = hal.prove_segment(gc, po2, cc, dev, full)
        root = cc.root()
        verdict = c.verify(seal, code_root=root)
        assert r0.verify_seal(blob, seal, code_root=root)[:2] == verdict
        if oracle is not None and verdict[0] == 0:
            assert np.array_equal(seal, c.prove(po2, ocode, oracle, full))
        return verdict
    finally:
        cc.free()
        code.free()


@pytest.mark.parametrize("name", sorted(tcr.PROGRAMS))
def test_the_device_witness_of_a_corner_program(hal, orc, circ, name):
    expect = (0, 0x00050003) if name == "ecall" else (0, 0)
    vm = tcr.run(tcr.PROGRAMS[name](), expect=expect)
    assert len(vm.segments()) == 1
    rows, bounds = vm.preflight_arrays(0)
    data, glob = vm.trace_witness(0, PO2)
    dev, dglob, m = device_checks(hal, circ[1], rows, bounds, PO2, host=(data, glob))
    try:
        assert seal_of(hal, orc, circ, PO2, dev, dglob, seed=len(rows), oracle=data) == (0, "ok")
        if name != "mext":
            return
        # a result changed where nobody reads it, one per M family: the high word of a product off by one, the neighbouring
        # quotient / remainder pair of a division -- the memory argument still balances, the multiplier / divider objects
        rng = np.random.default_rng(7)
        for family in ("mulh", "div", "rem"):
            r, value = forged_row(rows, family, rng)
            lie = tcr.dead_lie(rows, bounds, r, value)
            hal.trace_witgen(lie[0], lie[1], PO2, into=dev, circuit=circ[1])
            assert seal_of(hal, orc, circ, PO2, dev, dglob, seed=r)[0] == 4, (family, r)
    finally:
        dev.free()


def forged_row(rows, family, rng):
    """a row of the family with signed corners among its operands and the lie it tells"""
    f3s = {"mulh": (1, 2, 3), "div": (4, 5), "rem": (6, 7)}[family]
    cands = []
    for r in range(len(rows) - 8):
        insn, a, b = (int(x) for x in rows[r, [F["insn"], F["rs1"], F["rs2"]]])
        f3 = (insn >> 12) & 7
        if (insn & 0xFE00007F) != 0x02000033 or f3 not in f3s or not rows[r, F["rd"]] or not (a >> 31 or b >> 31):
            continue
        if family != "mulh" and (b == 0 or (f3 in (4, 6) and a == 0x80000000 and b == 0xFFFFFFFF)):
            continue
        cands.append(r)
    r = int(rng.choice(cands))
    b, out = (int(x) for x in rows[r, [F["rs2"], F["rd_after"]]])
    if family == "mulh":
        return r, (out + 1) & tcr.M32
    if family == "div":  # quotient + 1 (its remainder would be remainder - divisor)
        return r, (out + 1) & tcr.M32
    return r, (out - b) & tcr.M32  # remainder - divisor (its quotient would be quotient + 1)


def test_the_device_witness_of_a_pause_and_of_the_tables_edges(hal, orc, circ):
    vm = tcr.run(tcr.ecall_program(pause=True, code=0xFFFF0001), expect=(r0.Vm.PAUSED, 0xFFFF0001))
    rows, bounds = vm.preflight_arrays(0)
    dev, dglob, _ = device_checks(hal, circ[1], rows, bounds, PO2, host=vm.trace_witness(0, PO2))
    dev.free()
    assert canonical_globals(dglob)[11:15] == [2, 1, 1, 0xFFFF]
    vm = tcr.run(tcr.lookup_program(tcr.LOOKUP_ITERATIONS))
    rows, bounds = vm.preflight_arrays(0)
    po2 = tcr.LOOKUP_PO2
    dev, dglob, m = device_checks(hal, circ[1], rows, bounds, po2, host=vm.trace_witness(0, po2))
    try:
        assert m[COL["m16"], 0] > 1 << 16 and m[COL["mand"], 0xFFFF] > 1 << 16 and min(m[COL["m16"], [1, 4095, 4096, 65535]]) >= tcr.LOOKUP_ITERATIONS
        assert seal_of(hal, orc, circ, po2, dev, dglob, seed=1) == (0, "ok")
    finally:
        dev.free()


def test_the_largest_segment(hal, orc, circ):
    """po2 = R0H_TRACE_MAX_PO2 with more than 2^20 cycles"""
    po2 = r0.TRACE_MAX_PO2
    vm = tcr.run(tcr.lookup_program(180_000), segment_po2=po2)
    assert len(vm.segments()) == 1
    rows, bounds = vm.preflight_arrays(0)
    assert len(rows) > 1 << 20
    dev, dglob, _ = device_checks(hal, circ[1], rows, bounds, po2, host=vm.trace_witness(0, po2))
    try:
        assert seal_of(hal, orc, circ, po2, dev, dglob, seed=21) == (0, "ok")
    finally:
        dev.free()


def test_a_segment_without_blank_rows_and_one_of_a_single_cycle(hal, orc, circ):
    pad = 8
    for _ in range(2):  # untouched image words after the program: each a closing boundary row and no cycle
        vm = tcr.run(tcr.lookup_program(10_000) + [0] * pad, segment_po2=PO2)
        n = len(vm.preflight(0)) + len(vm.boundary(0))
        pad += (1 << PO2) - n
    assert len(vm.segments()) == 1 and n == 1 << PO2 and pad >= 8
    for vm in (vm, tcr.run([tcr.ECALL])):  # a0 = a7 = 0: HALT(0) in the first cycle
        rows, bounds = vm.preflight_arrays(0)
        dev, dglob, _ = device_checks(hal, circ[1], rows, bounds, PO2, host=vm.trace_witness(0, PO2))
        try:
            assert seal_of(hal, orc, circ, PO2, dev, dglob, seed=len(rows)) == (0, "ok")
        finally:
            dev.free()
    assert len(rows) == 1


@pytest.mark.parametrize("number", [1, 2, 65535, 65536])
@pytest.mark.parametrize("closing", [False, True])
def test_segment_numbers_at_the_ends_of_the_range(hal, circ, number, closing):
    """the memory program's rows as segment `number`, its boundary rows naming segment 0 and number - 1 as the earlier holders:
    DL2 = number - prev_seg - 1 reaches 65535, the last entry of the range table"""
    vm = tcr.run(tcr.memory_program())
    rows, bounds = vm.preflight_arrays(0)
    bounds[:, 4] = np.where(np.arange(len(bounds)) % 2, number - 1, 0)
    dev, _, m = device_checks(hal, circ[1], rows, bounds, PO2, number=number, closing=closing)
    dev.free()
    assert m[COL["dl2"], len(rows):len(rows) + len(bounds)].max() == number - 1
    for bad in (0, 65537):
        with pytest.raises(r0.R0HipError, match="outside"):
            hal.trace_witgen(rows, bounds, PO2, number=bad)
