"""The corner programs of trace_corners.py on the host: each runs to its end, and the host witness of every segment satisfies every
constraint and fraction of the trace circuit, carries the multiplicities the Python generator counts, equals the numpy restatement
in the columns that come straight from the compact rows, and says -- read back with Python integers -- what every instruction
computes (products, shifts, quotients and remainders, narrow loads, results).  The device gets the same programs in
test_gpu_trace_corners.py."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import trace_corners as tcr
from trace_corners import COL, F, PRIMARY, canonical, canonical_globals, decode, expand
from gen_circuit import check_trace_rows
import trace_circuit as tc

PO2 = r0.TRACE_MIN_PO2


def host_checks(vm, k, po2):
    """what the host witness of segment k must satisfy; -> (canonical witness, canonical globals, compact rows, bounds)"""
    rows, bounds = vm.preflight_arrays(k)
    data, glob = vm.trace_witness(k, po2)
    m, g = canonical(data, po2), canonical_globals(glob)
    assert check_trace_rows(m, g) == []
    recount = m.copy()
    tc.multiplicities(recount, g)
    assert np.array_equal(recount[[COL["m16"], COL["mand"]]], m[[COL["m16"], COL["mand"]]])
    primary = [COL[c] for c in PRIMARY]
    assert np.array_equal(m[primary], expand(rows, bounds, po2)[primary])
    assert decode(rows, m) == []
    return m, g, rows, bounds


@pytest.mark.parametrize("name", sorted(tcr.PROGRAMS))
def test_a_corner_program_has_a_witness_that_says_what_it_computes(name):
    expect = (0, 0x00050003) if name == "ecall" else (0, 0)
    vm = tcr.run(tcr.PROGRAMS[name](), expect=expect)
    assert len(vm.segments()) == 1
    m, g, rows, bounds = host_checks(vm, 0, PO2)
    ops = [(int(w[F["insn"]]) & 0x7F, (int(w[F["insn"]]) >> 12) & 7, int(w[F["insn"]]) >> 25) for w in rows]
    if name == "mext":
        for f3 in range(8):
            assert sum(o == (0x33, f3, 1) for o in ops) >= 25 * 25 + 8 * 4
    elif name == "alu":
        for kind in [(0x13, 1, 0), (0x13, 5, 0), (0x13, 5, 0x20), (0x33, 1, 0), (0x33, 5, 0), (0x33, 5, 0x20)]:
            assert sum(o == kind for o in ops) == (2 if kind[0] == 0x33 else 1) * 32 * 4
    elif name == "memory":
        addrs = [int(b) for b in bounds[:, 0]]
        hi = addrs.index((tcr.HIGH >> 2))
        assert addrs[0] == 0 and addrs[hi + 1] == r0.REG_BASE  # the largest gap: the highest guest word, then the registers
        lanes = {(o[1], (int(w[F["rs1"]]) + (int(w[F["insn"]]) >> 20)) & 3) for o, w in zip(ops, rows) if o[0] == 0x03}
        assert lanes >= {(f3, l) for f3 in (0, 4) for l in range(4)} | {(f3, l) for f3 in (1, 5) for l in (0, 2)} | {(2, 0)}
    elif name == "control":
        taken = {(o[1], int(w[F["next_pc"]]) != int(w[F["pc"]]) + 4) for o, w in zip(ops, rows) if o[0] == 0x63 and w[F["insn"]] & 0x1F00000 != 0}
        assert taken == {(f3, t) for f3 in (0, 1, 4, 5, 6, 7) for t in (False, True)}
        assert any(o[0] == 0x67 and int(w[F["next_pc"]]) < int(w[F["pc"]]) for o, w in zip(ops, rows))       # a jump back through JALR
        assert any(o[0] == 0x6F and int(w[F["next_pc"]]) < int(w[F["pc"]]) for o, w in zip(ops, rows))
    elif name == "ecall":
        sysrows = [w for w in rows if w[F["insn"]] == 0x73]
        assert [int(w[F["rs1"]]) for w in sysrows] == [1] + [1] * 2 + [1] * tcr.N_INPUT + [2] + [2] * tcr.N_INPUT + [3, 0]  # (a transfer of n words: n + 1 rows)
        assert g[11:15] == [1, 1, 3, 5]  # HALT, non-zero, the exit code's halves


def test_a_pause_ends_the_segment_with_its_exit_code():
    vm = tcr.run(tcr.ecall_program(pause=True, code=0xFFFF0001), expect=(r0.Vm.PAUSED, 0xFFFF0001))
    m, g, rows, _ = host_checks(vm, 0, PO2)
    assert g[11:15] == [2, 1, 1, 0xFFFF] and g[8:11] == [tcr.BASE, int(rows[-1, F["next_pc"]]), len(rows)]


def test_lookups_of_the_tables_edges_are_counted():
    """value 0 (by subtraction) and the AND table's (0xFF, 0xFF) counted more than 2^16 times, 1 / 4095 below the LDS bins' edge,
    4096 / 65535 above it"""
    vm = tcr.run(tcr.lookup_program(tcr.LOOKUP_ITERATIONS))
    m, _, _, _ = host_checks(vm, 0, tcr.LOOKUP_PO2)
    m16, mand = m[COL["m16"]], m[COL["mand"]]
    assert m16[0] > 1 << 16 and mand[0xFFFF] > 1 << 16
    assert min(m16[[1, 4095, 4096, 65535]]) >= tcr.LOOKUP_ITERATIONS


def test_the_decode_objects_to_a_wrong_product_quotient_and_remainder():
    """the decode is a reference, not an echo: a wrong word of each kind is named"""
    vm = tcr.run(tcr.mext_program())
    rows, _ = vm.preflight_arrays(0)
    m = canonical(vm.trace_witness(0, PO2)[0], PO2)
    kind = lambda r: (int(rows[r, F["insn"]]) >> 12) & 7 if (int(rows[r, F["insn"]]) & 0xFE00007F) == 0x02000033 else None
    mulh = next(r for r in range(len(rows)) if kind(r) == 1 and rows[r, F["rs1"]] >> 31 and rows[r, F["rs2"]] >> 31)
    div = next(r for r in range(len(rows)) if kind(r) == 4 and rows[r, F["rs2"]] not in (0, 0xFFFFFFFF) and rows[r, F["rs1"]] >> 31)
    for col, r, what in (("w_hi", mulh, "Z + 2^32 W"), ("u1", div, "quotient"), ("z_hi", div, "remainder")):
        bad = m.copy()
        bad[COL[col], r] ^= 1
        assert what in [x[1] for x in decode(rows, bad) if x[0] == r], (col, r)
