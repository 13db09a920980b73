"""Corner programs for the trace circuit's witness, and the references they are checked against (a helper module for
test_trace_corners.py, test_gpu_trace_corners.py and test_trace_circuit.py; no tests of its own).

The programs are built with test_rv32im's assembler and aim at the places a witness generator goes wrong: the M extension over a cross
product of operand corners (with the aliasing forms), every shift amount, wrap-around and sign edges of the ALU, narrow loads and stores
at every byte lane, the lowest and highest guest words, every branch both ways at signed and unsigned boundaries, jumps back and
forth, every ecall, and lookups of the range table's and the AND table's edge values counted more than 2^16 times.

The references are written from the RISC-V specification and include/r0hip.h, independently of csrc/trace.hpp: `expand` restates the
columns that come straight from the compact rows with numpy; `decode` reads back, with Python integers, what the work words of each
row say the instruction computed."""
import os
import sys

import numpy as np

import hyperfridge_r0_amd as r0
from test_rv32im import A0, A1, A7, ECALL, ADDI, B, I, J, LI, R, S, U, flat

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from gen_circuit import OPCODES, TRACE_COLUMNS  # noqa: E402

COL = {name: i for i, name in enumerate(TRACE_COLUMNS)}
P = 2013265921
R_INV = pow(1 << 32, P - 2, P)
M32 = 0xFFFFFFFF
F = dict(cycle=0, pc=1, insn=2, next_pc=3, rs1=4, rs2=5, rd=6, rd_before=7, rd_after=8, mem_kind=9, mem_addr=10, mem_before=11, mem_after=12, prev=13)
STAMP = {0: 2, 1: 3, 2: 4, 3: 5, 4: 1}  # access (x[rs1], x[rs2], x[rd], memory, fetch) -> its place in the cycle

PRIMARY = (["live", "bnd", "cycle", "pc", "next_pc"] + ["opc_" + n for n, _ in OPCODES[:-1]] + ["f3_%d" % k for k in range(1, 8)]
           + ["rd0", "rdA", "rdB", "r10", "r1A", "r1B", "r20", "r2A", "r2B", "b25", "f7A", "f7B", "b30", "b31"]
           + ["rs1_lo", "rs1_hi", "dl0", "dh0", "rs2_lo", "rs2_hi", "dl1", "dh1", "zrd", "inv_rd", "act2", "old_lo", "old_hi", "dl2", "dh2"]
           + ["mem_wr", "top", "addr3", "before_lo", "before_hi", "after_lo", "after_hi", "p3", "dl4", "dh4", "fimg"])


def expand(rows, bounds, po2, number=1, closing=True):
    """The columns of the DATA group that come straight from the compact rows (PRIMARY), as canonical integers, [column, row]: the
    specification of include/r0hip.h (r0h_preflight_row, r0h_preflight_bound, the trace-circuit paragraph) written out with numpy.
    (Access 3's timestamp limbs are left out: rows that multiply keep a carry there.)"""
    n, nr, nb = 1 << po2, len(rows), len(bounds)
    m = np.zeros((len(TRACE_COLUMNS), n), dtype=np.int64)
    inv = lambda v: pow(int(v) % P, P - 2, P)
    r = rows.astype(np.int64)
    L = slice(0, nr)
    insn, cyc = r[:, F["insn"]], r[:, F["cycle"]]
    m[COL["live"], L] = 1
    m[COL["cycle"], L] = cyc
    m[COL["pc"], L] = r[:, F["pc"]]
    m[COL["next_pc"], L] = r[:, F["next_pc"]]
    for name, code in OPCODES[:-1]:  # (FENCE, the last of the list, has no column: it is `live` minus the others)
        m[COL["opc_" + name], L] = (insn & 0x7F) == code
    for k in range(1, 8):            # (funct3 = 0 likewise: one minus the others)
        m[COL["f3_%d" % k], L] = ((insn >> 12) & 7) == k
    for stem, shift in (("rd", 7), ("r1", 15), ("r2", 20)):
        idx = (insn >> shift) & 31
        m[COL[stem + "0"] if stem != "rd" else COL["rd0"], L] = idx & 1
        m[COL[stem + "A"], L] = (idx >> 1) & 3
        m[COL[stem + "B"], L] = idx >> 3
    m[COL["b25"], L], m[COL["f7A"], L], m[COL["f7B"], L], m[COL["b30"], L], m[COL["b31"], L] = (insn >> 25) & 1, (insn >> 26) & 3, (insn >> 28) & 3, (insn >> 30) & 1, insn >> 31
    small = np.array([0] + [inv(i) for i in range(1, 32)], dtype=np.int64)
    for k, (lo, hi, dl, dh, val) in enumerate((("rs1_lo", "rs1_hi", "dl0", "dh0", "rs1"), ("rs2_lo", "rs2_hi", "dl1", "dh1", "rs2"))):
        m[COL[lo], L] = r[:, F[val]] & 0xFFFF          # every cycle reads two registers, x0 included
        m[COL[hi], L] = r[:, F[val]] >> 16
        diff = 5 * cyc + STAMP[k] - r[:, F["prev"] + k] - 1
        assert (diff >= 0).all() and (diff < 1 << 24).all()
        m[COL[dl], L], m[COL[dh], L] = diff & 0xFFFF, diff >> 16
    m[COL["zrd"]] = 1
    m[COL["zrd"], L] = ((insn >> 7) & 31) == 0
    m[COL["inv_rd"], L] = small[(insn >> 7) & 31]
    wr = r[:, F["rd"]] != 0
    m[COL["act2"], L] = wr
    m[COL["old_lo"], L] = np.where(wr, r[:, F["rd_before"]] & 0xFFFF, 0)
    m[COL["old_hi"], L] = np.where(wr, r[:, F["rd_before"]] >> 16, 0)
    diff = np.where(wr, 5 * cyc + STAMP[2] - r[:, F["prev"] + 2] - 1, 0)
    m[COL["dl2"], L], m[COL["dh2"], L] = diff & 0xFFFF, diff >> 16
    mem = r[:, F["mem_kind"]] != 0
    m[COL["mem_wr"], L] = r[:, F["mem_kind"]] == r0.MEM_WRITE
    m[COL["addr3"], L] = np.where(mem, r[:, F["mem_addr"]] >> 2, 0)
    for name, f in (("before", "mem_before"), ("after", "mem_after")):
        m[COL[name + "_lo"], L] = np.where(mem, r[:, F[f]] & 0xFFFF, 0)
        m[COL[name + "_hi"], L] = np.where(mem, r[:, F[f]] >> 16, 0)
    m[COL["p3"], L] = np.where(mem, r[:, F["prev"] + 3], 0)
    diff = 5 * cyc + STAMP[4] - r[:, F["prev"] + 4] - 1
    m[COL["dl4"], L], m[COL["dh4"], L] = diff & 0xFFFF, diff >> 16
    if nb:
        bb = bounds.astype(np.int64)
        B_ = slice(nr, nr + nb)
        m[COL["bnd"], B_] = 1
        m[COL["addr3"], B_] = bb[:, 0]
        m[COL["after_lo"], B_], m[COL["after_hi"], B_] = bb[:, 1] & 0xFFFF, bb[:, 1] >> 16     # written: the value found, timestamp 0
        m[COL["before_lo"], B_], m[COL["before_hi"], B_] = bb[:, 2] & 0xFFFF, bb[:, 2] >> 16   # read: the value left, at its last timestamp
        m[COL["p3"], B_] = bb[:, 3]
        assert (bb[:, 0] < (1 << 28) + 32).all()
        top = bb[:, 0] >> 28                                                                   # the address: two limbs and the register bit
        low = bb[:, 0] - (top << 28)
        m[COL["top"], B_] = top
        m[COL["dl0"], B_], m[COL["dl1"], B_] = low & 0xFFFF, low >> 16
        m[COL["dh0"], B_] = np.where(top == 1, 8 * (low & 0xFFFF), 0)
        m[COL["dl2"], B_] = number - bb[:, 4] - 1                                              # the segment that held the address before: an earlier one
        if closing:
            m[COL["old_lo"], B_], m[COL["old_hi"], B_] = bb[:, 5] & 0xFFFF, bb[:, 5] >> 16     # the address's initial value
            m[COL["fimg"], B_] = bb[:, 6] & 1
    return m


def montgomery(m):
    return ((m.astype(object) << 32) % P).astype(np.uint32)


def canonical(words, po2):
    """witness words (Montgomery form, column-major) -> [column, row] canonical integers"""
    return (words.reshape(len(TRACE_COLUMNS), 1 << po2).astype(np.int64) * R_INV) % P


def canonical_globals(glob):
    return [int(x) * R_INV % P for x in glob]


# ---- the exact-integer decode: what the work words of each row say, against what the instruction defines
def _s32(v):
    return v - (1 << 32) if v >> 31 else v


def _div(p, q):  # rounds toward zero
    return abs(p) // abs(q) * (1 if (p < 0) == (q < 0) else -1)


def decode(rows, m):
    """Checks every live row of canonical witness m [column, row] against rows [n, 18] (the compact rows) with Python integers.
    -> a list of (row, what, got, want) for every disagreement (empty: the witness says what the instructions compute).
    Products and shifts: Z + 2^32 W is the 64-bit two's-complement product of the row's variant (a shift is a product by a power
    of two: 2^s to the left, 2^(32 - s) to the right, whose high word W is the result).  Divisions: U is the quotient, Z the
    remainder (the specification's table for a zero divisor and -2^31 / -1), W = |divisor| - |remainder| - 1 for a non-zero
    divisor.  Narrow loads: the result is the lane, sign- or zero-extended.  Every row that writes a register: the result columns
    are what the register receives."""
    col = lambda name: [int(x) for x in m[COL[name], :len(rows)]]
    zq, zhi, ob0, ob1, wlo, whi = col("zq"), col("z_hi"), col("ob0"), col("ob1"), col("w_lo"), col("w_hi")
    u = [col("u%d" % i) for i in range(4)]
    rlo, rhi = col("res_lo"), col("res_hi")
    bad = []
    for r, w in enumerate(rows.tolist()):
        insn, a, b = w[F["insn"]], w[F["rs1"]], w[F["rs2"]]
        op, f3, f7 = insn & 0x7F, (insn >> 12) & 7, insn >> 25
        Z = ob0[r] + 2 * ob1[r] + 4 * zq[r] + (zhi[r] << 16)
        W = wlo[r] + (whi[r] << 16)
        res = rlo[r] + (rhi[r] << 16)
        if w[F["rd"]] and res != w[F["rd_after"]]:
            bad.append((r, "res", res, w[F["rd_after"]]))
        want = None
        if op == 0x33 and f7 == 1 and f3 < 4:
            x = _s32(a) if f3 in (1, 2) else a
            y = _s32(b) if f3 == 1 else b
            want = (x * y) & ((1 << 64) - 1)
            res_want = want & M32 if f3 == 0 else want >> 32
        elif (op == 0x33 and f7 in (0, 0x20) or op == 0x13) and f3 in (1, 5):
            s = (b if op == 0x33 else insn >> 20) & 31
            if f3 == 1:
                want, res_want = a << s, (a << s) & M32
            else:
                x = _s32(a) if (insn >> 30) & 1 else a
                want = (x << (32 - s)) & ((1 << 64) - 1)
                res_want = (x >> s) & M32
        if want is not None:
            if Z + (W << 32) != want:
                bad.append((r, "Z + 2^32 W", Z + (W << 32), want))
            if res != res_want:
                bad.append((r, "result", res, res_want))
            continue
        if op == 0x33 and f7 == 1:  # division
            signed = f3 in (4, 6)
            x, y = (_s32(a), _s32(b)) if signed else (a, b)
            if y == 0:
                q, rem = -1, x
            elif signed and x == -2**31 and y == -1:
                q, rem = x, 0
            else:
                q = _div(x, y)
                rem = x - q * y
            Q = sum(u[i][r] << (8 * i) for i in range(4))
            if Q != q & M32:
                bad.append((r, "quotient", Q, q & M32))
            if Z != rem & M32:
                bad.append((r, "remainder", Z, rem & M32))
            if y != 0 and W != abs(y) - abs(rem) - 1:
                bad.append((r, "|b| - |rem| - 1", W, abs(y) - abs(rem) - 1))
            if res != (q if f3 in (4, 5) else rem) & M32:
                bad.append((r, "result", res, (q if f3 in (4, 5) else rem) & M32))
        elif op == 0x03:
            lane, word = (a + (insn >> 20) - ((insn >> 31) << 12)) & 3, w[F["mem_before"]]  # the effective address's lane (mem_addr is the word's)
            byte, half = (word >> (8 * lane)) & 0xFF, (word >> (8 * lane)) & 0xFFFF
            lw = {0: byte - ((byte & 0x80) << 1), 1: half - ((half & 0x8000) << 1), 2: word, 4: byte, 5: half}[f3] & M32
            if res != lw:
                bad.append((r, "load", res, lw))
    return bad


# ---- the programs
BASE = 0x1000
HALT0 = flat(ADDI(A0, 0, 0), ADDI(A7, 0, 0), ECALL)
CORNERS = [0, 1, 2, 3, 0x7F, 0x80, 0xFF, 0x100, 0x7FFF, 0x8000, 0xFFFF, 0x10000, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF,
           0xFFFF0000, 0x12345678, 0xEDCBA988]
INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF


def mext_program():
    """every ordered pair of CORNERS and five seeded random words through all eight M instructions (x1..x25 hold the operands, the
    results go to x26..x31 in turn, so that every result is overwritten unread), then the aliasing forms on a subset of pairs"""
    rng = np.random.default_rng(36)
    vals = CORNERS + [int(v) for v in rng.integers(0, 1 << 32, 5, dtype=np.uint64)]
    body = flat(*[LI(1 + i, v) for i, v in enumerate(vals)])
    k = 0
    for i in range(len(vals)):
        for j in range(len(vals)):
            for f3 in range(8):
                body.append(R(1, 1 + j, 1 + i, f3, 26 + k % 6))
                k += 1
    for a, b in [(INT_MIN, M32), (M32, M32), (INT_MIN, INT_MIN), (INT_MAX, M32), (0x12345678, 0), (7, 0xFFFFFFF9), (0xFFFF, 0x10000), (3, 2)]:
        for f3 in range(8):
            body += flat(LI(26, a), LI(27, b), R(1, 27, 26, f3, 26),        # rd = rs1
                         LI(26, a), R(1, 27, 26, f3, 27),                   # rd = rs2
                         R(1, 26, 26, f3, 28),                              # rs1 = rs2
                         R(1, 27, 26, f3, 0))                               # rd = x0
    return flat(body, HALT0)


def alu_program():
    """shifts by every amount (immediate, register, register with the high bits set), ADD / SUB wrapping, comparisons at the sign
    edges, the logic immediates at the 12-bit sign edge, LUI / AUIPC with bit 31"""
    body = flat(LI(1, 1), LI(2, 0x12345678), LI(3, 0x80000000), LI(4, 0xFFFFFFFF))
    for s in range(32):
        body += flat(ADDI(5, 0, s), LI(6, 0xFFFFFFE0 | s))
        for x in (1, 2, 3, 4):
            body += [I(s, x, 1, 7, 0x13), I(s, x, 5, 8, 0x13), I(0x400 | s, x, 5, 9, 0x13),     # SLLI SRLI SRAI
                     R(0, 5, x, 1, 10), R(0, 5, x, 5, 11), R(0x20, 5, x, 5, 12),                # SLL SRL SRA
                     R(0, 6, x, 1, 13), R(0, 6, x, 5, 14), R(0x20, 6, x, 5, 15)]                # ... by 0xFFFFFFE0 | s
    pairs = [(INT_MIN, INT_MAX), (INT_MAX, INT_MIN), (M32, 0), (0, M32), (INT_MAX, 1), (INT_MIN, 1), (M32, 1), (0, 1), (5, 5), (INT_MIN, INT_MIN)]
    for a, b in pairs:
        body += flat(LI(16, a), LI(17, b), R(0, 17, 16, 0, 18), R(0x20, 17, 16, 0, 19),            # ADD SUB
                     R(0, 17, 16, 2, 20), R(0, 17, 16, 3, 21))                                       # SLT SLTU
        for imm in (0, 1, 0x7FF, 0x800, 0xFFF):                                                      # (0xFFF: -1)
            body += [I(imm, 16, 0, 22, 0x13), I(imm, 16, 2, 23, 0x13), I(imm, 16, 3, 24, 0x13),      # ADDI SLTI SLTIU
                     I(imm, 16, 4, 25, 0x13), I(imm, 16, 6, 26, 0x13), I(imm, 16, 7, 27, 0x13)]      # XORI ORI ANDI
    body += [U(0x80000, 28, 0x37), U(0xFFFFF, 29, 0x37), U(0x80000, 30, 0x17), U(0xFFFFF, 31, 0x17), U(0x7FFFF, 28, 0x17), U(0x80001, 0, 0x37)]
    return flat(body, HALT0)


DATA = 0x40000
LOW, HIGH = 0, (1 << 30) - 4  # the lowest and the highest guest word


def memory_program():
    """narrow and full loads at every lane over the bytes 0x00 / 0x7F / 0x80 / 0xFF, stores at every lane, the lowest and the highest
    guest word, and a store over the instruction's own word"""
    words = [0xFF807F00, 0x00FF807F, 0x7F00FF80, 0x807F00FF]  # every byte value at every lane
    body = flat(LI(1, DATA))
    for k, v in enumerate(words):
        body += flat(LI(2, v), S(4 * k, 2, 1, 2))
    for k in range(len(words)):
        for lane in range(4):
            body += [I(4 * k + lane, 1, 0, 3, 0x03), I(4 * k + lane, 1, 4, 4, 0x03)]              # LB LBU
        for lane in (0, 2):
            body += [I(4 * k + lane, 1, 1, 5, 0x03), I(4 * k + lane, 1, 5, 6, 0x03)]              # LH LHU
        body += [I(4 * k, 1, 2, 7, 0x03)]                                                         # LW
    body += flat(LI(8, 0xA5C3F18E))
    for lane in range(4):
        body += [S(0x40 + lane, 8, 1, 0), I(0x40, 1, 2, 9, 0x03)]                                 # SB, then the word read back
    for lane in (0, 2):
        body += [S(0x50 + lane, 8, 1, 1), I(0x50, 1, 2, 9, 0x03)]                                 # SH
    body += [S(0x60, 8, 1, 2), I(0x60, 1, 2, 9, 0x03)]                                            # SW
    body += flat(LI(10, HIGH), S(0, 8, 0, 2), I(0, 0, 2, 11, 0x03),                               # the lowest word: stored, read back
                 I(0, 10, 2, 12, 0x03), S(0, 8, 10, 2), I(0, 10, 0, 13, 0x03))                    # the highest: read, stored, read
    body += flat(U(0, 14, 0x17),                                                                  # auipc x14, 0
                 I(4, 14, 2, 15, 0x03),                                                           # lw x15, 4(x14): this very word
                 ADDI(16, 0, 0x13),                                                               # x16 = the word of `addi x0, x0, 0`
                 U(0, 14, 0x17),                                                                  # auipc x14, 0
                 S(4, 16, 14, 2))                                                                 # sw x16, 4(x14): over itself
    return flat(body, HALT0)


def control_program():
    """every branch kind taken and not taken at signed and unsigned boundaries, JAL and JALR forward and back, JALR to an odd
    target, links into x0.  x31 counts the instructions a wrong turn would execute: it must stay zero."""
    body = []
    for a, b in [(INT_MIN, INT_MAX), (INT_MAX, INT_MIN), (M32, 0), (0, M32), (5, 5), (INT_MIN, INT_MIN), (0, 0)]:
        body += flat(LI(1, a), LI(2, b))
        for f3 in (0, 1, 4, 5, 6, 7):
            # taken: skips the marker; not taken: falls into it and the taken branch after it skips the next marker
            body += [B(8, 2, 1, f3), ADDI(30, 30, 1), B(8, 0, 0, 0), ADDI(31, 31, 1)]
    body += [J(8, 1),            # k0: jal x1, k2
             J(12, 0),           # k1: jal x0, k4 (forward)
             J(-4, 0),           # k2: jal x0, k1 (back)
             ADDI(31, 31, 1)]    # k3: never
    body += [U(0, 5, 0x17),         # k0: auipc x5, 0
             I(13, 5, 0, 6, 0x67),  # k1: jalr x6, 13(x5): forward to k0 + 12 (bit 0 dropped)
             ADDI(31, 31, 1),       # k2: never
             U(0, 5, 0x17),         # k3: auipc x5, 0
             J(8, 0),               # k4: jal x0, k6
             J(12, 0),              # k5: jal x0, k8
             I(9, 5, 0, 0, 0x67),   # k6: jalr x0, 9(x5): back to k5 (k3 + 8, bit 0 dropped), link into x0
             ADDI(31, 31, 1)]       # k7: never
    return flat(body, ADDI(A0, 31, 0), ADDI(A7, 0, 0), ECALL)  # HALT(x31): 0 unless a wrong turn was taken


IO_BUF = 0x50000
N_INPUT = 40


def ecall_program(pause=False, code=0x00050003):
    """READ_WORDS with n = 0, 1 and many; COMMIT with n = 0 and many; CYCLES; then HALT (or PAUSE) with `code`"""
    J0 = r0.JOURNAL_BASE
    body = flat(LI(A0, IO_BUF), ADDI(A1, 0, 0), ADDI(A7, 0, 1), ECALL,          # READ_WORDS n = 0
                LI(A0, IO_BUF), ADDI(A1, 0, 1), ADDI(A7, 0, 1), ECALL,          # n = 1
                LI(A0, J0), ADDI(A1, 0, N_INPUT - 1), ADDI(A7, 0, 1), ECALL,    # n = many, into the journal window
                LI(A0, J0), ADDI(A1, 0, 0), ADDI(A7, 0, 2), ECALL,              # COMMIT n = 0
                LI(A0, J0), ADDI(A1, 0, N_INPUT - 1), ADDI(A7, 0, 2), ECALL,    # n = many
                ADDI(A7, 0, 3), ECALL, ADDI(9, A0, 0),                          # CYCLES
                LI(A0, code), ADDI(A7, 0, 4 if pause else 0), ECALL)
    return body


def lookup_program(iterations):
    """rows that look up the range table's edges (0, 1, 4095, 4096, 65535: halves of sums) and the AND table's (0xFF, 0xFF) many times
    each -- zero and (0xFF, 0xFF) more than 2^16 times at 2^17 rows: the LDS bins below 4096 and the global counters above"""
    return flat(LI(1, 0xFFFFFFFF), LI(2, 0x0FFF0004), LI(3, 0x10004000), LI(4, iterations),
                R(0, 0, 1, 0, 5),         # add x5, x1, x0: Z's high half 65535
                R(0, 0, 2, 0, 6),         # add x6, x2, x0: 4095, and 1 above Z's two low bits
                R(0, 0, 3, 0, 7),         # add x7, x3, x0: 4096, 4096
                R(0, 1, 1, 7, 8),         # and x8, x1, x1: (0xFF, 0xFF) four times
                ADDI(4, 4, -1), B(-20, 0, 4, 1), HALT0)


LOOKUP_ITERATIONS, LOOKUP_PO2 = 16500, 17  # four (0xFF, 0xFF) lookups per iteration: more than 2^16 in all

PROGRAMS = {"mext": mext_program, "alu": alu_program, "memory": memory_program, "control": control_program, "ecall": ecall_program}


def run(prog, segment_po2=20, inputs=None, expect=(0, 0)):
    vm = r0.Vm()
    vm.load(BASE, prog)
    vm.set_pc(BASE)
    vm.set_input(list(range(1, N_INPUT + 1)) if inputs is None else inputs)
    assert vm.run(segment_po2=segment_po2, keep_trace=True, boundary_rows=True) == expect
    return vm


def dead_lie(rows, bounds, r, value):
    """(rows, bounds) with row r claiming it wrote `value` into its register, a register nobody reads before its next write (or
    before the boundary row that leaves it) -- memory stays consistent, only the instruction's own unit can object"""
    reg = int(rows[r, F["rd"]])
    assert reg and rows[r, F["insn"]] != 0x73
    reads = lambda w: (17, 10) if w[F["insn"]] == 0x73 else ((int(w[F["insn"]]) >> 15) & 31, (int(w[F["insn"]]) >> 20) & 31)
    nxt = next((q for q in range(r + 1, len(rows)) if reg in reads(rows[q]) or rows[q, F["rd"]] == reg), None)
    assert nxt is None or reg not in reads(rows[nxt]), "the register is read"
    bad_rows, bad_bounds = rows.copy(), bounds.copy()
    bad_rows[r, F["rd_after"]] = value
    if nxt is not None:
        bad_rows[nxt, F["rd_before"]] = value
    else:
        bad_bounds[int(np.nonzero(bounds[:, 0] == r0.REG_BASE + reg)[0][0]), 2] = value
    return bad_rows, bad_bounds
