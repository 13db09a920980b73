"""What a trace-circuit witness CLAIMS: the inverse of trace_corners.expand() (a helper module for test_trace_forgeries.py and
test_gpu_trace_forgeries.py; no tests of its own).

`claims(m, n_rows, n_bounds)` reads a canonical witness [column, row] back into the execution it asserts, in plain Python integers:
per live row the cycle, the pc and the next pc, the instruction word, both register values read, the register written (index, old
value, value written) and the memory word touched (word address, value before, value after, written or read); per boundary row the
address, the first and the last value, the last timestamp, the previous segment, the initial value and the image flag.  Which fields
a row carries is decided by the instruction word (and, for an ecall, by the values of a7 and a1 it read) and the ISA alone, written
here from the RISC-V specification and include/r0hip.h -- no flag of the circuit's own (act2, zrd, alu, mem_act, ...) is consulted.
Timestamp limbs, carries, inverses, byte decompositions and the multiplicity columns are auxiliary: they are no part of the claim.

A forged cell either changes the claim -- then a constraint or a fraction has to object -- or it does not, and then it is the
prover's own business.  That is the criterion the forgery sweep judges single cells by; `verdict` states it."""
import numpy as np

import hyperfridge_r0_amd as r0
from trace_corners import COL, F, P

OPCODE_OF = dict(lui=0x37, auipc=0x17, jal=0x6F, jalr=0x67, branch=0x63, load=0x03, store=0x23, imm=0x13, op=0x33, system=0x73, fence=0x0F)
WRITES_RD = (0x37, 0x17, 0x6F, 0x67, 0x03, 0x13, 0x33)
A0, A1 = 10, 11


def _word(v, lo, hi):
    return int(v[lo]) + (int(v[hi]) << 16)


def insn_of(v):
    """the 32-bit instruction word of a row (v: column name -> canonical integer), reassembled from the one-hot opcode and funct3, the
    register digits and the funct7 bits"""
    named = [n for n in OPCODE_OF if n != "fence"]
    fence = int(v["live"]) - sum(int(v["opc_" + n]) for n in named)
    opcode = sum(OPCODE_OF[n] * int(v["opc_" + n]) for n in named) + OPCODE_OF["fence"] * fence
    f3 = sum(k * int(v["f3_%d" % k]) for k in range(1, 8))
    reg = lambda s: int(v[s + "0"]) + 2 * int(v[s + "A"]) + 8 * int(v[s + "B"])
    f7 = int(v["b25"]) + 2 * int(v["f7A"]) + 8 * int(v["f7B"]) + 32 * int(v["b30"]) + 64 * int(v["b31"])
    return opcode + (reg("rd") << 7) + (f3 << 12) + (reg("r1") << 15) + (reg("r2") << 20) + (f7 << 25)


LIVE_COLUMNS = (["live", "bnd", "cycle", "pc", "next_pc"] + ["opc_" + n for n in OPCODE_OF if n != "fence"] + ["f3_%d" % k for k in range(1, 8)]
                + ["rd0", "rdA", "rdB", "r10", "r1A", "r1B", "r20", "r2A", "r2B", "b25", "f7A", "f7B", "b30", "b31", "rs1_lo", "rs1_hi", "rs2_lo", "rs2_hi",
                   "old_lo", "old_hi", "res_lo", "res_hi", "addr3", "before_lo", "before_hi", "after_lo", "after_hi"])
BOUND_COLUMNS = ["live", "bnd", "addr3", "after_lo", "after_hi", "before_lo", "before_hi", "p3", "dl2", "old_lo", "old_hi", "fimg"]


def live_claim(m, r):
    v = {c: int(m[COL[c], r]) for c in LIVE_COLUMNS}
    insn = insn_of(v)
    out = dict(live=v["live"], bnd=v["bnd"], cycle=v["cycle"], pc=v["pc"], next_pc=v["next_pc"], insn=insn,
               rs1=_word(v, "rs1_lo", "rs1_hi"), rs2=_word(v, "rs2_lo", "rs2_hi"))
    op, rd = insn & 0x7F, (insn >> 7) & 31
    old = _word(v, "old_lo", "old_hi")
    mem = None
    if op == 0x73:   # an ecall reads a7 (the function) and a0; READ_WORDS / COMMIT count a1 down and move a word while it is not zero
        fn = out["rs1"]
        rd = A1 if fn in (1, 2) else A0 if fn == 3 else 0
        if fn in (1, 2) and old != 0:
            mem = fn == 1
    elif op not in WRITES_RD:
        rd = 0
    if op in (0x03, 0x23):
        mem = op == 0x23
    if rd:
        out["rd"] = (rd, old, _word(v, "res_lo", "res_hi"))
    if mem is not None:
        out["mem"] = (v["addr3"], _word(v, "before_lo", "before_hi"), _word(v, "after_lo", "after_hi"), mem)
    return out


def bound_claim(m, r, number=1):
    v = {c: int(m[COL[c], r]) for c in BOUND_COLUMNS}
    return dict(live=v["live"], bnd=v["bnd"], addr=v["addr3"], first=_word(v, "after_lo", "after_hi"), last=_word(v, "before_lo", "before_hi"),
                last_ts=v["p3"], prev_seg=(number - 1 - v["dl2"]) % P, init=_word(v, "old_lo", "old_hi"), image=v["fimg"])


def claims(m, n_rows, n_bounds, only=None, number=1):
    """-> {"rows": {row: claim}, "bounds": {row: claim}, "blank": rows past the boundary rows that are flagged live or boundary}.
    `only`: the rows to read (a claim of a row is a function of that row's cells alone); default all of them."""
    n = m.shape[1]
    rows = range(n) if only is None else only
    out = {"rows": {r: live_claim(m, r) for r in rows if r < n_rows},
           "bounds": {r: bound_claim(m, r, number) for r in rows if n_rows <= r < n_rows + n_bounds}}
    rest = np.asarray([r for r in rows if r >= n_rows + n_bounds], dtype=np.int64)
    flagged = rest[(m[COL["live"], rest] != 0) | (m[COL["bnd"], rest] != 0)] if len(rest) else rest
    out["blank"] = [int(r) for r in flagged]
    return out


def executed(rows, bounds):
    """the same structure from the executor's compact rows [n, 18] and bounds [n, 7] (include/r0hip.h: r0h_preflight_row,
    r0h_preflight_bound): what an honest witness must claim"""
    out = {"rows": {}, "bounds": {}, "blank": []}
    for r, w in enumerate(rows.tolist()):
        c = dict(live=1, bnd=0, cycle=w[F["cycle"]], pc=w[F["pc"]], next_pc=w[F["next_pc"]], insn=w[F["insn"]], rs1=w[F["rs1"]], rs2=w[F["rs2"]])
        if w[F["rd"]]:
            c["rd"] = (w[F["rd"]], w[F["rd_before"]], w[F["rd_after"]])
        if w[F["mem_kind"]]:
            c["mem"] = (w[F["mem_addr"]] >> 2, w[F["mem_before"]], w[F["mem_after"]], w[F["mem_kind"]] == r0.MEM_WRITE)
        out["rows"][r] = c
    for j, b in enumerate(bounds.tolist()):
        out["bounds"][len(rows) + j] = dict(live=0, bnd=1, addr=b[0], first=b[1], last=b[2], last_ts=b[3], prev_seg=b[4], init=b[5], image=b[6] & 1)
    return out


def verdict(caught, before, after):
    """the criterion: 'caught' if a checker objected, else 'harmless' if the claim is what it was, else 'HOLE'"""
    return "caught" if caught else "harmless" if before == after else "HOLE"
