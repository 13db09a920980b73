"""The forgery plan of the trace circuit's single-cell sweep (a helper module for test_trace_forgeries.py and
test_gpu_trace_forgeries.py; no tests of its own): which cells of the honest witnesses of trace_corners.PROGRAMS are edited, and to
what.  Everything here is deterministic.

Rows, per program: one live row per instruction kind (opcode, funct3, funct7 class -- the classes of
test_trace_circuit.test_what_an_instruction_computes_is_constrained_kind_by_kind; an ecall's third entry is 2 x its function number a7
plus whether it moves a word), each kind used once across the programs, at a row that writes a register other than x0 where the kind
writes one; a second row for the kind where one with rd = x0 exists; row 0, the last live row, the first, a middle and the last
boundary row, the first blank row and row N - 1.  Columns: every DATA column but the two multiplicity columns (the forger recounts
them), and the public inputs 8..19 once each.  Values per cell: old + 1, old - 1 mod p, a value that leaves the cell's table (256 for
a byte, 65536 for a 16-bit half, 4 for a radix-4 digit, 2 for a bit) and one seeded random word -- without duplicates and never `old`.

What the sweep can and cannot find: a single-cell edit finds a cell NOTHING constrains (or a lookup nobody makes).  It does not find
a consistent lie told in several cells at once -- the value written changed with every later sight of it: trace_corners.dead_lie and
the kind-by-kind test of test_trace_circuit.py keep that job."""
import numpy as np

import hyperfridge_r0_amd as r0
import trace_corners as tcr
from trace_corners import COL, F, P

PO2 = r0.TRACE_MIN_PO2
N = 1 << PO2
ORDER = ("mext", "alu", "memory", "control", "ecall")          # the order in which the programs are given their kinds
assert sorted(ORDER) == sorted(tcr.PROGRAMS)
COLUMNS = [c for c in tcr.TRACE_COLUMNS if c not in ("m16", "mand")]
GLOBALS = list(range(8, 20))
WRITES_RD = (0x37, 0x17, 0x6F, 0x67, 0x03, 0x13, 0x33)

BITS = set(["live", "bnd", "alu", "rd0", "r10", "r20", "b25", "b30", "b31", "zrd", "act2", "mem_wr", "top", "su", "sv", "vrb", "ob0", "ob1", "c0", "c1", "lt",
            "eq", "sgn", "sx", "sm", "dv", "ovf", "a31", "f0", "f1", "f2", "fn_cyc", "cact", "fimg"]
           + [c for c in COLUMNS if c.startswith(("opc_", "f3_"))] + ["sh%d" % k for k in range(5)])
DIGITS = {"rdA", "rdB", "r1A", "r1B", "r2A", "r2B", "f7A", "f7B", "vrd", "ce0", "ce1a", "ce1b", "ce2"}
BYTES = set(["u%d" % k for k in range(4)] + ["v%d" % k for k in range(1, 4)] + ["a%d" % k for k in range(4)] + ["mb%d" % k for k in range(4)]
            + ["dh%d" % k for k in range(5)] + ["sb", "cb1", "cb2", "cband"])
HALVES = set(["dl%d" % k for k in range(5)] + ["rs1_lo", "rs1_hi", "rs2_lo", "rs2_hi", "old_lo", "old_hi", "before_lo", "before_hi", "after_lo", "after_hi",
              "res_lo", "res_hi", "z_hi", "zq", "w_lo", "w_hi", "aux0", "aux1"])
OUTSIDE = {**{c: 2 for c in BITS}, **{c: 4 for c in DIGITS}, **{c: 256 for c in BYTES}, **{c: 65536 for c in HALVES}}
assert not (BITS & DIGITS or BITS & BYTES or BITS & HALVES or DIGITS & BYTES or BYTES & HALVES) and set(OUTSIDE) <= set(COLUMNS)
VALUE_KINDS = ("+1", "outside", "random", "-1")                 # in the order of preference in which a sweep short of time keeps them


def kind_of(w):
    """the instruction kind of a compact row (a list or an array row)"""
    insn = int(w[F["insn"]])
    op, f3, f7 = insn & 0x7F, (insn >> 12) & 7, insn >> 25
    if op == 0x73:
        fn = int(w[F["rs1"]])
        return (op, 0, 2 * fn + int(w[F["mem_kind"]] != 0))
    return (op, f3, f7 if op == 0x33 else (f7 & 0x20) if (op == 0x13 and f3 == 5) else 0)


class Honest:
    """a corner program's run: compact rows, boundary rows, the host reference's witness as canonical integers and its public inputs"""

    def __init__(self, prog):
        self.prog = prog
        self.words = tcr.PROGRAMS[prog]()
        self.vm = tcr.run(self.words, expect=(0, 0x00050003) if prog == "ecall" else (0, 0))
        self.rows, self.bounds = self.vm.preflight_arrays(0)
        self.n_rows, self.n_bounds = len(self.rows), len(self.bounds)
        self.data, self.glob = self.vm.trace_witness(0, PO2)
        self.m = tcr.canonical(self.data, PO2)
        self.g = tcr.canonical_globals(self.glob)
        self.journal = bytes(self.vm.journal)

    def verifier_side(self):
        """what the verifier of the one-segment closing session adds to the session sum: [(numerator, vector)] per image word and
        journal word (the vectors of r0h_session_balance_add_tuples: 1, -address, -low half, -high half, -tag)"""
        import struct
        import trace_circuit as tc
        image = [((tcr.BASE >> 2) + i, w, tc.TAG_IMG) for i, w in enumerate(self.words)]
        journal = [(r0.JOURNAL_BASE // 4 + i, w, tc.TAG_JRN) for i, w in enumerate(struct.unpack("<%dI" % (len(self.journal) // 4), self.journal))]
        return [(P - 1, [1, (-a) % P, (-(w & 0xFFFF)) % P, (-(w >> 16)) % P, (-t) % P]) for a, w, t in image + journal]


_HONEST = {}


def honest(prog):
    if prog not in _HONEST:
        _HONEST[prog] = Honest(prog)
    return _HONEST[prog]


def kind_rows():
    """-> {program: [(row, kind, "kind" | "kind, rd = x0")]}: every kind once, in the first program of ORDER that executes it, at a
    seeded choice among its rows there"""
    rng = np.random.default_rng(26)
    seen, out = set(), {}
    for prog in ORDER:
        h = honest(prog)
        by_kind = {}
        for r, w in enumerate(h.rows.tolist()):
            if 0 < r < h.n_rows - 1:                            # (row 0 and the last live row are sites of their own)
                by_kind.setdefault(kind_of(w), []).append(r)
        out[prog] = []
        for kind in sorted(by_kind):
            if kind in seen:
                continue
            seen.add(kind)
            cand = by_kind[kind]
            rd = lambda r: (int(h.rows[r, F["insn"]]) >> 7) & 31
            if kind[0] in WRITES_RD:
                writing, x0 = [r for r in cand if rd(r)], [r for r in cand if not rd(r)]
                if writing:
                    out[prog].append((writing[int(rng.integers(0, len(writing)))], kind, "kind"))
                if x0:
                    out[prog].append((x0[int(rng.integers(0, len(x0)))], kind, "kind, rd = x0"))
            else:
                out[prog].append((cand[int(rng.integers(0, len(cand)))], kind, "kind"))
    return out


_KIND_ROWS = []


def site_rows(prog):
    """-> [(row, what)] of the program's sites, in row order, every row once (a row that is two things keeps its first name)"""
    if not _KIND_ROWS:
        _KIND_ROWS.append(kind_rows())
    h = honest(prog)
    nr, nb = h.n_rows, h.n_bounds
    special = [(0, "row 0"), (nr - 1, "last live row"), (nr, "first boundary row"), (nr + nb // 2, "middle boundary row"), (nr + nb - 1, "last boundary row"),
               (nr + nb, "first blank row"), (N - 1, "row N - 1")]
    rows = {}
    for r, what in special + [(r, "%s %s" % (w, "%#x/%d/%#x" % k)) for r, k, w in _KIND_ROWS[0][prog]]:
        rows.setdefault(r, what)
    return sorted(rows.items())


def values(col, old, rng):
    """-> [(value kind, canonical value)] for a cell holding `old`, in VALUE_KINDS order"""
    out, seen = [], {old}
    for kind, v in (("+1", (old + 1) % P), ("outside", OUTSIDE.get(col)), ("random", int(rng.integers(0, P))), ("-1", (old - 1) % P)):
        if v is not None and v not in seen:
            seen.add(v)
            out.append((kind, v))
    return out


def plan(prog, columns=None, kinds=VALUE_KINDS):
    """-> [(column name, row, what the row is, value kind, old, new)]: the program's DATA edits, column by column"""
    h = honest(prog)
    out = []
    for col in (COLUMNS if columns is None else columns):
        rng = np.random.default_rng([26, ORDER.index(prog), COL[col]])
        for row, what in site_rows(prog):
            old = int(h.m[COL[col], row])
            out += [(col, row, what, k, old, v) for k, v in values(col, old, rng) if k in kinds]
    return out


def global_plan(prog):
    """-> [(public input, old, new)]: each of the public inputs 8..19 once"""
    h = honest(prog)
    return [(k, h.g[k], (h.g[k] + 1) % P) for k in GLOBALS]


BLOCKS = [COLUMNS[i:i + 32] for i in range(0, len(COLUMNS), 32)]


# ---- the row-local judge: what a single edit breaks, without walking 2^16 rows
def _early_terms(pr, data, code, gl):
    """{term: mask over the columns of `data`} of the circuit's early terms (check_ref's evaluation, on any number of columns)"""
    import check_ref as cr
    groups = {cr.G_CODE: code.astype(np.uint64), cr.G_DATA: data.astype(np.uint64)}
    p64, width = np.uint64(P), data.shape[1]
    early = [t for t in range(len(pr.terms)) if not pr.late[t]]
    need, stack = set(), [v for t in early for v in [pr.terms[t][0]] + pr.terms[t][1]]
    while stack:
        v = stack.pop()
        if v not in need:
            need.add(v)
            op, a, b, _ = pr.fp[v]
            if op in (cr.OP_ADD, cr.OP_SUB, cr.OP_MUL):
                stack += [a, b]
    vals = {}
    for v, (op, a, b, _) in enumerate(pr.fp):
        if v not in need:
            continue
        if op == cr.OP_CONST:
            vals[v] = np.full(width, a % P, dtype=np.uint64)
        elif op == cr.OP_GET:
            g, col, back = pr.taps[a]
            vals[v] = np.roll(groups[g][col], back)
        elif op == cr.OP_GET_GLOBAL:
            vals[v] = np.full(width, gl[b], dtype=np.uint64)
        else:
            x, y = vals[a], vals[b]
            vals[v] = (x + y) % p64 if op == cr.OP_ADD else (x + p64 - y) % p64 if op == cr.OP_SUB else (x * y) % p64
    out = {}
    for t in early:
        w = vals[pr.terms[t][0]]
        for g in pr.terms[t][1]:
            w = (w * vals[g]) % p64
        out[t] = w != 0
    return out


def _row_tuples(fractions, data, code, gl):
    """per column of `data`: {denominator parts: [net numerator, fraction names]} of the fractions that are no lookups, and the names of
    the lookups whose value is not in its table"""
    import trace_circuit as tc
    width = data.shape[1]
    tuples, outside = [dict() for _ in range(width)], [set() for _ in range(width)]
    for f in fractions:
        if f.name.startswith("table:"):
            continue
        num = f.num.evaluate(data, code, gl)
        parts = [lf.evaluate(data, code, gl) for _, lf in f.parts[1:]]
        if f.table:
            value = (-parts[0]) % P
            idx = value - tc.TAG_AND
            ok = ((idx >= 0) & (idx < (1 << 24)) & (((idx & 255) & ((idx >> 8) & 255)) == (idx >> 16))) if f.table == tc.TABLE_AND else (value < 65536)
            for i in np.nonzero(~ok & (num != 0))[0]:
                outside[i].add(f.name)
            continue
        for i in np.nonzero(num)[0]:
            entry = tuples[i].setdefault(tuple(int(p[i]) for p in parts), [0, []])
            entry[0] = (entry[0] + int(num[i])) % P
            entry[1].append(f.name)
    return tuples, outside


def local_judge(prog, edits, chunk=1500):
    """What each single edit of `edits` (plan entries) breaks, judged on the edited row and its two neighbours alone -> per edit
    (names of the early terms that do not vanish, names of the fractions that do not cancel or look outside their table).

    A constraint reads a row and the row before it, so an edit at row r can only show on rows r and r + 1; a fraction reads its own
    row, so with the multiplicities recounted the argument balances iff the edited row makes the tuples the honest row made (the
    honest witness balances) and every value looked up is in its table.  Restated from check_ref's term numbering and
    tools/trace_circuit.fractions: it shares nothing with the library, and nothing with check_trace_rows but the circuit."""
    import check_ref as cr
    import gen_circuit
    import trace_circuit as tc
    from conftest import circuit_path
    h = honest(prog)
    pr = cr.Program(np.fromfile(circuit_path("trace"), dtype=np.uint32))
    names = gen_circuit.term_names("trace")
    code = np.array(tc.code_columns(N), dtype=np.int64)
    chained, session = tc.fractions()
    out = []
    for at in range(0, len(edits), chunk):
        part = edits[at:at + chunk]
        idx = np.array([[(e[1] - 1) % N, e[1], (e[1] + 1) % N] for e in part]).reshape(-1)
        was, local_code = h.m[:, idx], code[:, idx]
        now = was.copy()
        for k, e in enumerate(part):
            now[COL[e[0]], 3 * k + 1] = e[5]
        broken = [set() for _ in part]
        for t, mask in _early_terms(pr, now, local_code, h.g).items():
            for i in np.nonzero(mask)[0]:
                if i % 3:                   # (the first row of a triple has a stranger before it)
                    broken[i // 3].add(names[t])
        new_t, new_out = _row_tuples(chained + session, now, local_code, h.g)
        old_t, _ = _row_tuples(chained + session, was, local_code, h.g)
        for k in range(len(part)):
            i, open_ = 3 * k + 1, set(new_out[3 * k + 1])
            for key in set(new_t[i]) | set(old_t[i]):
                a, b = new_t[i].get(key, [0, []]), old_t[i].get(key, [0, []])
                if (a[0] - b[0]) % P:
                    open_ |= set(a[1] + b[1])
            out.append((broken[k], open_))
    return out
