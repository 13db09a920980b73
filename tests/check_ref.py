"""Reference for r0h_check_witness: a numpy interpreter of a circuit blob's constraint program, written from the blob format
(include/r0hip_circuit.h) alone -- it shares nothing with the library's emitter.

Term t of a circuit is the t-th AndEqz of its PolyExtStep program once AndCond gates are flattened into their inner chains,
numbered by the power of poly_mix the verifier folds it with: walking a MixState chain from True, an AndEqz takes one power, an
AndCond as many as its inner chain holds (and multiplies every inner term by its condition).  On an N-row trace the value of a
term at row r is the AndEqz value times its gates, a tap (group, column, back) being the witness column at row (r - back) mod N
(tools/gen_circuit.py check_trace_rows: np.roll(src, back); the verifier evaluates back-taps at z w^-back, the same direction).
The witness satisfies the circuit iff every term vanishes on every row.

Words are the device's: Montgomery form (x 2^32 mod p) unless montgomery=False.  Zero is zero in both forms; the arithmetic here
is canonical.
"""
import numpy as np

P = 15 * 2**27 + 1
R_INV = pow(1 << 32, P - 2, P)
SEC_GROUPS, SEC_TAPS, SEC_GLOBALS, SEC_POLY = 1, 2, 3, 4
OP_CONST, OP_GET, OP_GET_GLOBAL, OP_ADD, OP_SUB, OP_MUL, OP_TRUE, OP_AND_EQZ, OP_AND_COND = 0, 2, 3, 4, 5, 6, 7, 8, 9
G_ACCUM, G_CODE, G_DATA = 0, 1, 2


class Program:
    def __init__(self, blob):
        w = [int(x) for x in np.asarray(blob, dtype=np.uint32)]
        assert w[0] == 0x31433052 and w[1] == 1
        at, sec = 3, {}
        for _ in range(w[2]):
            sec[w[at]] = w[at + 2:at + 2 + w[at + 1]]
            at += 2 + w[at + 1]
        self.group_size = sec[SEC_GROUPS][:3]
        t = sec[SEC_TAPS]
        self.taps = [tuple(t[1 + 3 * k:4 + 3 * k]) for k in range(t[0])]
        self.n_global, self.n_mix = sec[SEC_GLOBALS][:2]
        p = sec[SEC_POLY]
        self.ret = p[1]
        self.fp, self.mix = [], []  # variable -> (op, a, b, c); the two kinds are numbered separately in creation order
        for k in range(p[0]):
            st = tuple(p[2 + 4 * k:6 + 4 * k])
            (self.mix if st[0] in (OP_TRUE, OP_AND_EQZ, OP_AND_COND) else self.fp).append(st)
        self.terms = []  # term t = (value variable, [gate variables])
        self._flatten(self.ret, [])
        # which variables reach the ACCUM group or the accumulation mix: their terms have no value before the mix is drawn
        late = []
        for op, a, b, _ in self.fp:
            late.append(self.taps[a][0] == G_ACCUM if op == OP_GET else a == 1 if op == OP_GET_GLOBAL else
                        (late[a] or late[b]) if op in (OP_ADD, OP_SUB, OP_MUL) else False)
        self.late = [late[v] or any(late[g] for g in gates) for v, gates in self.terms]

    def _flatten(self, m, gates):
        chain = []
        while self.mix[m][0] != OP_TRUE:
            chain.append(m)
            m = self.mix[m][1]
        for m in reversed(chain):
            op, _, b, c = self.mix[m]
            if op == OP_AND_EQZ:
                self.terms.append((b, list(gates)))
            else:
                self._flatten(c, gates + [b])

    @property
    def n_and_eqz(self):
        return sum(1 for st in self.mix if st[0] == OP_AND_EQZ)


def _columns(words, count, n, montgomery):
    m = np.asarray(words).reshape(count, n).astype(np.uint64)
    return (m * np.uint64(R_INV)) % np.uint64(P) if montgomery else m % np.uint64(P)


def check(blob, po2, code, data, glob, accum=None, mix=None, montgomery=True):
    """-> {term: (rows that violate it, the first of them)} over the terms the witness violates.  code / data / accum: the groups'
    columns, [column][row] (flat or 2-D); glob / mix: the public inputs and the accumulation mix.  Without `accum` only the terms
    that reach neither an ACCUM tap nor a mix word are evaluated."""
    pr = Program(blob)
    n = 1 << po2
    groups = {G_CODE: _columns(code, pr.group_size[G_CODE], n, montgomery), G_DATA: _columns(data, pr.group_size[G_DATA], n, montgomery)}
    if accum is not None:
        groups[G_ACCUM] = _columns(accum, pr.group_size[G_ACCUM], n, montgomery)
    scal = lambda x: (int(x) * R_INV if montgomery else int(x)) % P
    gl = [scal(x) for x in glob][:pr.n_global]
    mx = [scal(x) for x in mix] if mix is not None else None
    wanted = [t for t in range(len(pr.terms)) if accum is not None or not pr.late[t]]
    # evaluate what those terms reach, freeing every variable after its last reader
    uses = [0] * len(pr.fp)
    need = set()
    stack = [v for t in wanted for v in [pr.terms[t][0]] + pr.terms[t][1]]
    for v in stack:
        uses[v] += 1
    while stack:
        v = stack.pop()
        if v in need:
            continue
        need.add(v)
        op, a, b, _ = pr.fp[v]
        if op in (OP_ADD, OP_SUB, OP_MUL):
            uses[a] += 1
            uses[b] += 1
            stack += [a, b]
    readers = {}  # variable -> terms that read it directly, evaluated as soon as all of their variables exist
    pending = {}
    for t in wanted:
        vs = set([pr.terms[t][0]] + pr.terms[t][1])
        pending[t] = len(vs)
        for v in vs:
            readers.setdefault(v, []).append(t)
    vals, out = {}, {}
    p64 = np.uint64(P)

    def release(v, k=1):
        uses[v] -= k
        if uses[v] == 0:
            del vals[v]

    for v, (op, a, b, _) in enumerate(pr.fp):
        if v not in need:
            continue
        if op == OP_CONST:
            r = np.full(n, a % P, dtype=np.uint64)
        elif op == OP_GET:
            g, col, back = pr.taps[a]
            r = np.roll(groups[g][col], back)
        elif op == OP_GET_GLOBAL:
            r = np.full(n, gl[b] if a == 0 else mx[b], dtype=np.uint64)
        else:
            x, y = vals[a], vals[b]
            r = (x + y) % p64 if op == OP_ADD else (x + p64 - y) % p64 if op == OP_SUB else (x * y) % p64
            release(a)
            release(b)
        vals[v] = r
        for t in readers.get(v, ()):
            pending[t] -= 1
            if pending[t]:
                continue
            tv, gates = pr.terms[t]
            w = vals[tv]
            for g in gates:
                w = (w * vals[g]) % p64
            bad = np.nonzero(w)[0]
            if len(bad):
                out[t] = (int(len(bad)), int(bad[0]))
            for u in [tv] + gates:
                release(u)
    return out


# trace-circuit columns a single wrong cell of which some constraint notices on any live row (tests/test_trace_circuit.py forges these)
TRACE_MUTATION_COLUMNS = ("pc", "next_pc", "cycle", "live", "mem_wr")


def mutations(blob, po2, seed, count, columns=None, rows=None):
    """Seeded single-cell mutations of a DATA group for the tests: [(column, row, new word)], rows 0 and N - 1 first (the wrap).
    Columns: `columns` if given; else the DERIVED columns of a synthetic circuit's column program (WITGEN kind 1 / 2) -- each is
    pinned on every row by its own constraint `column = product + term`, where a free or padding column may be read by nothing on
    most rows and a mutation of it would say nothing.  `rows` bounds the rows drawn (default: all N).  The new word is a random
    Montgomery word that differs from nothing in particular: a collision with the old one has probability 2^-31."""
    w = [int(x) for x in np.asarray(blob, dtype=np.uint32)]
    n = 1 << po2
    if columns is None:
        at = 3
        while w[at] != 5:  # WITGEN
            at += 2 + w[at + 1]
        q = at + 2 + 1 + 2 * w[at + 2]
        columns = [k for k in range(w[q]) if w[q + 1 + 5 * k] in (1, 2)]
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        row = 0 if k == 0 else n - 1 if k == 1 else int(rng.integers(0, rows or n))
        out.append((int(columns[int(rng.integers(0, len(columns)))]), row, int(rng.integers(1, P))))
    return out
