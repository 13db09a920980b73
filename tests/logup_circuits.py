"""Generated circuits whose only argument is a log-derivative one (blob section LOGUP), with their witnesses -- a helper module for
test_logup.py and test_gpu_logup.py; no tests of its own.

`generate(seed)` varies what the committed circuits hold fixed (trace.r0c: tables R16 then AND, every numerator 1, every lookup in a
chain link; image.r0c: no tables): no table, R16 alone or R16 and AND; 1-6 chain links and 0-3 accumulators with a public total; 1-8
parts per denominator under all three challenge kinds; forms with public-input coefficients and constants; lookups whose numerator is
1 or a DATA selector (gated), whose value combines several columns.  Fractions that are not lookups come in pairs that cancel on every
row, so a witness whose multiplicities are right closes the chain.  The constraints are tools/trace_circuit.accum_constraints, so
seals of these circuits prove and verify like the committed ones.

Witnesses are numpy: looked-up values are drawn from the tables' edges (4096 is where logup_count_kernel stops binning in LDS), gated-off
rows hold values outside the table, every other column and the public inputs come from the corners of [0, p)."""
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_circuit as gc  # noqa: E402
from trace_circuit import G_ACCUM, G_CODE, G_DATA, LF, ONE, SEC_LOGUP, Fraction, accum_constraints  # noqa: E402

import logup_ref as ref  # noqa: E402

P = ref.P
EXTREME = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**31 - 2**27, 0x0FFFFFFF, 0x70000000]  # test_gpu_parity._extreme
VALUES = [0, 1, 2, 4095, 4096, 4097, 65534, 65535]
BYTES = [0, 1, 127, 128, 255]
N_COEF_GLOBALS = 4               # public inputs 0..3 are coefficients of forms; then the challenges; then the public totals
N_CH_GLOBALS = 2                 # challenges of four public inputs each
CODE_FIRST, CODE_LAST, CODE_RANDOM = 0, 1, 2
N_SEL = 4                        # selector columns: all 0, all 1, two random bit columns


class Circuit:
    """the blob (`words`), and what the witness generator needs to know about its columns"""

    def __init__(self, seed, tables=None, n_chain=None, n_public=None, lean=False):
        rng = random.Random(seed)
        self.seed, self.lean = seed, lean   # lean: forms of one term, denominators of one or two parts (for the largest sizes)
        self.kinds = tables if tables is not None else rng.choice([[], [1], [1, 2]])
        self.n_chain = n_chain if n_chain is not None else rng.randint(1, 6)
        self.n_public = n_public if n_public is not None else rng.randint(0, 3)
        self.n_mix = 4 * (len(self.kinds) + 2)
        self.n_global = N_COEF_GLOBALS + 4 * N_CH_GLOBALS + 4 * self.n_public
        self.code_cols = [(0, 0), (1, 0), (3, 7)]
        self.table_code = {}
        for k in self.kinds:
            self.table_code[k] = len(self.code_cols)
            self.code_cols.append((3 + k, 0))          # CODE kind 4 the range table, kind 5 the byte-AND table
        self.n_data = 0
        self.mult = {k: self._col() for k in self.kinds}
        self.sel = [self._col() for _ in range(N_SEL)]
        self.free = [self._col() for _ in range(4)]     # extreme values
        self.lookups = []                               # (kind, num selector or None / ("not", s), pivot col, its coef, the rest of the form, and cols)
        self.rng = rng
        slots = 4 * self.n_chain - len(self.kinds)
        n_look = rng.randint(1, max(1, slots - 1)) if self.kinds else 0
        chain = [self._table_fraction(k) for k in self.kinds]
        chain += [self._lookup(rng.choice(self.kinds)) for _ in range(min(n_look, slots))]
        rest = 4 * self.n_chain - len(chain)
        while rest >= 2:
            num, parts = self._form(rng, codes=True), self._den(rng, (0, 1, 2))
            chain += [Fraction("pair", num, parts), Fraction("pair", -num, parts)]
            rest -= 2
        if rest:
            chain.append(Fraction("nothing", LF(), self._den(rng, (1,))))
        rng.shuffle(chain)
        self.accs = [(chain[4 * j:4 * j + 4], None) for j in range(self.n_chain)]
        first_total = N_COEF_GLOBALS + 4 * N_CH_GLOBALS
        for j in range(self.n_public):
            frs = [Fraction("public", self._form(rng, codes=True), self._den(rng, (0, 2))) for _ in range(4)]
            self.accs.append((frs, first_total + 4 * j))
        self.words = self._blob()

    def _col(self):
        self.n_data += 1
        return self.n_data - 1

    def _coef(self, rng):
        return rng.choice([1, 2, P - 1, 65536, rng.randrange(1, P)])

    def _form(self, rng, codes=False):
        """a linear form over DATA (and CODE) columns, public-input coefficients and constants"""
        f = LF()
        for _ in range(1 if self.lean else rng.randint(1, 4)):
            what = rng.randrange(4)
            if what == 0:
                f = f + self._coef(rng) * LF.of(1)
            elif what == 1:
                f = f + self._coef(rng) * LF.glob(rng.randrange(N_COEF_GLOBALS))
            elif what == 2 and codes:
                f = f + self._coef(rng) * LF.col(CODE_RANDOM, G_CODE)
            else:
                c = LF.col(rng.choice(self.free + self.sel))
                f = f + self._coef(rng) * (LF.glob(rng.randrange(N_COEF_GLOBALS)) * c if rng.random() < 0.3 else c)
        return f

    def _challenge(self, rng, kinds):
        kind = rng.choice(kinds)
        if kind == 1:
            return ("mix", rng.randrange(len(self.kinds), self.n_mix // 4))
        if kind == 2:
            return ("glob", N_COEF_GLOBALS + 4 * rng.randrange(N_CH_GLOBALS))
        return ("one",)

    def _den(self, rng, kinds):
        """1-8 parts; the first is an extension challenge times one, so that the denominator is not zero"""
        lead = [k for k in kinds if k] or [0]
        parts = [(self._challenge(rng, lead), ONE)]
        for _ in range(rng.randint(0, 1 if self.lean else 7)):
            parts.append((self._challenge(rng, kinds), self._form(rng, codes=True)))
        return parts

    def _table_fraction(self, kind):
        return Fraction("table", -LF.col(self.mult[kind]), [(("mix", kind - 1), ONE), (("one",), -LF.col(self.table_code[kind], G_CODE))])

    def _lookup(self, kind):
        rng = self.rng
        gate = rng.choice([None, None, ("sel", rng.randrange(N_SEL)), ("not", rng.randrange(N_SEL))])
        num = ONE if gate is None else LF.col(self.sel[gate[1]]) if gate[0] == "sel" else 1 - LF.col(self.sel[gate[1]])
        if kind == 1:   # value = k_p pivot + the rest (columns, public-input coefficients, constants): the pivot is solved for
            pivot, k_p = self._col(), self._coef(rng)
            rest = LF()
            for _ in range(rng.randint(0, 3)):
                rest = rest + self._form(rng)
            value = k_p * LF.col(pivot) + rest
            cols = (pivot, k_p, rest)
        else:           # value = a + 256 b + 65536 (a & b) + 2^24, three columns of their own
            a, b, r = self._col(), self._col(), self._col()
            value = LF.col(a) + 256 * LF.col(b) + 65536 * LF.col(r) + ref.TAG_AND
            cols = (a, b, r)
        self.lookups.append((kind, gate, cols))
        return Fraction("lookup", num, [(("mix", kind - 1), ONE), (("one",), -value)], kind)

    def _blob(self):
        b = gc.Builder()
        for g, size in ((G_ACCUM, 4 * len(self.accs)), (G_CODE, len(self.code_cols)), (G_DATA, self.n_data)):
            for c in range(size):
                b.taps.add((g, c, 0))
        cons = []
        first = gc.E(b, b.get(G_CODE, CODE_FIRST, 0), 1)
        accum_constraints(b, gc.E, gc.fp4_mul_sym, self.accs, first, cons)
        x = b.true()
        for _, var, _, _ in cons:
            x = b.and_eqz(x, var)
        taps = sorted(b.taps)
        tap_index = {t: i for i, t in enumerate(taps)}
        steps = [(op, tap_index[(a[1], a[2], a[3])] if op == gc.OP_GET else a, bb, cc) for op, a, bb, cc in b.steps]
        return blob(len(self.accs), len(self.code_cols), self.n_data, taps, self.n_global, self.n_mix, x, steps, self.code_cols,
                    logup_words(self.accs, [(self.mult[k], k) for k in self.kinds]))

    # ---- witnesses
    def witness(self, po2, seed=0, challenges="extreme"):
        """-> (DATA Montgomery words, column-major, multiplicity columns zero; public inputs; mix): the public totals are left zero,
        the challenges among the public inputs and the mix come from the corners of [0, p) (challenges="extreme") or not"""
        rng = np.random.default_rng([self.seed, po2, seed])
        n = 1 << po2
        m = np.asarray(EXTREME, dtype=np.int64)[rng.integers(0, len(EXTREME), size=(self.n_data, n))]
        for k in self.kinds:
            m[self.mult[k]] = 0
        m[self.sel[0]], m[self.sel[1]] = 0, 1
        for s in self.sel[2:]:
            m[s] = rng.integers(0, 2, size=n)
        glob = np.asarray(EXTREME, dtype=np.int64)[rng.integers(0, len(EXTREME), size=self.n_global)]
        mix = np.asarray(EXTREME, dtype=np.int64)[rng.integers(0, len(EXTREME), size=self.n_mix)]
        if challenges != "extreme":
            glob[N_COEF_GLOBALS:] = rng.integers(1, P, size=self.n_global - N_COEF_GLOBALS)
            mix = rng.integers(1, P, size=self.n_mix)
        glob[N_COEF_GLOBALS + 4 * N_CH_GLOBALS:] = 0
        gl = [int(x) for x in glob]
        for kind, gate, cols in self.lookups:
            on = np.ones(n, dtype=bool) if gate is None else (m[self.sel[gate[1]]] == 1) == (gate[0] == "sel")
            if kind == 1:
                v = np.where(rng.random(n) < 0.5, np.asarray(VALUES)[rng.integers(0, len(VALUES), size=n)], rng.integers(0, 1 << 16, size=n))
                v = np.where(on, v, np.asarray([65536, 65537, 1 << 20, P - 1])[rng.integers(0, 4, size=n)])  # gated off: outside the table
                pivot, k_p, rest = cols
                r = rest.evaluate(m, None, gl) if rest.t else 0
                m[pivot] = (v - r) % P * pow(k_p, P - 2, P) % P
            else:
                a, b, r = cols
                m[a] = np.where(rng.random(n) < 0.5, np.asarray(BYTES)[rng.integers(0, len(BYTES), size=n)], rng.integers(0, 256, size=n))
                m[b] = np.where(rng.random(n) < 0.5, np.asarray(BYTES)[rng.integers(0, len(BYTES), size=n)], rng.integers(0, 256, size=n))
                m[r] = np.where(on, m[a] & m[b], (m[a] & m[b]) ^ 1)
        return ref.enc(m).reshape(-1), ref.enc(glob), ref.enc(mix)


def logup_words(accs, tables):
    words = [len(accs), len(tables)]
    for col, kind in tables:
        words += [col, kind]
    for fr, final in accs:
        words += [len(fr), 0xFFFFFFFF if final is None else final]
        for f in fr:
            words += f.words()
    return words


def blob(n_acc, n_code, n_data, taps, n_global, n_mix, ret, steps, code_cols, logup):
    def section(tag, words):
        return [tag, len(words)] + list(words)
    words = [0x31433052, 1, 6]
    words += section(1, [4 * n_acc, n_code, n_data])
    words += section(2, [len(taps)] + [w for t in taps for w in t])
    words += section(3, [n_global, n_mix])
    words += section(4, [len(steps), ret] + [w for st in steps for w in st])
    words += section(5, [n_code] + [w for cc in code_cols for w in cc] + [n_data] + [0] * (5 * n_data))
    words += section(SEC_LOGUP, logup)
    return np.array(words, dtype=np.uint32)


def generate(seed, **kw):
    return Circuit(seed, **kw)


def replace_logup(words, logup):
    """the blob with its LOGUP section replaced (what the parser tests break)"""
    w = [int(x) for x in words]
    out, pos = w[:3], 3
    for _ in range(w[2]):
        tag, n = w[pos], w[pos + 1]
        out += [tag, len(logup)] + list(logup) if tag == SEC_LOGUP else w[pos:pos + 2 + n]
        pos += 2 + n
    return np.array(out, dtype=np.uint32)
