"""Tuple-style LOGUP circuits for the balance check (r0h_logup_check_balance) -- a helper module for test_balance.py and
test_gpu_balance.py; no tests of its own.

Where logup_circuits.generate pairs fractions that cancel on the same row, these are producers +n / (c - a0 - b a1 ...) and consumers
-n / (...) over DIFFERENT columns whose witnesses are permutations of one another: the cancellation happens across rows, which is what
the balance check has to see.  Every circuit is a real blob (logup_circuits.blob / logup_words, trace_circuit.Fraction /
accum_constraints): it loads, and its seals would prove like the committed circuits'.  No tables: the CODE group is not read.

    scenario(name, po2, seed) -> (Circuit, DATA words with the argument balanced, public inputs)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_circuit as gc  # noqa: E402
from trace_circuit import G_ACCUM, G_CODE, G_DATA, LF, ONE, Fraction, accum_constraints  # noqa: E402

import logup_circuits as lc  # noqa: E402
import logup_ref as ref  # noqa: E402

P = ref.P
A, B = ("mix", 0), ("mix", 1)      # the tuple's constant term and its second coordinate's weight
G = ("glob", 0)                    # a challenge among the public inputs
CODE_COLS = [(0, 0), (1, 0), (3, 7)]


class Circuit:
    def __init__(self, fractions, n_data, n_global=0, n_mix=8):
        fractions = list(fractions)
        while len(fractions) % 4:
            fractions.append(Fraction("nothing", LF(), [(A, ONE)]))   # a numerator of zero: never a tuple
        self.fractions, self.n_data, self.n_global, self.n_mix = fractions, n_data, n_global, n_mix
        self.accs = [(fractions[i:i + 4], None) for i in range(0, len(fractions), 4)]
        self.words = self._blob()

    def _blob(self):
        b = gc.Builder()
        for g, size in ((G_ACCUM, 4 * len(self.accs)), (G_CODE, len(CODE_COLS)), (G_DATA, self.n_data)):
            for c in range(size):
                b.taps.add((g, c, 0))
        cons = []
        accum_constraints(b, gc.E, gc.fp4_mul_sym, self.accs, gc.E(b, b.get(G_CODE, 0, 0), 1), cons)
        x = b.true()
        for _, var, _, _ in cons:
            x = b.and_eqz(x, var)
        taps = sorted(b.taps)
        tap_index = {t: i for i, t in enumerate(taps)}
        steps = [(op, tap_index[(a[1], a[2], a[3])] if op == gc.OP_GET else a, bb, cc) for op, a, bb, cc in b.steps]
        return lc.blob(len(self.accs), len(CODE_COLS), self.n_data, taps, self.n_global, self.n_mix, x, steps, CODE_COLS, lc.logup_words(self.accs, []))


def col(k):
    return LF.col(k)


def pair(parts_of, cols_p, cols_c, num_p=ONE, num_c=-ONE):
    """a producer over cols_p and a consumer over cols_c with denominators of one shape"""
    return [Fraction("produce", num_p, parts_of(*cols_p)), Fraction("consume", num_c, parts_of(*cols_c))]


def two(a0, a1):
    return [(A, ONE), (("one",), -col(a0)), (B, -col(a1))]


def five(first):
    """a pair's denominator spread over the five mix challenges from `first` on and over "one": six identities"""
    m = [("mix", first + k) for k in range(5)]
    return lambda a0, a1: [(m[0], ONE), (("one",), -col(a0)), (m[1], -col(a1)), (m[2], -col(a0)), (m[3], -col(a1)), (m[4], -col(a0))]


def _values(rng, n):
    """n field elements from the corners of [0, p) and from all of it, no two rows' pairs alike (the second coordinate is the row)"""
    corner = np.asarray(lc.EXTREME, dtype=np.int64)[rng.integers(0, len(lc.EXTREME), size=n)]
    return np.where(rng.random(n) < 0.5, corner, rng.integers(0, P, size=n))


def scenario(name, po2, seed=0):
    rng = np.random.default_rng([seed, po2, sum(name.encode())])
    n = 1 << po2
    perm = rng.permutation(n)
    rows = np.arange(n, dtype=np.int64)
    glob = ref.enc(rng.integers(1, P, size=4))
    if name == "permutation":   # (a0, row) produced, consumed in another order; a third fraction whose numerator is zero over garbage parts
        c = Circuit(pair(two, (0, 1), (2, 3)) + [Fraction("gated", col(4), [(A, col(5)), (B, col(6)), (("one",), col(0))])], 7)
        m = np.zeros((7, n), dtype=np.int64)
        m[0], m[1] = _values(rng, n), rows
        m[2], m[3] = m[0][perm], m[1][perm]
        m[5], m[6] = rng.integers(0, P, size=n), rng.integers(0, P, size=n)
    elif name == "order":       # one class reached through parts in another order, under a public challenge, and through a challenge split over two parts
        frs = [Fraction("produce", ONE, [(A, ONE), (("one",), -col(0)), (G, -col(1))]),
               Fraction("consume", -ONE, [(G, -col(3)), (A, ONE), (("one",), -col(2))]),
               Fraction("produce2", ONE, [(A, ONE), (("one",), -col(0)), (G, -col(1))]),
               Fraction("consume2", -ONE, [(G, -col(4)), (("one",), -col(2)), (G, -col(5)), (A, LF.of(2)), (A, -ONE)])]
        c = Circuit(frs, 6, n_global=4)
        m = np.zeros((6, n), dtype=np.int64)
        m[0], m[1] = _values(rng, n), rows
        m[2], m[3] = m[0][perm], m[1][perm]
        m[4] = rng.integers(0, P, size=n)
        m[5] = (m[3] - m[4]) % P
    elif name == "zero part":   # a part whose value is zero on every row against a denominator without that part
        c = Circuit([Fraction("produce", ONE, two(0, 1)), Fraction("consume", -ONE, [(A, ONE), (("one",), -col(2))])], 3)
        m = np.zeros((3, n), dtype=np.int64)
        m[0] = rng.permutation(n) * 3 % P
        m[2] = m[0][perm]
    elif name == "weights":     # numerators a and p - a on one class
        c = Circuit(pair(two, (0, 1), (2, 3), num_p=col(4), num_c=col(5)), 6)
        m = np.zeros((6, n), dtype=np.int64)
        m[0], m[1], m[4] = _values(rng, n), rows, np.where(rng.random(n) < 0.5, rng.integers(1, P, size=n), np.asarray([1, P - 1, (P - 1) // 2])[rng.integers(0, 3, size=n)])
        m[2], m[3], m[5] = m[0][perm], m[1][perm], (P - m[4][perm]) % P
    elif name == "minus ones":  # p - 1 on every row of one class (the sum passes many multiples of p) against the count on one row
        c = Circuit([Fraction("consume", -ONE, [(A, ONE), (("one",), -col(0))]), Fraction("produce", col(1), [(A, ONE), (("one",), -col(2))])], 3)
        m = np.zeros((3, n), dtype=np.int64)
        m[0], m[2] = 9, 9
        m[1, n // 3] = n
    elif name == "own class":   # eight fractions, every tuple in a class of its own: 8 n classes, none of which balances
        c = Circuit([Fraction("f%d" % k, ONE, [(A, ONE), (("one",), -col(k)), (B, LF.of(k + 1))]) for k in range(8)], 8)
        m = np.stack([rng.permutation(n) + 17 * k for k in range(8)]).astype(np.int64)
    elif name in ("hot", "surplus"):   # every row in ONE class on both sides; with one producer too many
        c = Circuit(pair(lambda a: [(A, ONE), (("one",), -col(a))], (0,), (1,)) + [Fraction("extra", col(2), [(A, ONE), (("one",), -col(0))])], 3)
        m = np.zeros((3, n), dtype=np.int64)
        m[0], m[1] = 7, 7
        if name == "surplus":
            m[2, n - 3] = 1
    elif name == "many identities":   # two pairs under five mix challenges each: eleven identities with "one", more than a session's eight
        c = Circuit(pair(five(0), (0, 1), (2, 3)) + pair(five(5), (4, 5), (6, 7)), 8, n_mix=40)
        m = np.zeros((8, n), dtype=np.int64)
        other = rng.permutation(n)
        m[0], m[1], m[4], m[5] = _values(rng, n), rows, _values(rng, n), rows
        m[2], m[3], m[6], m[7] = m[0][perm], m[1][perm], m[4][other], m[5][other]
    else:
        raise KeyError(name)
    return c, ref.enc(m).reshape(-1), glob[:c.n_global]


def altered(data, po2, column, row):
    """the witness with one cell changed (by one)"""
    bad = data.copy()
    at = (column << po2) + row
    bad[at] = ref.enc((int(ref.dec(bad[at])) + 1) % P)
    return bad


SCENARIOS = ("permutation", "order", "zero part", "weights", "minus ones", "own class", "hot", "surplus", "many identities")
BALANCED = ("permutation", "order", "zero part", "weights", "minus ones", "hot", "many identities")
