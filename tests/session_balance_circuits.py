"""Tuple-style LOGUP circuits with an accumulator whose total is public, for the session balance (r0h_session_balance_*) -- a helper
module for test_session_balance.py and test_gpu_session_balance.py; no tests of its own.

Like balance_circuits, but what has to cancel sits in an accumulator with a `final` and cancels ACROSS SEGMENTS: a session is a list of
witnesses of different sizes, a tuple's producer in one of them and its consumer in another (or given from outside, the verifier's
side).  One chain accumulator whose two fractions cancel on every row goes along, so the blobs are real circuits: they load, and the
chain's own check finds nothing.  Public inputs: 0..3 coefficients (early), the challenges G0 at 4 and G1 at 8, the total at 12; the
last 12 are late.

    Circuit(kind)                               the blob (`words`) of one of KINDS
    session(kind, sizes, seed)               -> (Circuit, [(source, po2, None, DATA words, public inputs)]) balanced over its segments
    slot(session, k, column, row)            -> index of a DATA word of segment k"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_circuit as gc  # noqa: E402
from trace_circuit import G_ACCUM, G_CODE, G_DATA, LF, ONE, SEC_LATE, Fraction, accum_constraints  # noqa: E402

import balance_circuits as bc  # noqa: E402
import logup_circuits as lc  # noqa: E402
import logup_ref as ref  # noqa: E402

P = ref.P
G0, G1 = ("glob", 4), ("glob", 8)
N_GLOBAL, FINAL, N_LATE = 16, 12, 12
col = bc.col
# DATA columns: 0, 1 the produced pair; 2, 3 the consumed pair; 4, 5 the two numerators (the consumer's is negated by its fraction)
N_DATA = 6


def two(a0, a1):
    return [(G0, ONE), (("one",), -col(a0)), (G1, -col(a1))]


def fractions(kind):
    if kind == "pairs":          # +n / (G0 - a0 - G1 a1) over columns 0, 1 and -n / (...) over columns 2, 3
        return [Fraction("produce", col(4), two(0, 1)), Fraction("consume", -col(5), two(2, 3))]
    if kind == "zero part":      # the consumer's denominator has no G1 part: one class with producers whose second coordinate is zero
        return [Fraction("produce", col(4), two(0, 1)), Fraction("consume", -col(5), [(G0, ONE), (("one",), -col(2))])]
    if kind == "nine":           # nine challenge identities under the public-total accumulator (a fraction has at most eight parts)
        return [Fraction("produce", col(4), [(("glob", k), col(0)) for k in range(8)]), Fraction("consume", -col(5), [(("glob", 0), ONE), (("one",), col(1))])]
    if kind == "late":           # a part that reads the VALUE of a late public input
        return [Fraction("produce", col(4), [(G0, ONE), (("one",), LF.glob(5) * col(0))])]
    if kind == "early":          # ... and of an early one, which is fine: the second coordinate is public input 1 times the column
        return [Fraction("produce", col(4), [(G0, ONE), (("one",), -col(0)), (G1, -(LF.glob(1) * col(1)))]), Fraction("consume", -col(5), two(2, 3))]
    raise KeyError(kind)


KINDS = ("pairs", "zero part", "nine", "late", "early")


class Circuit:
    def __init__(self, kind):
        session = fractions(kind)
        while len(session) % 4:
            session.append(Fraction("nothing", LF(), [(G0, ONE)]))
        chain = bc.pair(bc.two, (0, 1), (0, 1)) + [Fraction("nothing", LF(), [(bc.A, ONE)])] * 2    # cancels on every row
        self.kind, self.accs, self.n_data, self.n_global, self.n_mix = kind, [(chain, None), (session, FINAL)], N_DATA, N_GLOBAL, 8
        self.words = self._blob()

    def _blob(self):
        b = gc.Builder()
        for g, size in ((G_ACCUM, 4 * len(self.accs)), (G_CODE, len(bc.CODE_COLS)), (G_DATA, self.n_data)):
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
        words = [int(w) for w in lc.blob(len(self.accs), len(bc.CODE_COLS), self.n_data, taps, self.n_global, self.n_mix, x, steps, bc.CODE_COLS, lc.logup_words(self.accs, []))]
        words[2] += 1
        return np.array(words + [SEC_LATE, 1, N_LATE], dtype=np.uint32)


def session(kind, sizes, seed=0, fill=0.75, producers=True, consumers=True):
    """A balanced session over segments of 2^sizes[k] rows: `fill` of all rows produce one tuple each and as many consume one, every
    tuple produced on one (segment, row) and consumed on another, mostly in another segment; the pairs (a0, a1) are all different.
    producers / consumers = False leaves that side's numerators zero (the other side then stands alone)."""
    rng = np.random.default_rng([seed, len(sizes), sum(kind.encode())] + list(sizes))
    c = Circuit(kind)
    n_rows = [1 << s for s in sizes]
    total = sum(n_rows)
    t = max(1, int(total * fill))
    a0 = np.where(rng.random(t) < 0.5, np.asarray(lc.EXTREME, dtype=np.int64)[rng.integers(0, len(lc.EXTREME), size=t)], rng.integers(0, P, size=t))
    a1 = np.zeros(t, dtype=np.int64) if kind == "zero part" else np.arange(t, dtype=np.int64) + 1
    if kind == "zero part":
        a0 = rng.choice(P, size=t, replace=False).astype(np.int64)   # told apart by a0 alone
    glob = np.zeros(N_GLOBAL, dtype=np.int64)
    glob[:4] = [3, 5, 7, 11]
    m = np.zeros((N_DATA, total), dtype=np.int64)    # all segments side by side
    where_p, where_c = rng.permutation(total)[:t], rng.permutation(total)[:t]
    k1 = pow(5, P - 2, P) if kind == "early" else 1     # "early": the producer's column holds a1 / public input 1
    m[0, where_p], m[1, where_p], m[4, where_p] = a0, a1 * k1 % P, 1 if producers else 0
    m[2, where_c], m[3, where_c], m[5, where_c] = a0, a1, 1 if consumers else 0
    out, at = [], 0
    for k, n in enumerate(n_rows):
        out.append((k, sizes[k], None, ref.enc(m[:, at:at + n]).reshape(-1), ref.enc(glob)))
        at += n
    return c, out


def slot(segments, k, column, row):
    return column * (1 << segments[k][1]) + row
