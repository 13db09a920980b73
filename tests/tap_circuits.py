"""Hand-built circuits whose tap sets no shipped circuit has, each with a witness numpy can write down -- so that whole proofs of
them verify, and the oracle, both verifiers and the device paths can be held against each other on register and combo shapes beyond
{0}, {0,1}, {0,1,2}, {0,2}.  Built like the families of evalcheck_circuits.py (tools/gen_circuit.Builder, GROUPS / TAPS / GLOBALS /
POLY only, 2 public inputs, 2 mix words); there is no ACCUM section, so every prover is handed the accumulation: `accum(data, mix)`.

A column is either free (random words) or defined from others by shifts and products of degree at most 3; `x(b)` below is column x
read at back b, np.roll(x, b) -- the row direction of check_ref.  One term per defined column, in the order the columns are listed:
the column minus its definition.  All words in and out are the device's (Montgomery form); groups are [column][row], flat.

  wide   DATA f0 f1 d2 d3:  d2 = sum_{b=1..63} w_b f0(b)            f0 is a 64-tap register, every back the format admits
                            d3 = f0(63) f1(5) + f1 + g0 g1
         CODE c0 c1:        c1 = c0(7) + c0(1)
         ACCUM a0 a1:       a0 = mix0 f0(3) + mix1;  a1 = a0(1) f1 + a0(63)
         combos {0,1,63} {0} {0,1,7} {0..63} {0,5}; 65 DEEP points with z^4
  odd    CODE c0 c1:        c1 = c0(3) c0(31) + c0(32)              {0,3,31,32} is CODE's alone
         DATA f0 f1 d2 d3:  d2 = f0(1) f0(2) f0(5) + f0(63) + g0    five taps: 2 + 2 + 1 two-point passes
                            d3 = f1(31) f1(32) + g1 f1              {0,31,32}: the combo ACCUM's a0 created, joined by DATA
         ACCUM a0 a1:       a0 = mix0 f1 + mix1;  a1 = a0(31) a0(32) + a0
         combos {0,31,32} {0} {0,3,31,32} {0,1,2,5,63}: 3, 1, 4 and 5 divisions
  far    CODE c0;  DATA f0 d1 f2:  d1 = f0 f2(63) + g0 + g1 c0;  ACCUM a0 = mix0 f0 + mix1 d1
         combos {0} and, created last, {0,63} (the last DATA column): a head of two coefficients

`spoilers(n)` names one-cell violations, a DATA cell and an ACCUM cell (the word there plus one), and the table check_ref must give:
a cell of x at row r shows in a term that reads x(b) at row (r + b) mod n.  The accumulation of a spoiled DATA group is made from
the spoiled columns, so a DATA cell shows in DATA's terms only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_circuit  # noqa: E402
from gen_circuit import G_ACCUM, G_CODE, G_DATA  # noqa: E402
from evalcheck_circuits import N_GLOBAL, N_MIX, finish  # noqa: E402

P = gen_circuit.P
R = (1 << 32) % P
R_INV = pow(1 << 32, P - 2, P)
_P = np.uint64(P)


def dec(words):
    """device words -> field elements (uint64)"""
    return (np.asarray(words).astype(np.uint64) * np.uint64(R_INV)) % _P


def enc(values):
    """field elements -> device words"""
    return ((np.asarray(values).astype(np.uint64) % _P) * np.uint64(R) % _P).astype(np.uint32)


def _mul(*xs):
    out = xs[0] % _P
    for x in xs[1:]:
        out = (out * (x % _P)) % _P
    return out


def _add(*xs):
    out = xs[0] % _P
    for x in xs[1:]:
        out = (out + x % _P) % _P
    return out


def _free(rng, n):
    return rng.integers(0, P, n).astype(np.uint64)


GLOB = enc([3, P - 2])  # the public inputs every witness here is made for


class Family:
    """sizes = (ACCUM, CODE, DATA) columns; subclasses give build(b) -> ret, code(n, rng), data(n, rng, code, g), acc(data, mix)"""
    glob = GLOB

    @classmethod
    def blob(cls):
        b = gen_circuit.Builder()
        return finish(b, cls.sizes, cls.build(b))

    @classmethod
    def witness(cls, n, rng):
        """(code, data): the free columns drawn from rng, the others defined from them"""
        code = cls.code(n, rng)
        data = cls.data(n, rng, code, dec(GLOB))
        return enc(np.concatenate(code)), enc(np.concatenate(data))

    @classmethod
    def accum(cls, data, mix):
        """the ACCUM group of DATA group `data` under the mix words `mix`"""
        d = dec(data).reshape(cls.sizes[G_DATA], -1)
        m = dec(mix)
        return enc(np.concatenate(cls.acc(d, m)))


def spoil(words, n, col, row):
    """a copy of a group with the word of (col, row) one more than it was"""
    out = np.array(words, dtype=np.uint32).reshape(-1).copy()
    out[col * n + row] = (int(out[col * n + row]) + R) % P
    return out


WIDE_W = [(b * b + 7) % P for b in range(64)]  # w_1 .. w_63 are distinct (w_0 is not used)


class wide(Family):
    sizes = (2, 2, 4)

    @staticmethod
    def build(b):
        f0 = [b.get(G_DATA, 0, back) for back in range(64)]
        f1, f1_5, d2, d3 = b.get(G_DATA, 1, 0), b.get(G_DATA, 1, 5), b.get(G_DATA, 2, 0), b.get(G_DATA, 3, 0)
        x = b.true()
        s = b.mul(b.const(WIDE_W[1]), f0[1])
        for back in range(2, 64):
            s = b.add(s, b.mul(b.const(WIDE_W[back]), f0[back]))
        x = b.and_eqz(x, b.sub(d2, s))  # 0
        x = b.and_eqz(x, b.sub(d3, b.add(b.add(b.mul(f0[63], f1_5), f1), b.mul(b.glob(0, 0), b.glob(0, 1)))))  # 1
        x = b.and_eqz(x, b.sub(b.get(G_CODE, 1, 0), b.add(b.get(G_CODE, 0, 7), b.get(G_CODE, 0, 1))))  # 2
        a0 = [b.get(G_ACCUM, 0, back) for back in (0, 1, 63)]
        x = b.and_eqz(x, b.sub(a0[0], b.add(b.mul(b.glob(1, 0), f0[3]), b.glob(1, 1))))  # 3
        x = b.and_eqz(x, b.sub(b.get(G_ACCUM, 1, 0), b.add(b.mul(a0[1], f1), a0[2])))  # 4
        return x

    @staticmethod
    def code(n, rng):
        c0 = _free(rng, n)
        return [c0, _add(np.roll(c0, 7), np.roll(c0, 1))]

    @staticmethod
    def data(n, rng, code, g):
        f0, f1 = _free(rng, n), _free(rng, n)
        d2 = np.zeros(n, dtype=np.uint64)
        for back in range(1, 64):
            d2 = _add(d2, _mul(np.uint64(WIDE_W[back]), np.roll(f0, back)))
        d3 = _add(_mul(np.roll(f0, 63), np.roll(f1, 5)), f1, _mul(g[0], g[1]))
        return [f0, f1, d2, d3]

    @staticmethod
    def acc(d, m):
        a0 = _add(_mul(m[0], np.roll(d[0], 3)), m[1])
        return [a0, _add(_mul(np.roll(a0, 1), d[1]), np.roll(a0, 63))]

    @staticmethod
    def spoilers(n):
        # f0's back-0 tap is read by no term: the cell shows through backs 1 .. 63 of d2's term and back 63 of d3's, nowhere else
        return [("data", G_DATA, 0, 0, {0: (63, 1), 1: (1, 63)}),
                ("accum", G_ACCUM, 0, 0, {3: (1, 0), 4: (2, 1)})]  # a0's own term at row 0; a1's through backs 1 and 63


class odd(Family):
    sizes = (2, 2, 4)

    @staticmethod
    def build(b):
        c0 = {back: b.get(G_CODE, 0, back) for back in (3, 31, 32)}
        f0 = {back: b.get(G_DATA, 0, back) for back in (1, 2, 5, 63)}
        f1 = {back: b.get(G_DATA, 1, back) for back in (0, 31, 32)}
        a0 = {back: b.get(G_ACCUM, 0, back) for back in (0, 31, 32)}
        x = b.true()
        x = b.and_eqz(x, b.sub(b.get(G_CODE, 1, 0), b.add(b.mul(c0[3], c0[31]), c0[32])))  # 0
        x = b.and_eqz(x, b.sub(b.get(G_DATA, 2, 0), b.add(b.add(b.mul(b.mul(f0[1], f0[2]), f0[5]), f0[63]), b.glob(0, 0))))  # 1
        x = b.and_eqz(x, b.sub(b.get(G_DATA, 3, 0), b.add(b.mul(f1[31], f1[32]), b.mul(b.glob(0, 1), f1[0]))))  # 2
        x = b.and_eqz(x, b.sub(a0[0], b.add(b.mul(b.glob(1, 0), f1[0]), b.glob(1, 1))))  # 3
        x = b.and_eqz(x, b.sub(b.get(G_ACCUM, 1, 0), b.add(b.mul(a0[31], a0[32]), a0[0])))  # 4
        return x

    @staticmethod
    def code(n, rng):
        c0 = _free(rng, n)
        return [c0, _add(_mul(np.roll(c0, 3), np.roll(c0, 31)), np.roll(c0, 32))]

    @staticmethod
    def data(n, rng, code, g):
        f0, f1 = _free(rng, n), _free(rng, n)
        d2 = _add(_mul(np.roll(f0, 1), np.roll(f0, 2), np.roll(f0, 5)), np.roll(f0, 63), g[0])
        d3 = _add(_mul(np.roll(f1, 31), np.roll(f1, 32)), _mul(g[1], f1))
        return [f0, f1, d2, d3]

    @staticmethod
    def acc(d, m):
        a0 = _add(_mul(m[0], d[1]), m[1])
        return [a0, _add(_mul(np.roll(a0, 31), np.roll(a0, 32)), a0)]

    @staticmethod
    def spoilers(n):
        # the last row: backs 31 and 32 wrap to rows 30 and 31, back 0 stays
        return [("data", G_DATA, 1, n - 1, {2: (3, 30)}),
                ("accum", G_ACCUM, 0, n - 1, {3: (1, n - 1), 4: (3, 30)})]


class far(Family):
    sizes = (1, 1, 3)

    @staticmethod
    def build(b):
        f0, d1, c0 = b.get(G_DATA, 0, 0), b.get(G_DATA, 1, 0), b.get(G_CODE, 0, 0)
        x = b.true()
        x = b.and_eqz(x, b.sub(d1, b.add(b.add(b.mul(f0, b.get(G_DATA, 2, 63)), b.glob(0, 0)), b.mul(b.glob(0, 1), c0))))  # 0
        x = b.and_eqz(x, b.sub(b.get(G_ACCUM, 0, 0), b.add(b.mul(b.glob(1, 0), f0), b.mul(b.glob(1, 1), d1))))  # 1
        return x

    @staticmethod
    def code(n, rng):
        return [_free(rng, n)]

    @staticmethod
    def data(n, rng, code, g):
        f0, f2 = _free(rng, n), _free(rng, n)
        return [f0, _add(_mul(f0, np.roll(f2, 63)), g[0], _mul(g[1], code[0])), f2]

    @staticmethod
    def acc(d, m):
        return [_add(_mul(m[0], d[0]), _mul(m[1], d[1]))]

    @staticmethod
    def spoilers(n):
        return [("data", G_DATA, 2, n - 1, {0: (1, 62)}),  # the last row, read 63 rows on: row 62
                ("accum", G_ACCUM, 0, 7, {1: (1, 7)})]


FAMILIES = {"wide": wide, "odd": odd, "far": far}
# the combos as blob.cpp and the oracle number them (by first appearance over the sorted tap table), as lists of backs
COMBOS = {
    "wide": [[0, 1, 63], [0], [0, 1, 7], list(range(64)), [0, 5]],
    "odd": [[0, 31, 32], [0], [0, 3, 31, 32], [0, 1, 2, 5, 63]],
    "far": [[0], [0, 63]],
}


def registers(blob):
    """[(group, column, [backs])] of a blob's tap table, in table order"""
    import check_ref
    regs = []
    for g, col, back in check_ref.Program(blob).taps:
        if regs and regs[-1][:2] == (g, col):
            regs[-1][2].append(back)
        else:
            regs.append((g, col, [back]))
    return regs


def combos(blob):
    """the distinct back-lists of a blob's registers, by first appearance"""
    out = []
    for _, _, backs in registers(blob):
        if backs not in out:
            out.append(backs)
    return out
