"""Hand-built circuit blobs that aim at the structural rules of the constraint-evaluator generator (csrc/evalcheck_emit.cpp), one
family per rule, built on tools/gen_circuit.Builder and carrying only the GROUPS, TAPS, GLOBALS and POLY sections (no column
program: the tests supply every operand).  Each family returns the blob as uint32 words.

Every circuit declares 2 public inputs and 2 mix words whether it reads them or not, and every group at least one column, so that
all of them are driven through the same calls.  `CUTS` names the R0H_EC_BUDGET values the cut variants are loaded under and the
number of kernels each must give -- the tests read that number back from the emitted text."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_circuit  # noqa: E402
from gen_circuit import G_ACCUM, G_CODE, G_DATA  # noqa: E402

P = gen_circuit.P
N_GLOBAL = N_MIX = 2
BARE_SIZES = (1, 3, 4, 5, 6, 7, 8, 9, 33)


def finish(b, groups, ret):
    """the blob of Builder `b`: every column of every group owns a back-0 tap, taps sorted, GET steps renumbered to the table"""
    for g, size in enumerate(groups):
        for col in range(size):
            b.taps.add((g, col, 0))
    taps = sorted(b.taps)
    index = {t: i for i, t in enumerate(taps)}
    steps = [(op, index[a[1:]] if op == gen_circuit.OP_GET else a, bb, c) for op, a, bb, c in b.steps]

    def section(tag, words):
        return [tag, len(words)] + list(words)

    words = [gen_circuit.MAGIC, 1, 4]
    words += section(gen_circuit.SEC_GROUPS, list(groups))
    words += section(gen_circuit.SEC_TAPS, [len(taps)] + [w for t in taps for w in t])
    words += section(gen_circuit.SEC_GLOBALS, [N_GLOBAL, N_MIX])
    words += section(gen_circuit.SEC_POLY, [len(steps), ret] + [w for s in steps for w in s])
    return np.array(words, dtype=np.uint32)


def bare(n_terms, backs=None):
    """Running 64-bit sums (emit_accumulate, dfix, dfinish): term t is the bare tap of DATA column t (at back backs[t], default 0),
    so the term values are the operand words themselves and all of them can be p - 1 at once.  Four products fit as they are; from
    position 4 on the high word is corrected before every second product: 4 | 5 | 6 | 7 terms walk that cadence, 33 runs it long."""
    b = gen_circuit.Builder()
    x = b.true()
    for t in range(n_terms):
        x = b.and_eqz(x, b.get(G_DATA, t, backs[t] if backs else 0))
    return finish(b, (1, 1, n_terms), x)


def lazy():
    """Lazy additions (lazy_additions): an ADD stays uncorrected (below 2p) only if every reader is a product, at most one operand
    of a product may be uncorrected, a square never takes one, and a sum that is a term's value, a gate or an operand of ADD/SUB
    is corrected.  One term (or pair of terms) per rule, over six DATA columns a..f."""
    b = gen_circuit.Builder()
    a, bb, c, d, e, f = (b.get(G_DATA, k, 0) for k in range(6))
    x = b.true()
    x = b.and_eqz(x, b.mul(b.add(a, bb), b.add(c, d)))  # 0: a product of two sums: exactly one may stay uncorrected
    s = b.add(e, f)
    x = b.and_eqz(x, b.mul(s, s))  # 1: the square of a sum
    s = b.add(a, c)
    x = b.and_eqz(x, b.sub(b.mul(s, bb), b.sub(s, d)))  # 2: a sum read by a product and by a SUB
    s = b.add(bb, d)
    x = b.and_eqz(x, b.mul(s, e))  # 3: a sum read by a product ...
    x = b.and_eqz(x, s)  # 4: ... and used as a term's value (two readers of one sub-expression, in adjacent terms)
    s = b.add(c, e)
    x = b.and_cond(x, s, b.and_eqz(b.true(), b.mul(s, f)))  # 5: a sum used as a gate (and read by a product)
    s = b.add(a, f)
    x = b.and_eqz(x, b.mul(b.mul(s, d), s))  # 6: a sum used twice in a product chain, (s * x) * s
    x = b.and_eqz(x, b.mul(b.add(b.add(a, bb), b.add(c, d)), e))  # 7: a sum of two sums
    x = b.and_eqz(x, b.mul(b.add(d, f), b.const(P - 1)))  # 8: a sum times a CONST,
    x = b.and_eqz(x, b.mul(b.add(a, e), b.glob(0, 1)))  # 9: times a public input,
    x = b.and_eqz(x, b.mul(b.add(bb, f), b.glob(1, 0)))  # 10: and times a mix word (a late term)
    return finish(b, (1, 1, 6), x)


def gates():
    """Gates (flatten): an AndCond multiplies every inner term by its gate and consumes as many powers of poly_mix as its inner
    chain holds; gates nest (depth 3 here), and an inner chain can be True alone, which takes no power -- the next term's power
    must not move.  Also: a gate that is a back-tap of CODE, a term that is CONST p - 1, terms that are a public input alone, and
    late terms (an ACCUM tap times a mix word) between early ones and at the end."""
    b = gen_circuit.Builder()
    d = [b.get(G_DATA, k, 0) for k in range(6)]
    x = b.true()
    x = b.and_eqz(x, d[0])  # 0
    x = b.and_eqz(x, b.mul(b.get(G_ACCUM, 0, 0), b.glob(1, 0)))  # 1: late, between early terms
    x = b.and_eqz(x, b.const(P - 1))  # 2
    in3 = b.and_eqz(b.and_eqz(b.true(), d[4]), b.glob(0, 0))  # 5, 6 under three gates
    in2 = b.and_eqz(b.and_cond(b.and_eqz(b.true(), d[3]), b.get(G_CODE, 1, 0), in3), d[5])  # 4 | 5, 6 | 7 under two
    in1 = b.and_eqz(b.and_cond(b.and_eqz(b.true(), d[1]), d[2], in2), b.sub(d[0], d[1]))  # 3 | 4..7 | 8 under one
    x = b.and_cond(x, b.get(G_CODE, 0, 1), in1)  # the outer gate is a back-tap of CODE
    x = b.and_cond(x, d[5], b.true())  # an empty inner chain: no term, no power
    x = b.and_eqz(x, b.glob(0, 1))  # 9: a public input alone, at power 9
    x = b.and_eqz(x, b.mul(b.get(G_ACCUM, 0, 1), b.glob(1, 1)))  # 10: late
    return finish(b, (1, 2, 6), x)


TAP_BACKS = (0, 1, 2, 63)


def taps():
    """Taps: eval_check reads tap (column, back) at row (i - 4 back) mod 4N, check_witness at row (i - back) mod N; 63 is the largest
    back the blob format admits.  Backs {0, 1, 2, 63} on column 0 of each of ACCUM, CODE and DATA; per group the terms are the
    differences of neighbouring backs and, against a second column read at back 0 only, the back-63 tap alone: a cell planted in
    row 0 of column 0 shows in that term at row 63 and nowhere else."""
    b = gen_circuit.Builder()
    x = b.true()
    for g in (G_DATA, G_ACCUM, G_CODE):
        t = [b.get(g, 0, back) for back in TAP_BACKS]
        for k in range(3):
            x = b.and_eqz(x, b.sub(t[k], t[k + 1]))
        x = b.and_eqz(x, b.sub(t[3], b.get(g, 1, 0)))
    return finish(b, (2, 2, 2), x)


FAMILIES = {"lazy": lazy, "gates": gates, "taps": taps}
FAMILIES.update({"bare%d" % n: (lambda n=n: bare(n)) for n in BARE_SIZES})
# bare terms at back-offsets: the cadence and the tap rule in one circuit
FAMILIES["bare9back"] = lambda: bare(9, [0, 63, 1, 62, 2, 0, 63, 31, 32])

# (family, R0H_EC_BUDGET) -> kernels.  A term costs its not-yet-emitted expression nodes + 8, and a kernel closes before the term
# that would take it over the budget, so budget 1 makes every term its own kernel: every pair of terms that share a sub-expression
# is cut apart (lazy 3 | 4 share a sum, gates' terms share their gates), and the late terms of gates and taps land in kernels of
# their own.  The larger budgets cut after every second or third term, so that kernels hold shared sub-expressions inside and
# across their borders at once (lazy @ 30 cuts 2 3 | 4 5), and early and late terms share a kernel (gates @ 24: 0 1 | .. | 10,
# gates @ 40: 0 1 2 3 | .. | 8 9 10, taps @ 40: 3 4 5 | 6 7 8).  The counts are what make_plan gives; the tests read them back.
CUTS = {
    ("bare9", 1): 9, ("bare9", 20): 5, ("bare9", 30): 3,
    ("lazy", 1): 11, ("lazy", 30): 6,
    ("gates", 1): 11, ("gates", 24): 6, ("gates", 40): 3,
    ("taps", 1): 12, ("taps", 24): 6, ("taps", 40): 4,
}


def cases():
    """[(family, budget or None)]: every hand circuit under the default budget (one kernel), then the cut variants"""
    return [(name, None) for name in FAMILIES] + sorted(CUTS)


def case_id(case):
    return case[0] if case[1] is None else "%s@%d" % case


def kernels_in(text):
    """K of the `// terms: .., kernels: K` line of either emitted text"""
    return int(text.split("// terms: ")[1].split("kernels: ")[1].split("\n")[0])


# the operand families of field_words.py and one more: `near`, every word within 1024 of p.  A product of two uncorrected sums
# (or the square of one) leaves Montgomery's bound by a margin that depends on the low words: with every operand exactly p - 1 it
# happens to stay inside (the all-top family is one point), with operands spread just below p it leaves it on most lanes.
KINDS = ("random", "pool", "top", "near")


def words(rng, n, kind):
    import field_words
    if kind == "near":
        return (P - 1 - rng.integers(0, 1024, size=n)).astype(np.uint32)
    return field_words.family(rng, n, kind)


# ---- planted witnesses for the witness checker: all-zero columns with a few non-zero cells ---------------------------------
def row_sets(n):
    """the rows a planted column is non-zero on: the edges of a wave and of the trace, a whole wave, one row in each of two blocks"""
    sets = [[0], [63], [n - 1]]
    if n > 64:
        sets += [[64], [63, 64], list(range(64, 128))]
    else:
        sets += [list(range(64))]
    if n > 256:
        sets += [[5, 300]]
    return sets


def planted(name, n, rows, rng, k):
    """(accum, code, data, glob, mix) for `gates` or `taps`, groups as [column][row] arrays: zero but for non-zero words on `rows`
    of the columns the terms read bare, with every gate open; the public inputs alternate with k between (x, 0) and (0, x)"""
    sizes = {"gates": (1, 2, 6), "taps": (2, 2, 2)}[name]
    accum, code, data = (np.zeros((size, n), dtype=np.uint32) for size in sizes)
    cells = lambda: rng.integers(1, P, len(rows)).astype(np.uint32)
    if name == "gates":
        code[:] = rng.integers(1, P, code.shape)  # both CODE gates open on every row
        data[2] = rng.integers(1, P, n)  # the DATA gate too
        for col in (0, 3, 4):
            data[col, rows] = cells()
        accum[0, rows] = cells()
        glob = np.array([int(rng.integers(1, P)), 0] if k % 2 else [0, int(rng.integers(1, P))], dtype=np.uint32)
    else:
        for g in (accum, code, data):
            g[0, rows] = cells()
        glob = np.zeros(2, dtype=np.uint32)
    return accum, code, data, glob, rng.integers(1, P, 2).astype(np.uint32)


def planted_cases(name, po2, seed=19):
    """[(rows, witness, check_ref's table with the accumulation, and without)] over row_sets, the scenario asserted: term 0 of
    gates is the planted column itself, and through the back-63 tap of taps a cell shows 63 rows on and nowhere else"""
    import check_ref
    blob, n = FAMILIES[name](), 1 << po2
    late = check_ref.Program(blob).late
    rng = np.random.default_rng([seed, po2])
    out = []
    for k, rows in enumerate(row_sets(n)):
        accum, code, data, glob, mix = w = planted(name, n, rows, rng, k)
        want = check_ref.check(blob, po2, code, data, glob, accum, mix)
        early = check_ref.check(blob, po2, code, data, glob)
        if name == "gates":
            assert want[0] == (len(rows), rows[0]) and want[2] == (n, 0)
        else:
            assert want[3] == (len(rows), min((r + 63) % n for r in rows)) and (rows != [0] or want[3] == (1, 63))
        assert any(late[t] for t in want) and early == {t: v for t, v in want.items() if not late[t]}
        out.append((rows, w, want, early))
    return out
