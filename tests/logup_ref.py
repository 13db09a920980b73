"""An exact restatement of the log-derivative argument (blob section LOGUP, include/r0hip_circuit.h) in canonical integers, for the
tests (a helper module; no tests of its own).

It reads the blob's words itself -- GROUPS, GLOBALS and LOGUP -- and shares no code with the library's parser, the oracle's or
tools/trace_circuit.py.  Arithmetic is numpy int64 over canonical residues, reduced after every product; the extension field is
GF(p)[x] / (x^4 - 11), and a whole column of extension elements is inverted at once (the norm down to GF(p), then Fermat).  Inputs
and outputs are the library's words (Montgomery form: x is stored as x 2^32 mod p), column-major like the DATA group.

    multiplicities(blob, data, glob, po2)   -> data with the multiplicity columns filled      (r0h_logup_multiplicities)
    row_terms(...)                          -> every accumulator's sum of fractions, row by row
    accum(...)                              -> the ACCUM group                                 (r0h_accum_public)
    totals(...)                             -> the public inputs with the public totals filled  (r0h_logup_totals)
"""
import numpy as np

P = 2013265921
R = (1 << 32) % P
R_INV = pow(1 << 32, P - 2, P)
BETA = 11
TAG_AND = 1 << 24
G_ACCUM, G_CODE, G_DATA = 0, 1, 2
SEC_GROUPS, SEC_GLOBALS, SEC_LOGUP = 1, 3, 10
CHAIN = 0xFFFFFFFF


class LogupError(ValueError):
    """the witness breaks the argument's contract (a numerator other than 0 or 1, a value outside its table, too many lookups)"""


# ---- Montgomery words <-> canonical integers
def dec(words):
    return np.asarray(words, dtype=np.uint32).astype(np.int64) * R_INV % P


def enc(x):
    return (np.asarray(x, dtype=np.int64) % P * R % P).astype(np.uint32)


# ---- the blob
def parse(blob):
    """-> dict(groups, n_global, n_mix, tables [(data column, kind)], accs [(final or None, [fraction])]); a fraction is
    dict(table, num, parts [(challenge kind, index, form)]) and a form [(coef, global + 1 or 0, ref + 1 or 0)]"""
    w = [int(x) for x in np.asarray(blob, dtype=np.uint32)]
    assert w[0] == 0x31433052 and w[1] == 1, "not a circuit blob"
    out, pos = {}, 3
    for _ in range(w[2]):
        tag, n = w[pos], w[pos + 1]
        body = w[pos + 2:pos + 2 + n]
        pos += 2 + n
        if tag == SEC_GROUPS:
            out["groups"] = body[:3]
        elif tag == SEC_GLOBALS:
            out["n_global"], out["n_mix"] = body[0], body[1]
        elif tag == SEC_LOGUP:
            it = iter(body)
            nx = lambda: next(it)

            def form():
                return [(nx(), nx(), nx()) for _ in range(nx())]
            n_acc, n_tab = nx(), nx()
            out["tables"] = [(nx(), nx()) for _ in range(n_tab)]
            accs = []
            for _ in range(n_acc):
                nf, final = nx(), nx()
                frs = []
                for _ in range(nf):
                    table = nx()
                    num = form()
                    parts = [(nx(), nx(), form()) for _ in range(nx())]
                    frs.append(dict(table=table, num=num, parts=parts))
                accs.append((None if final == CHAIN else final, frs))
            out["accs"] = accs
    return out


def n_chain(c):
    return sum(1 for final, _ in c["accs"] if final is None)


# ---- GF(p) and GF(p^4) on whole columns
def pow_p(a, e):
    a = np.asarray(a, dtype=np.int64) % P
    r = np.ones_like(a)
    while e:
        if e & 1:
            r = r * a % P
        a = a * a % P
        e >>= 1
    return r


def inv_p(a):
    return pow_p(a, P - 2)  # 0 -> 0, as the kernels' inverse


def mul4(x, y):
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] = (c[i + j] + x[i] * y[j] % P) % P
    return [(c[0] + BETA * c[4]) % P, (c[1] + BETA * c[5]) % P, (c[2] + BETA * c[6]) % P, c[3] % P]


def add4(x, y):
    return [(a + b) % P for a, b in zip(x, y)]


def scale4(x, s):
    return [a * s % P for a in x]


def inv4(a):
    """a = A(y) + x B(y), y = x^2 (y^2 = 11): a (A - x B) = A^2 - y B^2 =: D(y) in GF(p^2), D (D0 - D1 y) = D0^2 - 11 D1^2 in GF(p)"""
    a0, a1, a2, a3 = a
    A2_0, A2_1 = (a0 * a0 % P + BETA * (a2 * a2 % P)) % P, 2 * a0 % P * a2 % P
    B2_0, B2_1 = (a1 * a1 % P + BETA * (a3 * a3 % P)) % P, 2 * a1 % P * a3 % P
    D0, D1 = (A2_0 - BETA * B2_1) % P, (A2_1 - B2_0) % P          # A^2 - y B^2
    norm = inv_p((D0 * D0 % P - BETA * (D1 * D1 % P)) % P)
    I0, I1 = D0 * norm % P, (-D1 * norm) % P                        # 1 / D = I0 + I1 y
    # 1 / a = (A - x B) / D
    return [(a0 * I0 % P + BETA * (a2 * I1 % P)) % P, (-(a1 * I0 % P + BETA * (a3 * I1 % P))) % P,
            (a0 * I1 % P + a2 * I0 % P) % P, (-(a1 * I1 % P + a3 * I0 % P)) % P]


# ---- the argument
class Columns:
    """canonical views of the witness: CODE / DATA columns, public inputs, mix (all canonical int64)"""

    def __init__(self, c, po2, code, data, glob, mix):
        self.n = 1 << po2
        self.code = None if code is None else dec(code).reshape(-1, self.n)
        self.data = dec(data).reshape(-1, self.n)
        self.glob = None if glob is None else [int(x) for x in dec(glob)]
        self.mix = None if mix is None else [int(x) for x in dec(mix)]

    def form(self, f):
        acc = np.zeros(self.n, dtype=np.int64)
        for coef, g, ref in f:
            k = coef                                 # (canonical in the blob)
            if g:
                k = k * self.glob[g - 1] % P
            if ref:
                grp, col = (ref - 1) >> 28, (ref - 1) & 0xFFFFF
                acc = (acc + k * (self.data if grp == G_DATA else self.code)[col]) % P
            else:
                acc = (acc + k) % P
        return acc

    def challenge(self, kind, idx):
        if kind == 1:
            return self.mix[4 * idx:4 * idx + 4]
        return self.glob[idx:idx + 4]


def _term(cols, frs):
    """one accumulator's sum of its four fractions on every row, formed as the kernels form it:
    ((n0 d1 + n1 d0) d23 + (n2 d3 + n3 d2) d01) / (d01 d23) -- a zero denominator gives zero, as their inverse does"""
    z = np.zeros(cols.n, dtype=np.int64)
    d, num = [], []
    for f in frs:
        den = [z, z, z, z]
        for kind, idx, lf in f["parts"]:
            v = cols.form(lf)
            if kind == 0:
                den = [(den[0] + v) % P] + den[1:]
            else:
                den = add4(den, [v * int(e) % P for e in cols.challenge(kind, idx)])
        d.append(den)
        num.append(cols.form(f["num"]))
    d01, d23 = mul4(d[0], d[1]), mul4(d[2], d[3])
    top = add4(mul4(add4(scale4(d[1], num[0]), scale4(d[0], num[1])), d23), mul4(add4(scale4(d[3], num[2]), scale4(d[2], num[3])), d01))
    return mul4(top, inv4(mul4(d01, d23)))


def row_terms(blob, po2, code, data, glob, mix, which=None):
    """-> {accumulator index: [4 canonical int64 arrays]}: the accumulator's sum of fractions on every row"""
    c = parse(blob)
    cols = Columns(c, po2, code, data, glob, mix)
    which = range(len(c["accs"])) if which is None else which
    return {j: _term(cols, c["accs"][j][1]) for j in which}


def accum(blob, po2, code, data, glob, mix):
    """the ACCUM group (Montgomery words, column-major): the chain's one sum runs through every row's links and on through the rows
    from row 0; an accumulator with a public total runs alone"""
    c = parse(blob)
    n, nc = 1 << po2, n_chain(c)
    terms = row_terms(blob, po2, code, data, glob, mix)
    out = np.zeros((4 * len(c["accs"]), n), dtype=np.uint32)
    within = [[np.zeros(n, dtype=np.int64)] * 4]
    for j in range(nc):
        within.append(add4(within[-1], terms[j]))
    row_total = within[-1]
    before = [np.concatenate(([0], np.cumsum(t)[:-1] % P)) for t in row_total]   # the sum of all earlier rows (values < 2^31, n <= 2^24: no overflow)
    for j in range(nc):
        for i in range(4):
            out[4 * j + i] = enc((within[j + 1][i] + before[i]) % P)
    for j in range(nc, len(c["accs"])):
        for i in range(4):
            out[4 * j + i] = enc(np.cumsum(terms[j][i]) % P)
    return out.reshape(-1)


def totals(blob, po2, code, data, glob):
    """the public inputs with the total of every accumulator that runs alone written where the circuit reads it"""
    c = parse(blob)
    nc = n_chain(c)
    glob = np.array(glob, dtype=np.uint32).copy()
    terms = row_terms(blob, po2, code, data, glob, None, range(nc, len(c["accs"])))
    for j in range(nc, len(c["accs"])):
        glob[c["accs"][j][0]:c["accs"][j][0] + 4] = enc([int(t.sum() % P) for t in terms[j]])
    return glob


def lookups(blob, po2, data, glob):
    """-> [(table kind, numerator, value)] per lookup slot, canonical int64 columns (the value decoded: minus the form of part 1)"""
    c = parse(blob)
    cols = Columns(c, po2, None, data, glob, None)
    out = []
    for final, frs in c["accs"]:
        for f in frs:
            if f["table"]:
                out.append((f["table"], cols.form(f["num"]), (-cols.form(f["parts"][1][2])) % P))
    return out


def multiplicities(blob, data, glob, po2):
    """data (Montgomery words) with every table's multiplicity column filled: entry v counts the rows whose numerator is 1 and whose
    value is v.  Raises LogupError where the contract does: a numerator other than 0 or 1, a value outside its table on a row whose
    numerator is 1, more than p - 1 lookup slots of one table."""
    c = parse(blob)
    n = 1 << po2
    data = np.array(data, dtype=np.uint32).reshape(-1, n).copy()
    if not c["tables"]:
        return data.reshape(-1)
    if po2 < 16:
        raise LogupError("the tables have 2^16 rows")
    slots = [0] * len(c["tables"])
    for final, frs in c["accs"]:
        for f in frs:
            if f["table"]:
                slots[f["table"] - 1] += n
    if max(slots) > P - 1:
        raise LogupError("more than p - 1 lookups of one table")
    hist = [np.zeros(1 << 16, dtype=np.int64) for _ in c["tables"]]
    for table, num, value in lookups(blob, po2, data, glob):
        if np.any((num != 0) & (num != 1)):
            raise LogupError("a numerator other than 0 or 1")
        v = value[num == 1]
        if c["tables"][table - 1][1] == 2:
            v = v - TAG_AND
            a, b, r = v & 255, (v >> 8) & 255, v >> 16
            if np.any((v < 0) | (v >> 24 != 0) | ((a & b) != r)):
                raise LogupError("a value outside the byte-AND table")
            v = v & 0xFFFF
        elif np.any(v >> 16):
            raise LogupError("a value outside the 16-bit range table")
        hist[table - 1] += np.bincount(v, minlength=1 << 16)
    for k, (col, kind) in enumerate(c["tables"]):
        data[col] = 0
        data[col, :1 << 16] = enc(hist[k])
    return data.reshape(-1)
