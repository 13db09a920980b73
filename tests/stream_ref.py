"""Plain-Python reference of the DEEP-step streams of eltwise.hip and of the division of scan.hip: Python ints,
Fp4 = Fp[x]/(x^4 - 11), nothing shared with the device code or the oracle but the definitions.  Words go in and come out in Montgomery form (a word w stands for w / 2^32 mod p),
as numpy uint32 arrays laid out as the C ABI lays them out (include/r0hip.h, oracle/orc.h):
  evaluate     natural-order base-field coefficients, one extension point
  mix_poly     combos: extension elements, array of structs [combo][i]; input: base-field columns [c][i]
  sum_extelem  in: array of structs [count][n]; out: four columns [4][n]
  fri_fold     in: four columns [4][16 n_out], coefficients in bit-reversed order; out: four columns [4][n_out]
  poly_divide  array of structs, coefficients low to high
Slow (a few microseconds per field operation): for n up to about 2^10."""
import numpy as np

P = 2013265921
R = (1 << 32) % P
R_INV = pow(1 << 32, P - 2, P)
BETA = 11
FRI_FOLD = 16


def dec(words):
    """Montgomery words -> canonical Python ints"""
    return [int(w) * R_INV % P for w in np.asarray(words).reshape(-1)]


def enc(values):
    """canonical ints -> Montgomery words"""
    return np.array([v % P * R % P for v in values], dtype=np.uint32)


def _ext(values):
    """flat canonical ints, 4 per element -> list of 4-tuples"""
    return [tuple(values[i:i + 4]) for i in range(0, len(values), 4)]


def mul4(a, b):
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return ((c[0] + BETA * c[4]) % P, (c[1] + BETA * c[5]) % P, (c[2] + BETA * c[6]) % P, c[3] % P)


def add4(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def scale4(a, s):
    return tuple(x * s % P for x in a)


ZERO4, ONE4 = (0, 0, 0, 0), (1, 0, 0, 0)


def _flat(elems):
    return enc([v for e in elems for v in e])


def evaluate(coeff_words, x_words):
    """sum_i c[i] x^i by Horner: 4 words"""
    x = tuple(dec(x_words))
    tot = ZERO4
    for c in reversed(dec(coeff_words)):
        tot = mul4(tot, x)
        tot = ((tot[0] + c) % P,) + tot[1:]
    return enc(tot)


def evaluate_any(coeff_words, po2, which, xs_words):
    """out[k] = column which[k] of 2^po2 coefficients at xs[k]: 4 words per request"""
    n = 1 << po2
    xs = np.asarray(xs_words).reshape(-1, 4)
    return np.concatenate([evaluate(coeff_words[int(w) * n:(int(w) + 1) * n], xs[k]) for k, w in enumerate(which)])


def mix_poly(combo_words, mix_start, mix, input_words, combo_of, po2):
    """combos[combo_of[c]][i] += mix_start * mix^c * input[c][i]"""
    n = 1 << po2
    combos, inp = _ext(dec(combo_words)), dec(input_words)
    cur, m = tuple(dec(mix_start)), tuple(dec(mix))
    for c, combo in enumerate(combo_of):
        for i in range(n):
            at = int(combo) * n + i
            combos[at] = add4(combos[at], scale4(cur, inp[c * n + i]))
        cur = mul4(cur, m)
    return _flat(combos)


def sum_extelem(in_words, count, n):
    """out[q][i] = component q of sum_c in[c][i]"""
    inp = _ext(dec(in_words))
    out = [0] * (4 * n)
    for i in range(n):
        tot = ZERO4
        for c in range(count):
            tot = add4(tot, inp[c * n + i])
        for q in range(4):
            out[q * n + i] = tot[q]
    return enc(out)


def _brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


def fri_fold(in_words, mix, n_out):
    """out[idx] = sum_j mix^j * in[brev4(j) * n_out + idx]"""
    n_in = FRI_FOLD * n_out
    w, m = dec(in_words), tuple(dec(mix))
    out = [0] * (4 * n_out)
    for idx in range(n_out):
        tot, cur = ZERO4, ONE4
        for j in range(FRI_FOLD):
            src = _brev(j, 4) * n_out + idx
            tot = add4(tot, mul4(cur, tuple(w[q * n_in + src] for q in range(4))))
            cur = mul4(cur, m)
        for q in range(4):
            out[q * n_out + idx] = tot[q]
    return enc(out)


def poly_divide(words, z):
    """synthetic division by (x - z): (quotient with a zero top coefficient, remainder)"""
    p, zz = _ext(dec(words)), tuple(dec(z))
    cur = ZERO4
    for i in reversed(range(len(p))):
        nxt = add4(mul4(zz, cur), p[i])
        p[i] = cur
        cur = nxt
    return _flat(p), enc(cur)
