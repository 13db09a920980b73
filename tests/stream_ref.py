"""Plain-Python reference of the DEEP-step streams of eltwise.hip and of the division of scan.hip: Python ints,
Fp4 = Fp[x]/(x^4 - 11), nothing shared with the device code or the oracle but the definitions.  Words go in and come out in Montgomery form (a word w stands for w / 2^32 mod p),
as numpy uint32 arrays laid out as the C ABI lays them out (include/r0hip.h, oracle/orc.h):
  evaluate     natural-order base-field coefficients, one extension point
  mix_poly     combos: extension elements, array of structs [combo][i]; input: base-field columns [c][i]
  sum_extelem  in: array of structs [count][n]; out: four columns [4][n]
  fri_fold     in: four columns [4][16 n_out], coefficients in bit-reversed order; out: four columns [4][n_out]
  poly_divide  array of structs, coefficients low to high
and of steps 5 and 6 as the device-challenge forms compute them: pow4, deep_points, interpolate, deep_heads, divide_batch (below).
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


# ---- steps 5 and 6 of a proof as the device-challenge forms compute them (include/r0hip.h, beside r0h_ext_powers_buf).  The functions
# above take and return words; the ones below with a leading underscore work on canonical 4-tuples.
CHECK_SIZE = 16


def sub4(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def _pow4(b, e):
    r = ONE4  # the empty product: x^0 = 1 for every x, zero included
    while e:
        if e & 1:
            r = mul4(r, b)
        b = mul4(b, b)
        e >>= 1
    return r


def _inv4(a):
    """a^(p^4 - 2): the multiplicative group of Fp4 has p^4 - 1 elements"""
    assert a != ZERO4
    return _pow4(a, P**4 - 2)


def pow4(base, e):
    """base^e: 4 words"""
    return enc(_pow4(tuple(dec(base)), int(e)))


def deep_points(z, wpow):
    """z * wpow[i] for every base-field word of wpow, then z^4: 4 words each"""
    zz = tuple(dec(z))
    return _flat([scale4(zz, w) for w in dec(wpow)] + [_pow4(zz, 4)])


def interpolate(xs, ys):
    """Lagrange: the coefficients, low to high, of the polynomial of degree < n through (xs[i], ys[i]); the xs distinct"""
    xs, ys = _ext(dec(xs)), _ext(dec(ys))
    n = len(xs)
    acc = [ZERO4] * n
    for i in range(n):
        num, den = [ONE4], ONE4  # prod_{j != i} (x - xs[j]), low to high, and its value at xs[i]
        for j in range(n):
            if j == i:
                continue
            neg = sub4(ZERO4, xs[j])
            num = [add4(mul4(neg, num[k]) if k < len(num) else ZERO4, num[k - 1] if k else ZERO4) for k in range(len(num) + 1)]
            den = mul4(den, sub4(xs[i], xs[j]))
        s = mul4(ys[i], _inv4(den))
        acc = [add4(a, mul4(c, s)) for a, c in zip(acc, num)]
    return _flat(acc)


def evaluate4(coeff_words, x_words):
    """sum_i c[i] x^i for extension coefficients, low to high: 4 words"""
    x, tot = tuple(dec(x_words)), ZERO4
    for c in reversed(_ext(dec(coeff_words))):
        tot = add4(mul4(tot, x), c)
    return enc(tot)


def deep_heads(coeff_u, regs, n_taps, n_combos, mix):
    """What the head fix-up takes off the combos: {(combo, i): 4-tuple}.  regs: (combo, first tap, taps) in order; a running power of
    the mix per register, then one per CHECK column; CHECK's columns all land on coefficient 0 of combo n_combos."""
    u, m = _ext(dec(coeff_u)), tuple(dec(mix))
    assert len(u) == n_taps + CHECK_SIZE
    heads, cur = {}, ONE4
    for combo, first, size in regs:
        for i in range(size):
            heads[(combo, i)] = add4(heads.get((combo, i), ZERO4), mul4(cur, u[first + i]))
        cur = mul4(cur, m)
    for j in range(CHECK_SIZE):
        heads[(n_combos, 0)] = add4(heads.get((n_combos, 0), ZERO4), mul4(cur, u[n_taps + j]))
        cur = mul4(cur, m)
    return heads


def subtract_heads(combo_words, po2, heads):
    """the combos ([combo][2^po2] extension elements) less deep_heads' values"""
    combos = _ext(dec(combo_words))
    for (combo, i), h in heads.items():
        at = (combo << po2) + i
        combos[at] = sub4(combos[at], h)
    return _flat(combos)


def divide_batch(polys, n, jobs):
    """poly_divide job by job in the order given: jobs = [(polynomial, z words)], polys = [polynomial][n] extension elements
    -> (the polynomials after all divisions, the remainders, 4 words per job)"""
    polys = np.array(polys, dtype=np.uint32)
    rems = []
    for k, z in jobs:
        q, r = poly_divide(polys[4 * n * k:4 * n * (k + 1)], z)
        polys[4 * n * k:4 * n * (k + 1)] = q
        rems.append(r)
    return polys, (np.concatenate(rems) if rems else np.zeros(0, np.uint32))


def poly_mul_linear(words, z):
    """p(x) * (x - z), one coefficient longer"""
    p, zz = _ext(dec(words)), tuple(dec(z))
    out = [ZERO4] * (len(p) + 1)
    for i, c in enumerate(p):
        out[i + 1] = add4(out[i + 1], c)
        out[i] = sub4(out[i], mul4(c, zz))
    return _flat(out)
