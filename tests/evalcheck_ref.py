"""Plain reference of r0h_eval_check, written from the blob format (include/r0hip_circuit.h) alone: it shares the flattening of the
PolyExtStep program with check_ref.Program and nothing with the library's emitter or the oracle's C.

  check[i] = (sum_t poly_mix^t * val_t(i)) / ((3 w^i)^N - 1)        i in [0, 4N), w = 137^(2^27 / 4N) the 4N-th root of unity

Term t is the t-th AndEqz once AndCond gates are flattened (its value times its gates), poly_mix^t is taken in
F_p[x] / (x^4 - 11), a tap (group, column, back) is the group's evaluation column at row (i - 4 back) mod 4N, and the four
components of check come out as four columns [4][4N].  All arithmetic is canonical (uint64 numpy columns, Python ints for the
scalars); words are Montgomery form (x 2^32 mod p) on the way in and out.  For 4N up to a few thousand."""
import numpy as np

from check_ref import OP_ADD, OP_CONST, OP_GET, OP_GET_GLOBAL, OP_MUL, OP_SUB, P, R_INV, Program

R = (1 << 32) % P
BETA = 11
ROU_GEN, ROU_PO2 = 137, 27  # 137 has order 2^27 in F_p


def _mul4(a, b):
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return [(c[0] + BETA * c[4]) % P, (c[1] + BETA * c[5]) % P, (c[2] + BETA * c[6]) % P, c[3] % P]


def eval_check(blob, po2, ea, ec, ed, glob, mix, poly_mix):
    pr = Program(blob)
    n, domain = 1 << po2, 4 << po2
    p64 = np.uint64(P)

    def columns(words, count):
        return (np.asarray(words, dtype=np.uint32).reshape(count, domain).astype(np.uint64) * np.uint64(R_INV)) % p64

    groups = [columns(w, pr.group_size[g]) for g, w in enumerate((ea, ec, ed))]
    scalars = [[int(x) * R_INV % P for x in glob], [int(x) * R_INV % P for x in mix]]
    vals = []
    for op, a, b, _ in pr.fp:
        if op == OP_CONST:
            r = np.full(domain, a % P, dtype=np.uint64)
        elif op == OP_GET:
            g, col, back = pr.taps[a]
            r = np.roll(groups[g][col], 4 * back)  # r[i] = column[(i - 4 back) mod 4N]
        elif op == OP_GET_GLOBAL:
            r = np.full(domain, scalars[a][b], dtype=np.uint64)
        else:
            x, y = vals[a], vals[b]
            assert op in (OP_ADD, OP_SUB, OP_MUL)
            r = (x + y) % p64 if op == OP_ADD else (x + p64 - y) % p64 if op == OP_SUB else (x * y) % p64
        vals.append(r)
    tot = [np.zeros(domain, dtype=np.uint64) for _ in range(4)]
    power = [1, 0, 0, 0]
    pm = [int(x) * R_INV % P for x in poly_mix]
    for v, gates in pr.terms:
        w = vals[v]
        for g in gates:
            w = (w * vals[g]) % p64
        for q in range(4):
            tot[q] = (tot[q] + w * np.uint64(power[q])) % p64
        power = _mul4(power, pm)
    root = pow(ROU_GEN, 1 << (ROU_PO2 - po2 - 2), P)
    inv_van = np.array([pow((pow(3 * pow(root, i, P) % P, n, P) - 1) % P, P - 2, P) for i in range(domain)], dtype=np.uint64)
    out = [(((t * inv_van) % p64) * np.uint64(R)) % p64 for t in tot]
    return np.concatenate(out).astype(np.uint32)
