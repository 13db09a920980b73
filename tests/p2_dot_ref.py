"""The correction schedule of the Poseidon2 partial rounds' dot products (csrc/poseidon2_dot_schedule.hpp) and the permutation
itself, restated in Python integers / numpy for the tests: tables as fill_p2 (csrc/poseidon2_host.cpp) lays them out, the rule that derives the
masks, the walk that decides whether a schedule covers a table, and the sponge over any table (the oracle has no setter for its own)."""
import os
import re

import numpy as np

P = 2013265921
CELLS, RATE, HALF_FULL, PARTIAL = 24, 16, 4, 21
SIGMA_ROWS, ROWS, END = PARTIAL - 1, PARTIAL - 1 + CELLS - 1, 63
FIX_LIMIT, FIXED, END_LIMIT = (2 * P) << 32, (P << 32) - 1, 4 * P * P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_tables():
    """(round constants [29 * 24], diagonal minus one [24]): the canonical words of include/r0hip_poseidon2_consts.h"""
    text = open(os.path.join(ROOT, "include", "r0hip_poseidon2_consts.h")).read()
    out = []
    for name in ("R0H_P2_ROUND_CONSTANTS", "R0H_P2_INT_DIAG_M1"):
        body = re.search(name + r"\[[^\]]*\] = \{(.*?)\};", text, re.S).group(1)
        out.append([int(w, 16) for w in re.findall(r"0x([0-9a-f]{8})u", body)])
    assert len(out[0]) == CELLS * (2 * HALF_FULL + PARTIAL) and len(out[1]) == CELLS
    return out[0], out[1]


def enc(x):
    return (x << 32) % P


def dot_rows(diag_m1):
    """the constant words of the 43 dot products in evaluation order: part_sigma's rows for rounds 1..20, part_final's for lanes 1..23"""
    pw = [[pow(d, e, P) for d in diag_m1] for e in range(PARTIAL + 1)]
    kappa = [sum(pw[e][1:]) % P for e in range(PARTIAL + 1)]
    rows = [[enc(pw[r][i]) for i in range(1, CELLS)] + [enc(kappa[r - 1 - j]) for j in range(r)] for r in range(1, PARTIAL)]
    rows += [[enc(pw[e][i]) for e in range(PARTIAL, -1, -1)] for i in range(1, CELLS)]
    assert [len(r) for r in rows] == [CELLS + r for r in range(SIGMA_ROWS)] + [PARTIAL + 1] * (CELLS - 1)
    return rows


def schedule(rows):
    """the rule: an exact bound on the accumulator with every operand at p - 1; correct before a term that could take it to 2p 2^32,
    and at the end if it could have reached 4 p^2"""
    masks = []
    for k in rows:
        mask, bound = 0, (P - 1) * k[0]
        for i in range(1, len(k)):
            if bound + (P - 1) * k[i] >= FIX_LIMIT:
                mask |= 1 << i
                bound = FIXED
            bound += (P - 1) * k[i]
        if bound >= END_LIMIT:
            mask |= 1 << END
        masks.append(mask)
    return masks


def safe_schedule():
    return [sum(1 << i for i in range(4, n, 2)) | 1 << END for n in [CELLS + r for r in range(SIGMA_ROWS)] + [PARTIAL + 1] * (CELLS - 1)]


def corrections(masks):
    return sum(bin(m).count("1") for m in masks)


def covers(masks, rows):
    """whether every bound holds when `rows` is walked under `masks`: below 2^64 always, below 2p 2^32 at each correction, below 4 p^2
    at the finish"""
    for mask, k in zip(masks, rows):
        bound = 0
        for i, w in enumerate(k):
            if i and mask >> i & 1:
                if bound >= FIX_LIMIT:
                    return False
                bound = min(bound, FIXED)
            bound += (P - 1) * w
            if bound >> 64:
                return False
        if mask >> END & 1:
            if bound >= FIX_LIMIT:
                return False
            bound = min(bound, FIXED)
        if bound >= END_LIMIT:
            return False
    return True


# ---- the permutation over any table, vectorised over states: canonical values in uint64 (products stay below 2^62)
_RINV = pow(1 << 32, -1, P)


def _m_ext(c):
    col = np.zeros((c.shape[0], 4), np.uint64)
    for k in range(0, CELLS, 4):
        a, b, d, e = (c[:, k + j].copy() for j in range(4))
        t0, t1 = (a + b) % P, (d + e) % P
        t2, t3 = (2 * b + t1) % P, (2 * e + t0) % P
        t4, t5 = (4 * t1 + t3) % P, (4 * t0 + t2) % P
        c[:, k], c[:, k + 1], c[:, k + 2], c[:, k + 3] = (t3 + t5) % P, t5, (t2 + t4) % P, t4
        col = (col + c[:, k:k + 4]) % P
    for k in range(0, CELLS, 4):
        c[:, k:k + 4] = (c[:, k:k + 4] + col) % P


def _sbox(x):
    x2 = x * x % P
    x4 = x2 * x2 % P
    return x4 * x2 % P * x % P


def mix(cells, rc, diag_m1):
    """the permutation of an [n, 24] array of Montgomery words under the table (rc, diag_m1) of canonical words"""
    c = cells.astype(np.uint64) * np.uint64(_RINV) % np.uint64(P)
    rc = np.asarray(rc, np.uint64).reshape(2 * HALF_FULL + PARTIAL, CELLS)
    diag = np.asarray(diag_m1, np.uint64)
    _m_ext(c)
    for r in range(2 * HALF_FULL + PARTIAL):
        if r < HALF_FULL or r >= HALF_FULL + PARTIAL:
            c = _sbox((c + rc[r]) % P)
            _m_ext(c)
        else:
            c[:, 0] = _sbox((c[:, 0] + rc[r, 0]) % P)
            c = (c.sum(axis=1, keepdims=True) + c * diag) % P
    return ((c << np.uint64(32)) % np.uint64(P)).astype(np.uint32)


def hash_rows(matrix, rows, cols, rc, diag_m1):
    m = np.asarray(matrix, np.uint32).reshape(cols, rows)
    st = np.zeros((rows, CELLS), np.uint32)
    for blk in range(max(1, (cols + RATE - 1) // RATE)):
        part = m[blk * RATE:(blk + 1) * RATE].T
        st[:, :RATE] = 0
        st[:, :part.shape[1]] = part
        st = mix(st, rc, diag_m1)
    return st[:, :8].reshape(-1).copy()


def hash_fold(nodes, output_size, rc, diag_m1):
    out = np.asarray(nodes, np.uint32).copy().reshape(-1, 8)
    st = np.zeros((output_size, CELLS), np.uint32)
    st[:, :16] = out[2 * output_size:4 * output_size].reshape(output_size, 16)
    out[output_size:2 * output_size] = mix(st, rc, diag_m1)[:, :8]
    return out.reshape(-1)
