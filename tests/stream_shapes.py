"""Shapes and planned inputs shared by the operation-level tests of the DEEP-step streams (test_gpu_stream_edges.py: the host-challenge
forms; test_gpu_device_forms.py: the device-challenge forms; test_stream_ref_steps.py: what can be said of them without a GPU)."""
import numpy as np

import stream_ref as ref
from field_words import POINT_KINDS, point, rnd

GUARD = 0xA5A5A5A5  # no field word: above p

# (combo of each column, combos in the buffer): unsorted with gaps -- combos 1, 3 and 4 come back as they went in; one column; 70 in one.
# `gaps` is the layout whose combo_of is NOT sorted: mix_poly_coeffs sorts its columns to [1, 4, 0, 2, 3], so the k-th sorted column is
# not column k and a power table written in sorted order has to name the column's own exponent.
MIX_LAYOUTS = {"gaps": ([2, 0, 2, 5, 0], 6), "single": ([0], 1), "seventy": ([0] * 70, 1)}
UNSORTED_LAYOUT = "gaps"

# one element; two; fewer threads than a block; one block of one element per thread; two per thread; one full chunk; two chunks; 256
# chunks (one per thread of the link kernel); 512 (two per thread)
DIVIDE_SIZES = [1, 2, 128, 256, 512, 4096, 8192, 1 << 20, 1 << 21]

def distinct_points(rng, n):
    """n distinct extension points in a shuffled order: zero, one and (p-1)^4 among them from n = 4 on, the first n - 1 of those below"""
    pts = [point(rng, k) for k in ("zero", "one", "top")][:3 if n >= 4 else max(n - 1, 0)]
    while len(pts) < n:
        c = rnd(rng, 4)
        if not any(np.array_equal(c, q) for q in pts):
            pts.append(c)
    return np.concatenate([pts[i] for i in rng.permutation(n)])


# ---- job tables of the batched division: the polynomial of every job, in the order given
THREE_PASSES = [0, 1, 0, 2, 0, 2]  # launched as jobs 0 1 3 | 2 5 | 4: the third job given is the fourth launched
FRONT_LOADED = [0, 0, 0, 1, 2]     # launched as jobs 0 3 4 | 1 | 2


def launch_order(poly_idx):
    """the order poly_divide_batch launches its jobs in: pass k holds the k-th job of every polynomial"""
    seen, passes = {}, []
    for j, p in enumerate(poly_idx):
        k = seen.get(p, 0)
        seen[p] = k + 1
        if len(passes) <= k:
            passes.append([])
        passes[k].append(j)
    return [j for p in passes for j in p]


def divisible(rng, n, poly_idx, pt_idx, points):
    """[polynomial][n] extension coefficients (words): polynomial k = q_k(x) * prod over its jobs (x - point of the job), q_k random of
    the degree that fills n coefficients -- every division of the table leaves remainder zero"""
    n_polys = max(poly_idx) + 1
    pts = np.asarray(points, np.uint32).reshape(-1, 4)
    out = []
    for k in range(n_polys):
        mine = [pts[pt_idx[j]] for j in range(len(poly_idx)) if poly_idx[j] == k]
        assert len(mine) < n
        p = rnd(rng, 4 * (n - len(mine)))
        for z in mine:
            p = ref.poly_mul_linear(p, z)
        out.append(p)
    return np.concatenate(out)


def spoil(polys, n, poly_idx, pt_idx, points, j, delta):
    """`polys` (of divisible()) with delta * prod over the EARLIER jobs on job j's polynomial (x - their point) added to that polynomial:
    the earlier divisions stay exact, job j leaves remainder delta, and the quotient it hands on is what it was, so the later ones
    stay exact as well.  Exactly job j fails."""
    pts = np.asarray(points, np.uint32).reshape(-1, 4)
    k = poly_idx[j]
    add = np.asarray(delta, np.uint32)
    for i in range(j):
        if poly_idx[i] == k:
            add = ref.poly_mul_linear(add, pts[pt_idx[i]])
    out = polys.copy()
    head = ref.dec(out[4 * n * k:4 * n * k + add.size])
    out[4 * n * k:4 * n * k + add.size] = ref.enc([a + b for a, b in zip(head, ref.dec(add))])
    return out


LAST_WORD_ONLY = ref.enc([0, 0, 0, 1])  # a remainder whose only non-zero word is its last


def report_cases():
    """(name, n, poly_idx, pt_idx, points, polys, failing jobs): the inputs of the report-word tests.  Built once."""
    if _CASES:
        return _CASES
    rng = np.random.default_rng(4242)
    points = np.concatenate([point(rng, k) for k in POINT_KINDS] + [point(rng, "random")])  # random, (p-1)^4, zero, one, random
    delta = rnd(rng, 4)

    def add(name, n, poly_idx, pt_idx, fails, d=delta):
        polys = divisible(rng, n, poly_idx, pt_idx, points)
        for j in fails:
            polys = spoil(polys, n, poly_idx, pt_idx, points, j, d)
        _CASES.append((name, n, list(poly_idx), list(pt_idx), points, polys, sorted(fails)))

    for n_polys in (65, 130):  # one job each: the job table crosses 64 once, and twice
        idx, pt = list(range(n_polys)), [j % 5 for j in range(n_polys)]
        add("%d-all-divide" % n_polys, 16, idx, pt, [])
        for j in sorted({0, 63, 64, n_polys - 1}):
            add("%d-job-%d-fails" % (n_polys, j), 16, idx, pt, [j])
    add("130-last-word-only", 16, list(range(130)), [j % 5 for j in range(130)], [64], LAST_WORD_ONLY)
    add("one-job-last-word-only", 16, [0], [1], [0], LAST_WORD_ONLY)
    for table, name in ((THREE_PASSES, "three-passes"), (FRONT_LOADED, "front-loaded")):
        pt = [(3 * j + 1) % 5 for j in range(len(table))]
        add(name + "-all-divide", 32, table, pt, [])
        for j in range(len(table)):  # a report that names the launch position instead of the job is wrong for every job the passes move
            add("%s-job-%d-fails" % (name, j), 32, table, pt, [j])
    # two failures, the later one in the order given launched in the earlier pass
    add("three-passes-jobs-2-3-fail", 32, THREE_PASSES, [1, 0, 4, 2, 3, 0], [2, 3])
    add("three-passes-jobs-4-5-fail", 32, THREE_PASSES, [1, 0, 4, 2, 3, 0], [4, 5])
    add("front-loaded-jobs-1-4-fail", 32, FRONT_LOADED, [0, 0, 1, 2, 3], [1, 4])  # (also: one point twice on a polynomial)
    return _CASES


_CASES = []
