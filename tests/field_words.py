"""Operand families and corner points shared by the operation-level tests: BabyBear words in Montgomery form (R = 2^32 mod p).
Every word here is canonical (< p); what a family means to a kernel is the size of the products it feeds the lazy reductions."""
import numpy as np

P = 2013265921
ONE = (1 << 32) % P  # 268435454: the Montgomery word of 1

FAMILIES = ("random", "pool", "top")
POINT_KINDS = ("random", "top", "zero", "one")


def rnd(rng, n):
    return rng.integers(0, P, size=n, dtype=np.uint32)


def extreme(rng, n):
    """Words drawn from the corners of [0, p): the lazy-reduction bounds of the kernels are worst at p-1."""
    pool = np.array([0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**31 - 2**27, 0x0FFFFFFF, 0x70000000], dtype=np.uint32)
    return pool[rng.integers(0, pool.size, size=n)]


def family(rng, n, kind):
    """n words: `random` uniform in [0, p), `pool` from the corners, `top` every word p - 1"""
    if kind == "random":
        return rnd(rng, n)
    if kind == "pool":
        return extreme(rng, n)
    assert kind == "top"
    return np.full(n, P - 1, dtype=np.uint32)


def point(rng, kind):
    """an extension element, 4 words: a random canonical one, (p-1)^4, zero, or the Montgomery one"""
    if kind == "random":
        return rnd(rng, 4)
    return np.array({"top": [P - 1] * 4, "zero": [0] * 4, "one": [ONE, 0, 0, 0]}[kind], dtype=np.uint32)
