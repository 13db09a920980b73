"""The partial rounds' dot products correct their accumulators on a schedule derived from the compiled-in diagonal (258 conditional
subtractions per permutation instead of 550, csrc/poseidon2_dot_schedule.hpp); a table that schedule does not cover is hashed by the
kernels of the safe one.  Word for word, no tolerance: the default table against the CPU oracle at shapes that give many distinct
partial-round entries (random words and the all-(p-1) matrix, one to three sponge blocks, both fold kernels, a whole tree), and two
other diagonals -- one the tight schedule does not cover, one it does -- against the Python restatement of tests/p2_dot_ref.py, which is
itself held to the oracle under the default table first."""
import numpy as np
import pytest

import p2_dot_ref as ref

pytestmark = pytest.mark.gpu
P = ref.P
RC, DIAG = ref.header_tables()
# (that the tight schedule covers the one and not the other: tests/test_p2_dot_schedule.py, without a GPU)
# every D_i = -1: the table's words are enc(1) and enc(-1) = 0.87 p in turn, and whole rows of the latter overrun the tight schedule
UNCOVERED = [P - 1] * ref.CELLS
# D_0 halved: another permutation (lane 0's product with D_0 is in every partial round), the same dot-product tables -- they hold the
# powers of D_1..D_23 and their sums.  (The schedule leaves little slack: no single changed word among D_1..D_23 out of 3,000 random
# ones, nor 0, 1, 2, 3, 4, p - 1 or the halved word in any lane, keeps a table covered.)
COVERED = [DIAG[0] // 2] + DIAG[1:]


def words(seed, n):
    return np.full(n, P - 1, np.uint32) if seed is None else np.random.default_rng(seed).integers(0, P, size=n, dtype=np.uint32)


def gpu_hash_rows(hal, m, rows, cols):
    dig = hal.alloc(rows * 8)
    hal.zero(dig)
    hal.hash_rows(dig, hal.copy_from(m), rows, cols)
    return dig.to_host()


def gpu_hash_fold(hal, lvl, output_size):
    nb = hal.copy_from(lvl)
    hal.hash_fold(nb, output_size)
    return nb.to_host()


@pytest.mark.parametrize("cols", (16, 17, 40, 48))
def test_default_table_hash_rows(hal, orc, cols):
    assert hal.poseidon2_dot_schedule() == "tight"
    rows = 4096
    for seed in (11, 12, 13, None):
        m = words(None if seed is None else 100 * seed + cols, rows * cols)
        assert np.array_equal(gpu_hash_rows(hal, m, rows, cols), orc.hash_rows(m, rows, cols)), (cols, seed)


@pytest.mark.parametrize("output_size", (16384, 1))
def test_default_table_hash_fold(hal, orc, output_size):
    for seed in (21, None):
        lvl = words(seed, output_size * 4 * 8)
        assert np.array_equal(gpu_hash_fold(hal, lvl, output_size), orc.hash_fold(lvl, output_size)), seed


def test_default_table_merkle_build(hal, orc):
    rows, cols = 32768, 40
    m = words(31, rows * cols)
    nodes = hal.alloc(rows * 2 * 8)
    hal.zero(nodes)
    hal.merkle_build(nodes, hal.copy_from(m), rows, cols)
    assert np.array_equal(nodes.to_host()[8:], orc.merkle_build(m, rows, cols)[8:])


ROW_SHAPES = ((65, 17), (257, 40))
FOLD_SIZES = (2, 16384)


def check_against_the_restatement(hal, diag, orc=None):
    """hash_rows and hash_fold under the table the context holds, which is (RC, diag); against the oracle too where one is given"""
    for rows, cols in ROW_SHAPES:
        for seed in (41, None):
            m = words(seed, rows * cols)
            want = ref.hash_rows(m, rows, cols, RC, diag)
            if orc is not None:
                assert np.array_equal(want, orc.hash_rows(m, rows, cols)), "the restatement differs from the oracle"
            assert np.array_equal(gpu_hash_rows(hal, m, rows, cols), want), (rows, cols, seed)
    for output_size in FOLD_SIZES:
        for seed in (42, None):
            lvl = words(seed, output_size * 4 * 8)
            want = ref.hash_fold(lvl, output_size, RC, diag)
            if orc is not None:
                assert np.array_equal(want, orc.hash_fold(lvl, output_size)), "the restatement differs from the oracle"
            assert np.array_equal(gpu_hash_fold(hal, lvl, output_size), want), (output_size, seed)


@pytest.mark.parametrize("diag,schedule", ((UNCOVERED, "safe"), (COVERED, "tight")), ids=("uncovered", "covered"))
def test_another_diagonal_takes_the_kernels_its_table_allows(hal, orc, diag, schedule):
    assert hal.poseidon2_dot_schedule() == "tight"
    check_against_the_restatement(hal, DIAG, orc)  # the restatement itself, and the device, under the default table
    m = words(43, 65 * 17)
    default_digests = gpu_hash_rows(hal, m, 65, 17)
    try:
        hal.poseidon2_set_consts(np.array(RC, np.uint32), np.array(diag, np.uint32))
        assert hal.poseidon2_dot_schedule() == schedule
        assert not np.array_equal(gpu_hash_rows(hal, m, 65, 17), default_digests)
        check_against_the_restatement(hal, diag)
    finally:
        hal.poseidon2_set_consts(np.array(RC, np.uint32), np.array(DIAG, np.uint32))
    assert hal.poseidon2_dot_schedule() == "tight"
    assert np.array_equal(gpu_hash_rows(hal, m, 65, 17), default_digests)
    assert np.array_equal(default_digests, orc.hash_rows(m, 65, 17))
