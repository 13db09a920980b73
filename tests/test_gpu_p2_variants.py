"""The Poseidon2 kernels take shorter linear layers at a hash's ends -- a first block enters with a zero capacity, only the
digest is read from a last block -- and hash_rows runs every block through one body that picks them per block.  Word for word
against the CPU oracle at the shapes where that choice changes: no block, a lone partial block, exactly one block (first and
last at once), first + last, first + middle + partial last; rows below, at and above a wave and past one workgroup; fold levels
on both sides of the 8,192-parent switch between the two fold kernels.  Integer arithmetic throughout: no tolerance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921
ROWS = (1, 63, 64, 65, 257)
COLS = (0, 1, 15, 16, 17, 32, 40, 48)
FOLD_SIZES = (1, 2, 8192, 16384)
KINDS = ("random", "zero", "p-1")


def words(kind, n, seed):
    if kind == "zero":
        return np.zeros(n, np.uint32)
    if kind == "p-1":
        return np.full(n, P - 1, np.uint32)
    return np.random.default_rng(seed).integers(0, P, size=n, dtype=np.uint32)


@pytest.mark.parametrize("cols", COLS)
def test_hash_rows_at_the_block_shapes(hal, orc, cols):
    for rows in ROWS:
        for kind in KINDS:
            m = words(kind, rows * cols, 1000 * rows + cols)
            dig = hal.alloc(rows * 8)
            hal.zero(dig)
            hal.hash_rows(dig, hal.copy_from(m) if m.size else hal.alloc(4), rows, cols)
            assert np.array_equal(dig.to_host(), orc.hash_rows(m, rows, cols)), (rows, cols, kind)


@pytest.mark.parametrize("output_size", FOLD_SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_hash_fold_on_both_sides_of_the_switch(hal, orc, output_size, kind):
    lvl = words(kind, output_size * 4 * 8, output_size)
    nb = hal.copy_from(lvl)
    hal.hash_fold(nb, output_size)
    assert np.array_equal(nb.to_host(), orc.hash_fold(lvl, output_size))


@pytest.mark.parametrize("output_size", FOLD_SIZES)
def test_merkle_build_whose_first_fold_has_this_size(hal, orc, output_size):
    rows = 2 * output_size
    for cols, kind in ((0, "random"), (16, "random"), (17, "random"), (40, "zero"), (40, "p-1")):
        m = words(kind, rows * cols, rows + cols)
        nodes = hal.alloc(rows * 2 * 8)
        hal.zero(nodes)
        hal.merkle_build(nodes, hal.copy_from(m) if m.size else hal.alloc(4), rows, cols)
        assert np.array_equal(nodes.to_host()[8:], orc.merkle_build(m, rows, cols)[8:]), (rows, cols, kind)
