"""r0h_merkle_climb: packed openings hashed from the row up to the layer a seal carries, under both hash suites.  Trees are built
with Hal.merkle_build and opened with the existing opening path (Hal.merkle_open_top where a tree has a path, and the node array read
by tests/merkle_top_ref.py, which the former is held to); what the kernel reaches must be nodes[(idx + rows) >> path_digests], and the
same digest recomputed independently with hash_elems_host / hash_pair_host.

Shapes: cols 1, 15, 16, 17, 33 (under, at and over one and two rate blocks); rows 32 and 64 (the layer a seal carries is the one above
the leaves: path_digests 1, on either side of a 50-node layer) and 2^11 (6); 1, 50 and 65 queries (one lane, one partial wave, a second
wave) with rows 0 and rows - 1 among them.  path_digests 0 -- the leaf digest is what is reached -- is what MerkleShape gives a
one-row tree and no other, so that case is a one-row "tree" held to hash_elems_host alone."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import merkle_top_ref as ref

pytestmark = pytest.mark.gpu
P = 15 * (1 << 27) + 1
COLS = (1, 15, 16, 17, 33)
ROWS = (32, 64, 1 << 11)


@pytest.fixture(scope="module")
def sha():
    h = r0.Hal(0)
    h.set_hashfn("sha-256")
    yield h
    h.close()


@pytest.fixture(params=["poseidon2", "sha-256"])
def ctx(request, hal):
    return hal if request.param == "poseidon2" else request.getfixturevalue("sha")


def committed(h, rows, cols, seed):
    m = np.random.default_rng(seed).integers(0, P, size=(cols, rows), dtype=np.uint32)
    matrix, nodes = h.alloc(rows * cols), h.alloc(2 * rows * 8)
    matrix.upload(m)
    h.merkle_build(nodes, matrix, rows, cols)
    return m, matrix, nodes, nodes.to_host().reshape(2 * rows, 8)


def queries(rows, n_q, seed):
    if n_q == 1:
        return np.array([rows - 1], dtype=np.uint32)
    rest = np.random.default_rng(seed).integers(0, rows, size=n_q - 3)
    return np.concatenate([[0, rows - 1, rows // 2 + 1], rest]).astype(np.uint32)


def packed(h, m, matrix, nodes, host_nodes, idx, rows, cols):
    """the openings as the existing opening path packs them, in a device buffer"""
    want = ref.openings(m, host_nodes, idx)
    out = h.alloc(want.size)
    top = h.merkle_top(nodes, rows, 1)
    h.merkle_open_top(out, matrix, top, 1, idx, rows, cols)
    top.free()
    assert np.array_equal(out.to_host().reshape(want.shape), want)
    return out, want


def by_hand(suite, opening, row, cols, path):
    cur = r0.hash_elems_host(suite, opening[:cols])
    for l in range(path):
        sib = opening[cols + 8 * l:cols + 8 * l + 8]
        cur = r0.hash_pair_host(suite, sib, cur) if (row >> l) & 1 else r0.hash_pair_host(suite, cur, sib)
    return cur


@pytest.mark.parametrize("rows", ROWS)
def test_the_climb_reaches_the_trees_own_node(ctx, rows):
    path = ref.path_digests(rows)
    assert path == {32: 1, 64: 1, 1 << 11: 6}[rows]
    for cols in COLS:
        m, matrix, nodes, host_nodes = committed(ctx, rows, cols, 77 * rows + cols)
        for n_q in (1, 50, 65):
            idx = queries(rows, n_q, cols + n_q)
            out, want = packed(ctx, m, matrix, nodes, host_nodes, idx, rows, cols)
            got = ctx.merkle_climb(out, idx, rows, cols)
            assert got.shape == (n_q, 8)
            assert np.array_equal(got, host_nodes[(idx.astype(np.int64) + rows) >> path]), (rows, cols, n_q)
            if n_q == 50:  # the same digests, recomputed without the tree
                for q in (0, 1, 2, 49):
                    assert np.array_equal(got[q], by_hand(ctx.hashfn, want[q], int(idx[q]), cols, path)), (rows, cols, q)
            out.free()
        matrix.free(); nodes.free()


def test_with_no_path_digests_the_leaf_digest_is_what_is_reached(ctx):
    assert ref.path_digests(1) == 0
    for cols in COLS:
        values = np.random.default_rng(cols).integers(0, P, size=(3, cols), dtype=np.uint32)
        out = ctx.copy_from(values.ravel())
        got = ctx.merkle_climb(out, np.zeros(3, dtype=np.uint32), 1, cols)
        for q in range(3):
            assert np.array_equal(got[q], r0.hash_elems_host(ctx.hashfn, values[q])), (cols, q)
        out.free()


def test_one_flipped_value_word_changes_exactly_that_querys_digest(ctx):
    rows, cols, path = 1 << 11, 17, 6
    m, matrix, nodes, host_nodes = committed(ctx, rows, cols, 5)
    idx = queries(rows, 50, 9)
    out, want = packed(ctx, m, matrix, nodes, host_nodes, idx, rows, cols)
    good = ctx.merkle_climb(out, idx, rows, cols)
    bad = want.copy()
    bad[31, 16] ^= 1  # the last value of query 31: the padded rate block's only word
    out.upload(bad.ravel())
    got = ctx.merkle_climb(out, idx, rows, cols)
    differs = np.any(got != good, axis=1)
    assert differs[31] and differs.sum() == 1
    assert np.array_equal(got[31], by_hand(ctx.hashfn, bad[31], int(idx[31]), cols, path))
    for b in (out, matrix, nodes):
        b.free()


def test_a_row_outside_the_tree_is_an_error_that_names_the_bound(ctx):
    rows, cols = 64, 16
    out = ctx.alloc(3 * ref.opening_words(rows, cols))
    for bad in (rows, 0xFFFFFFFF):
        with pytest.raises(r0.R0HipError, match=r"r0h_merkle_climb: query 1 opens row %d of a 64-row tree" % bad):
            ctx.merkle_climb(out, np.array([0, bad, 1], dtype=np.uint32), rows, cols)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_climb: rows 63 is not a power of two"):
        ctx.merkle_climb(out, np.array([0], dtype=np.uint32), 63, cols)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_climb: cols 0: an opening holds at least one value"):
        ctx.merkle_climb(out, np.array([0], dtype=np.uint32), rows, 0)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_climb: 4 openings of 24 words exceed the buffer"):
        ctx.merkle_climb(out, np.array([0, 1, 2, 3], dtype=np.uint32), rows, cols)
    assert ctx.merkle_climb(out, np.zeros(0, dtype=np.uint32), rows, cols).shape == (0, 8)
    out.free()
