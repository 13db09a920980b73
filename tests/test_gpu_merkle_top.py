"""A tree kept as its top (r0h_merkle_top) and openings made from matrix and top (r0h_merkle_open_top), under both hash suites, held word
for word against tests/merkle_top_ref.py over the node array Hal.merkle_build leaves.

Shapes: rows 2^6, 2^7 (path_digests 1 and 2: only levels = 1 fits) and 2^11 (6: levels 1 and 6, the default, one wave per query); 2^13
besides, the smallest tree that admits levels = 8 (four waves per query, the rounds cross waves).  cols 1, 15, 16, 17 (one rate
block short, full, one over) and 128.  Queries: row 0, the last row, two rows of one subtree, one row twice; one query and fifty."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import merkle_top_ref as ref

pytestmark = pytest.mark.gpu
P = 15 * (1 << 27) + 1
COLS = (1, 15, 16, 17, 128)
SHAPES = [(1 << 6, 1), (1 << 7, 1), (1 << 11, 1), (1 << 11, 6), (1 << 13, 8)]


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
    """a matrix, its device copy, its tree on the device and on the host"""
    m = np.random.default_rng(seed).integers(0, P, size=(cols, rows), dtype=np.uint32)
    matrix, nodes = h.alloc(rows * cols), h.alloc(2 * rows * 8)
    matrix.upload(m)
    h.merkle_build(nodes, matrix, rows, cols)
    return m, matrix, nodes, nodes.to_host().reshape(2 * rows, 8)


def queries(rows, levels, n_q, seed):
    if n_q == 1:
        return np.array([rows - 1], dtype=np.uint32)
    span = 1 << levels
    fixed = [0, rows - 1, 5 * span % rows, 5 * span % rows + span - 1, rows // 2 + 1, rows // 2 + 1]  # ends, two of one subtree, one twice
    rest = np.random.default_rng(seed).integers(0, rows, size=n_q - len(fixed))
    return np.concatenate([fixed, rest]).astype(np.uint32)


def open_top(h, matrix, top, levels, idx, rows, cols):
    out = h.alloc(len(idx) * ref.opening_words(rows, cols))
    try:
        h.merkle_open_top(out, matrix, top, levels, idx, rows, cols)
        return out.to_host().reshape(len(idx), -1)
    finally:
        out.free()


@pytest.mark.parametrize("rows,levels", SHAPES)
def test_openings_from_the_top_are_the_full_trees(ctx, rows, levels):
    assert levels <= min(ref.MAX_TOP_LEVELS, ref.path_digests(rows))
    for cols in COLS:
        m, matrix, nodes, host_nodes = committed(ctx, rows, cols, 1000 * rows + cols)
        top = ctx.merkle_top(nodes, rows, levels)
        assert top.words == 8 * ref.top_digests(rows, levels)
        assert np.array_equal(top.to_host()[8:], host_nodes[1:ref.top_digests(rows, levels)].ravel())
        nodes.free()  # the openings below have the matrix and the top, nothing else
        for n_q in (1, 50):
            idx = queries(rows, levels, n_q, cols)
            got = open_top(ctx, matrix, top, levels, idx, rows, cols)
            assert np.array_equal(got, ref.openings(m, host_nodes, idx)), (rows, cols, levels, n_q)
        matrix.free(); top.free()


@pytest.mark.parametrize("rows,levels", [(1 << 7, 1), (1 << 11, 6)])
def test_a_top_of_another_matrix_is_named_at_the_first_query_it_shows_at(ctx, rows, levels):
    """the other matrix differs in the last row alone: every subtree but the last still hashes to the other top's node.  Query 2 is the
    first under the last subtree; the call after it, with the right top, succeeds on the same context."""
    cols = 17
    m, matrix, nodes, host_nodes = committed(ctx, rows, cols, 7)
    other = m.copy()
    other[3, rows - 1] ^= 1
    other_matrix, other_nodes = ctx.alloc(rows * cols), ctx.alloc(2 * rows * 8)
    other_matrix.upload(other)
    ctx.merkle_build(other_nodes, other_matrix, rows, cols)
    top, other_top = ctx.merkle_top(nodes, rows, levels), ctx.merkle_top(other_nodes, rows, levels)
    idx = np.array([0, rows // 2, rows - 2, 1, rows - 1], dtype=np.uint32)
    with pytest.raises(r0.R0HipError, match=r"r0h_merkle_open_top: tree top does not match the matrix under query 2 \(row %d\)" % (rows - 2)):
        open_top(ctx, matrix, other_top, levels, idx, rows, cols)
    with pytest.raises(r0.R0HipError, match=r"tree top does not match the matrix under query 0 \(row %d\)$" % (rows - 1)):
        open_top(ctx, matrix, other_top, levels, idx[4:], rows, cols)
    assert np.array_equal(open_top(ctx, matrix, top, levels, idx, rows, cols), ref.openings(m, host_nodes, idx))
    assert np.array_equal(open_top(ctx, other_matrix, other_top, levels, idx, rows, cols), ref.openings(other, other_nodes.to_host(), idx))
    for b in (matrix, nodes, other_matrix, other_nodes, top, other_top):
        b.free()


def test_levels_and_rows_outside_their_bounds_are_refused_by_name(ctx):
    rows, cols = 1 << 11, 16
    m, matrix, nodes, _ = committed(ctx, rows, cols, 3)
    assert ref.path_digests(rows) == 6 and ref.path_digests(1 << 13) == 8
    top, out, idx = ctx.alloc(2 * rows * 8), ctx.alloc(50 * ref.opening_words(rows, cols)), np.array([1], dtype=np.uint32)
    for levels, bound in ((0, 6), (7, 6), (9, 6)):
        with pytest.raises(r0.R0HipError, match=r"r0h_merkle_top: levels %d outside \[1, %d\]" % (levels, bound)):
            ctx.merkle_top(nodes, rows, levels, top)
        with pytest.raises(r0.R0HipError, match=r"r0h_merkle_open_top: levels %d outside \[1, %d\]" % (levels, bound)):
            ctx.merkle_open_top(out, matrix, top, levels, idx, rows, cols)
    big = ctx.alloc(2 * (1 << 13) * 8)
    with pytest.raises(r0.R0HipError, match=r"r0h_merkle_top: levels 9 outside \[1, 8\]"):  # eight is the most, whatever the tree
        ctx.merkle_top(big, 1 << 13, 9, top)
    with pytest.raises(r0.R0HipError, match=r"r0h_merkle_top: levels 2 outside \[1, 1\]"):
        ctx.merkle_top(nodes, 1 << 6, 2, top)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_top: rows 2047 is not a power of two"):
        ctx.merkle_top(nodes, rows - 1, 1, top)
    ctx.merkle_top(nodes, rows, 6, top)
    for bad in (rows, rows + 5, 0xFFFFFFFF):
        with pytest.raises(r0.R0HipError, match=r"r0h_merkle_open_top: query 1 opens row %d of a 2048-row tree" % bad):
            ctx.merkle_open_top(out, matrix, top, 6, np.array([0, bad, 1], dtype=np.uint32), rows, cols)
    small = ctx.alloc(8 * ref.top_digests(rows, 6) - 8)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_top: the top of a 2048-row tree at 6 levels is 2048 bytes, the output buffer holds 2016"):
        ctx.merkle_top(nodes, rows, 6, small)
    with pytest.raises(r0.R0HipError, match="r0h_merkle_open_top: the top of a 2048-row tree at 6 levels is 2048 bytes, the buffer holds 2016"):
        ctx.merkle_open_top(out, matrix, small, 6, idx, rows, cols)
    assert np.array_equal(open_top(ctx, matrix, top, 6, idx, rows, cols), ref.openings(m, nodes.to_host(), idx))  # and the context goes on
    for b in (matrix, nodes, top, out, big, small):
        b.free()
