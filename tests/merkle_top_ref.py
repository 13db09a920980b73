"""Openings of a Merkle tree, from the full node array (numpy; normative for tests/test_gpu_merkle_top.py and what rests on it).

A tree over `rows` leaves is 2 * rows digests of 8 words: index 0 unused, the root at 1, node i the hash of nodes 2i and 2i + 1, the
leaf of row r at rows + r (r0h_merkle_build).  A seal carries layer `top_layer` of a tree instead of its root -- the deepest layer of at
most 50 nodes (one per query) -- so an opening is the row's `cols` values followed by the sibling digests from the leaf up to,
excluding, that layer: nodes[((row + rows) >> l) ^ 1] for l < path_digests.  Nothing here hashes: the expected values are read from
the node array that Hal.merkle_build left, never from the code that opens a tree from its top."""
import numpy as np

QUERIES = 50
MAX_TOP_LEVELS = 8


def path_digests(rows):
    layers = rows.bit_length() - 1
    assert rows == 1 << layers
    top_layer = 0
    for i in range(1, layers):
        if (1 << i) > QUERIES:
            break
        top_layer = i
    return layers - top_layer


def opening_words(rows, cols):
    return cols + 8 * path_digests(rows)


def top_digests(rows, levels):
    """how many digests the top of a tree holds when it is kept down to `levels` levels above the leaves"""
    return (2 * rows) >> levels


def openings(matrix, nodes, idx):
    """matrix: [cols][rows] words; nodes: the 2 * rows digests as [2 * rows][8]; idx: the queried rows.  Returns [len(idx)][opening_words]."""
    matrix = np.asarray(matrix, dtype=np.uint32)
    cols, rows = matrix.shape
    nodes = np.asarray(nodes, dtype=np.uint32).reshape(2 * rows, 8)
    out = np.zeros((len(idx), opening_words(rows, cols)), dtype=np.uint32)
    for q, row in enumerate(idx):
        row = int(row)
        assert 0 <= row < rows
        out[q, :cols] = matrix[:, row]
        for level in range(path_digests(rows)):
            out[q, cols + 8 * level:cols + 8 * level + 8] = nodes[((row + rows) >> level) ^ 1]
    return out
