"""The DEEP-step streams of eltwise.hip and the division of scan.hip where the whole-proof tests cannot name a kernel: the running sums
of the evaluation kernel in their steady state, the host grouping of the evaluation requests, tables narrower than a row, and the mix,
fold, division and small element-wise kernels at corner operands and at every launch geometry.  Bit-exact against the CPU oracle, and against the plain-Python
reference (stream_ref.py) as well wherever n <= 2^10.  Operand families and points: field_words.py."""
import numpy as np
import pytest

import stream_ref as ref
from field_words import FAMILIES, ONE, P, POINT_KINDS, family, point, rnd
from stream_shapes import DIVIDE_SIZES, MIX_LAYOUTS

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5  # no field word: above p


def _rng(*key):
    return np.random.default_rng([int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key])


def _free(*bufs):
    for b in bufs:
        b.free()


def _evaluate(hal, cbuf, po2, which, xs, buffers=False):
    """the device's results, after checking that every slot was written and the word past the last one was not"""
    which, xs = np.asarray(which, np.uint32), np.asarray(xs, np.uint32)
    out = hal.copy_from(np.full(4 * which.size + 4, GUARD, np.uint32))
    if buffers:
        wb, xb = hal.copy_from(which), hal.copy_from(xs)
        hal.batch_evaluate_any_buf(cbuf, po2, wb, xb, which.size, out)
        _free(wb, xb)
    else:
        hal.batch_evaluate_any(cbuf, po2, which, xs, out)
    got = out.to_host()
    out.free()
    assert np.all(got[-4:] == GUARD), "the element past the last result was written"
    assert np.all(got[:-4] < P), "a result slot was left unwritten or holds a word that is not canonical"
    return got[:-4]


def _check_evaluate(hal, orc, cbuf, coeffs, po2, which, xs, buffers=False):
    got = _evaluate(hal, cbuf, po2, which, xs, buffers)
    assert np.array_equal(got, orc.batch_evaluate_any(coeffs, po2, which, xs))
    if po2 <= 10:
        assert np.array_equal(got, ref.evaluate_any(coeffs, po2, which, xs))


# ------------------------------------------------------------------ a. evaluation: the running sums in their steady state
def _rows_per_wave(po2, ng):
    """(fewest, most) rows a wave of eval_rows_kernel handles when ng columns share a point list (evaluate_any's launch geometry):
    rows of 2^9 coefficients, gb blocks of four waves per column, wave w of block b takes rows 4b + w, 4b + w + 4 gb, ..."""
    rows = 1 << (po2 - 9)
    gb = min(max(2048 // ng, 4), min((rows + 3) // 4, 64))
    return rows // (4 * gb), -(-rows // (4 * gb))


# (po2, columns, points per column): all columns of a case are asked at one point list, so they form one group of ng = columns
STEADY = [
    (20, 1, 1),    # rows 2048, gb = min(2048, 64) = 64: 256 waves, 8 rows each -- the fix branch runs at rows 4 and 6
    (20, 1, 2),    # the same through the two-point kernel
    (22, 1, 2),    # rows 8192, gb = 64: 32 rows each
    (19, 40, 1),   # rows 1024, gb = 2048 // 40 = 51: 204 waves, 1024 = 5 * 204 + 4 -- four waves take 6 rows, 200 take 5 (odd, unequal)
    (16, 600, 2),  # rows 128, gb = max(2048 // 600, 4) = 4: 16 waves, 8 rows each; 1,200 results: eval_reduce_kernel runs 19 blocks
]


def test_the_steady_state_shapes_reach_the_fix_branch():
    assert [_rows_per_wave(po2, ng) for po2, ng, _ in STEADY] == [(8, 8), (8, 8), (32, 32), (5, 6), (8, 8)]
    # what the operation-level tests had: one row per wave at most
    assert _rows_per_wave(16, 7) == (1, 1) and _rows_per_wave(12, 4) == (1, 1)


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("po2,cols,n_points", STEADY)
def test_evaluate_with_five_and_more_rows_per_wave(hal, orc, po2, cols, n_points, kind):
    """From a wave's fifth row on, the high words of its 64-bit sums are reduced before every second product; with words of p - 1
    the sums come as close to 2^64 as the coefficients can bring them.  Arithmetic per case: STEADY."""
    assert _rows_per_wave(po2, cols)[0] >= 5
    rng = _rng(10, po2, cols, n_points, kind)
    coeffs = family(rng, cols << po2, kind)
    cbuf = hal.copy_from(coeffs)
    try:
        lists = [("random",), ("top",)] if n_points == 1 else [("random", "top")]
        if (po2, cols, n_points) == STEADY[0]:
            lists += [("zero",), ("one",)]
        for kinds in lists:
            pts = np.concatenate([point(rng, k) for k in kinds])
            which = np.repeat(np.arange(cols, dtype=np.uint32), n_points)
            _check_evaluate(hal, orc, cbuf, coeffs, po2, which, np.tile(pts, cols))
    finally:
        cbuf.free()


# ------------------------------------------------------------------ b. evaluation: the host grouping
def _grouping_requests(rng):
    """(column, point) in request order.  Columns 0, 1, 2, 3 and 5 are asked at 1, 2, 3, 4 and 5 points, column 4 at none.  In the
    order a column's requests arrive: 1 -> [A B]; 2 -> [A B] [C], sharing the list [A B] with column 1; 3 -> [B A] [D D], the points
    of column 1 in the opposite order, then one point twice; 5 -> [C E] [A B] [D].  A third point is a second pass over the column."""
    A, B, C, D, E = point(rng, "random"), point(rng, "top"), point(rng, "random"), point(rng, "one"), point(rng, "zero")
    reqs = [(5, C), (3, B), (5, E), (2, A), (5, A), (3, A), (5, B), (1, A), (3, D), (2, B), (5, D), (0, A), (3, D), (1, B), (2, C)]
    cols = [c for c, _ in reqs]
    assert all(a != b for a, b in zip(cols, cols[1:])), "no two requests of a column are adjacent"
    assert [cols.count(c) for c in range(6)] == [1, 2, 3, 4, 0, 5]
    return reqs


@pytest.mark.parametrize("kind", FAMILIES)
def test_evaluate_groups_requests_by_column_and_point_list(hal, orc, kind):
    po2 = 11
    rng = _rng(20, kind)
    coeffs = family(rng, 6 << po2, kind)
    cbuf = hal.copy_from(coeffs)
    reqs = _grouping_requests(rng)
    which, xs = np.array([c for c, _ in reqs], np.uint32), np.concatenate([x for _, x in reqs])
    want = orc.batch_evaluate_any(coeffs, po2, which, xs)
    got = _evaluate(hal, cbuf, po2, which, xs)
    assert np.array_equal(got, want)
    # the same requests in the opposite order: other point lists per column, the same values
    back = _evaluate(hal, cbuf, po2, which[::-1], xs.reshape(-1, 4)[::-1].reshape(-1))
    assert np.array_equal(back.reshape(-1, 4)[::-1].reshape(-1), want)
    assert np.array_equal(_evaluate(hal, cbuf, po2, which, xs, buffers=True), want)
    for k in (0, 7):  # a single request
        assert np.array_equal(_evaluate(hal, cbuf, po2, which[k:k + 1], xs[4 * k:4 * k + 4]), want[4 * k:4 * k + 4])
    cbuf.free()


# ------------------------------------------------------------------ c. evaluation: tables narrower than a row, and the first rows
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("po2", [0, 1, 6, 7, 8, 9, 10])
def test_evaluate_narrow_tables(hal, orc, po2, kind):
    """po2 < 9: a row is shorter than the 512 positions a wave covers and the positions past it are masked -- one coefficient, two,
    one stripe of 64 lanes, two, four; 9: the first full row; 10: the first table with more than one."""
    rng = _rng(30, po2, kind)
    cols = 3
    coeffs = family(rng, cols << po2, kind)
    cbuf = hal.copy_from(coeffs)
    for kinds in [(k,) for k in POINT_KINDS] + [("random", "top"), ("zero", "one")]:
        pts = np.concatenate([point(rng, k) for k in kinds])
        which = np.repeat(np.arange(cols, dtype=np.uint32), len(kinds))
        _check_evaluate(hal, orc, cbuf, coeffs, po2, which, np.tile(pts, cols))
    cbuf.free()


# ------------------------------------------------------------------ d. mix_poly_coeffs, eltwise_sum_extelem
# the layouts: stream_shapes.MIX_LAYOUTS


def _check_mix(hal, orc, init, start, mix, inp, ibuf, combo_of, po2):
    combos = hal.copy_from(init)
    hal.mix_poly_coeffs(combos, start, mix, ibuf, combo_of, po2)
    got = combos.to_host()
    combos.free()
    want = orc.mix_poly_coeffs(init, start, mix, inp, combo_of, po2)
    assert np.array_equal(got, want)
    if po2 <= 10:
        assert np.array_equal(got, ref.mix_poly(init, start, mix, inp, combo_of, po2))
    return got


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("layout", sorted(MIX_LAYOUTS))
@pytest.mark.parametrize("po2", [0, 3, 8, 12])
def test_mix_poly_coeffs_at_corner_mixes(hal, orc, po2, layout, kind):
    """threads = n below 256 (po2 0, 3), exactly one block (8), many blocks (12); mix_start and mix over the four points"""
    rng = _rng(40, po2, layout, kind)
    n = 1 << po2
    combo_of, n_combo = MIX_LAYOUTS[layout]
    combo_of = np.array(combo_of, np.uint32)
    inp = family(rng, combo_of.size * n, kind)
    ibuf = hal.copy_from(inp)
    init = family(rng, 4 * n_combo * n, kind)
    for ks in POINT_KINDS:
        for km in POINT_KINDS:
            got = _check_mix(hal, orc, init, point(rng, ks), point(rng, km), inp, ibuf, combo_of, po2)
            untouched = [c for c in range(n_combo) if c not in combo_of]
            for c in untouched:
                assert np.array_equal(got[4 * c * n:4 * (c + 1) * n], init[4 * c * n:4 * (c + 1) * n])
    ibuf.free()


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_sum_extelem_over_a_mixed_result(hal, orc, n, kind):
    """six combos of 2^9 elements out of mix_poly_coeffs, summed as 6 x n and as 1 x n elements: less than a block, one short of
    one, exactly one, one more"""
    rng = _rng(50, n, kind)
    po2 = 9
    combo_of = np.array([2, 0, 2, 5, 0], np.uint32)
    inp = family(rng, combo_of.size << po2, kind)
    ibuf = hal.copy_from(inp)
    mixed = _check_mix(hal, orc, family(rng, 4 * 6 << po2, kind), point(rng, "random"), point(rng, "top"), inp, ibuf, combo_of, po2)
    mbuf = hal.copy_from(mixed)
    for count in (6, 1):
        out = hal.copy_from(np.full(4 * n + 1, GUARD, np.uint32))
        hal.eltwise_sum_extelem(out, mbuf, count, n)
        got = out.to_host()
        assert got[-1] == GUARD
        assert np.array_equal(got[:-1], orc.eltwise_sum_extelem(mixed, count, n))
        assert np.array_equal(got[:-1], ref.sum_extelem(mixed[:4 * count * n], count, n))
        out.free()
    _free(ibuf, mbuf)


# ------------------------------------------------------------------ e. fri_fold
@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n_out", [1, 3, 255, 257, 4096])
def test_fri_fold_tails_and_corner_mixes(hal, orc, n_out, kind):
    rng = _rng(60, n_out, kind)
    inp = family(rng, 4 * 16 * n_out, kind)
    ibuf = hal.copy_from(inp)
    for km in POINT_KINDS:
        mix = point(rng, km)
        out = hal.copy_from(np.full(4 * n_out + 1, GUARD, np.uint32))
        hal.fri_fold(out, ibuf, mix, n_out)
        got = out.to_host()
        out.free()
        assert got[-1] == GUARD
        assert np.array_equal(got[:-1], orc.fri_fold(inp, mix, n_out)), km
        if n_out <= 1 << 10:
            assert np.array_equal(got[:-1], ref.fri_fold(inp, mix, n_out)), km
    ibuf.free()


# ------------------------------------------------------------------ f. poly_divide
# the sizes: stream_shapes.DIVIDE_SIZES


@pytest.mark.parametrize("kind,n", [(k, n) for n in DIVIDE_SIZES for k in FAMILIES if n <= 8192 or k != "random"])
def test_poly_divide_at_corner_points_and_every_geometry(hal, orc, n, kind):
    rng = _rng(70, n, kind)
    v = family(rng, 4 * n, kind)
    buf = hal.copy_from(np.concatenate([v, np.full(4, GUARD, np.uint32)]))
    for kz in POINT_KINDS:
        z = point(rng, kz)
        buf.upload(v)
        rem = hal.poly_divide(buf, n, z)
        got = buf.to_host()
        assert np.all(got[-4:] == GUARD)
        q = got[:-4]
        want_q, want_rem = orc.poly_divide(v, n, z)
        assert np.array_equal(rem, want_rem) and np.array_equal(q, want_q), kz
        if n <= 1 << 10:
            ref_q, ref_rem = ref.poly_divide(v, z)
            assert np.array_equal(rem, ref_rem) and np.array_equal(q, ref_q), kz
        if kz == "zero":  # division by x: the coefficients move down by one, the constant term is left over
            assert np.array_equal(q[:-4], v[4:]) and not q[-4:].any() and np.array_equal(rem, v[:4])
    buf.free()


@pytest.mark.parametrize("kind", ["random", "top"])
def test_three_scans_back_to_back_share_a_pooled_block(hal, orc, kind):
    """At n = 8192 (two chunks) the temporaries of a prefix scan (48 bytes) and of a one-job division (128) fall into one size class of
    the context's pool, so sums, products and division enqueued with nothing read in between take the same block one after the other:
    only the stream orders them."""
    n = 8192
    rng = _rng(75, kind)
    a, b, c = (family(rng, 4 * n, kind) for _ in range(3))
    z = point(rng, "random")
    ab, bb, cb = hal.copy_from(a), hal.copy_from(b), hal.copy_from(c)
    hal.prefix_sums(ab, n)
    hal.prefix_products(bb, n)
    rem = hal.poly_divide(cb, n, z)
    got_a, got_b, got_c = ab.to_host(), bb.to_host(), cb.to_host()
    _free(ab, bb, cb)
    assert np.array_equal(got_a, (np.cumsum(a.reshape(n, 4).astype(np.int64), axis=0) % P).astype(np.uint32).reshape(-1))
    assert np.array_equal(got_b, orc.prefix_products(b, n))
    want_q, want_rem = orc.poly_divide(c, n, z)
    assert np.array_equal(got_c, want_q) and np.array_equal(rem, want_rem)


# ------------------------------------------------------------------ g. the small helpers
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_small_helpers_around_one_block(hal, n):
    rng = _rng(80, n)
    top, one = np.full(n, P - 1, np.uint32), np.full(n, 1, np.uint32)
    a = rnd(rng, n)
    tb, ob, ab = hal.copy_from(top), hal.copy_from(one), hal.copy_from(a)

    def run(op, *args):
        out = hal.copy_from(np.full(n + 1, GUARD, np.uint32))
        op(out, *args)
        got = out.to_host()
        out.free()
        assert got[-1] == GUARD
        return got[:-1]

    assert np.array_equal(run(hal.eltwise_add_elem, tb, tb, n), np.full(n, P - 2, np.uint32))  # 2 (p - 1) = p - 2
    assert not run(hal.eltwise_add_elem, tb, ob, n).any()                                      # (p - 1) + 1 = 0
    assert np.array_equal(run(hal.eltwise_add_elem, ab, tb, n), ((a.astype(np.int64) + P - 1) % P).astype(np.uint32))
    assert np.array_equal(run(hal.eltwise_copy_elem, ab, n), a)
    marked = np.concatenate([a, [0xFFFFFFFF]]).astype(np.uint32)  # the word past n is a marker too, and must stay one
    marked[[0, n // 2, n - 1]] = 0xFFFFFFFF
    zb = hal.copy_from(marked)
    hal.eltwise_zeroize_elem(zb, n)
    want = marked.copy()
    want[[0, n // 2, n - 1]] = 0
    assert np.array_equal(zb.to_host(), want)
    stride, idx = 5, 3
    src = rnd(rng, n * stride)
    sb = hal.copy_from(src)
    assert np.array_equal(run(hal.gather_sample, sb, idx, n, stride), src[idx::stride])
    _free(tb, ob, ab, zb, sb)


@pytest.mark.parametrize("m", [256, 257])
def test_scatter_of_one_block_and_one_more(hal, m):
    rng = _rng(90, m)
    offsets = rng.permutation(600)[:m + 2].astype(np.uint32)
    vals = rnd(rng, m + 2)
    want = np.full(600, GUARD, np.uint32)
    into = hal.copy_from(want)
    ob, vb = hal.copy_from(offsets), hal.copy_from(vals)
    ib = hal.copy_from(np.array([1, 9, m + 1], np.uint32))  # entries 1 .. m: exactly m of them
    hal.scatter(into, ib, ob, vb, 3)
    want[offsets[1:m + 1]] = vals[1:m + 1]
    assert np.array_equal(into.to_host(), want)
    _free(into, ob, vb, ib)
