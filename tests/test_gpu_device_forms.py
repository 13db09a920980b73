"""The device-challenge forms of steps 4-6 (what a proof runs under r0h_ctx_set_device_finish) called on their own, at the operands a
transcript never draws: challenges of zero, one and (p-1)^4, large exponents, unsorted columns, a point asked twice, job tables that
launch out of the given order, remainders that are not zero, and the launch geometries no shipped circuit reaches.  Bit-exact against
the host-challenge forms (pinned by test_gpu_stream_edges.py) and against the plain-Python reference (stream_ref.py) wherever n <= 2^10;
every output word canonical, a guard word behind every output and, where it sits at an offset, before it.  Operand families and
points: field_words.py; shapes and the planned divisions: stream_shapes.py (checked without a GPU by test_stream_ref_steps.py).

Not reachable, here or anywhere: how tail_collect turns a non-zero report word into "DEEP quotient of combo %u has a non-zero
remainder".  No honest or spoiled witness produces a non-zero remainder inside a live proof, and no hook into one is added for it; the
report word itself is pinned below (test_report_word_*).  The bit-reversed-coefficient path of the evaluation tables stays with the
whole-proof tests as well."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import evalcheck_circuits as hand
import stream_ref as ref
from conftest import circuit_path
from field_words import FAMILIES, ONE, P, POINT_KINDS, family, point, rnd
from test_gpu_evalcheck_rules import loaded
from stream_shapes import DIVIDE_SIZES, GUARD, MIX_LAYOUTS, THREE_PASSES, UNSORTED_LAYOUT, distinct_points, launch_order, report_cases

pytestmark = pytest.mark.gpu
CHECK = 16


def _rng(*key):
    return np.random.default_rng([int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key])


def _free(*bufs):
    for b in bufs:
        b.free()


def _placed(hal, words, offset=0):
    """`words` in device memory at word `offset`, guard words before and 4 behind"""
    return hal.copy_from(np.concatenate([np.full(offset, GUARD, np.uint32), np.asarray(words, np.uint32), np.full(4, GUARD, np.uint32)]))


def _blank(hal, n, offset=0):
    return hal.copy_from(np.full(offset + n + 4, GUARD, np.uint32))


def _taken(buf, n, offset=0, canonical=True):
    """the n words at `offset` of a buffer made by _placed / _blank, after checking the guards around them and that they are field words"""
    got = buf.to_host()
    assert got.size == offset + n + 4
    assert np.all(got[:offset] == GUARD), "a word before the output was written"
    assert np.all(got[offset + n:] == GUARD), "a word behind the output was written"
    if canonical:
        assert np.all(got[offset:offset + n] < P), "an output word was left unwritten or is not canonical"
    return got[offset:offset + n]


# ------------------------------------------------------------------ a. ext_powers
EXPS = [0, 1, 2, 1 << 31, (1 << 32) - 1, P - 1, P, P + 1]
_POWERS = {}  # (kind, with a table) -> (base, 257 powers by stream_ref.pow4): computed once, shared by every n and offset


def _powers(kind, table):
    if (kind, table) not in _POWERS:
        base = point(_rng(100, kind), kind)
        by_exp = {e: ref.pow4(base, e) for e in (EXPS if table else range(257))}
        want = np.concatenate([by_exp[EXPS[k % 8] if table else k] for k in range(257)])
        want.setflags(write=False)
        _POWERS[(kind, table)] = (base, want)
    return _POWERS[(kind, table)]


@pytest.mark.parametrize("table", [False, True], ids=["k", "exps"])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ext_powers(hal, n, table):
    """one lane short of a block, a block, one lane more; exponent k, and a table of 0, 1, 2, 2^31, 2^32 - 1, p - 1, p, p + 1 repeated;
    base, output and table at word offsets 0, 1 and 3 (the kernel claims word alignment only).  x^0 = 1 also for x = 0."""
    exps = np.array([EXPS[k % 8] for k in range(n)], np.uint32)
    for kind in POINT_KINDS:
        base, want = _powers(kind, table)
        if kind == "zero":
            assert np.array_equal(want[:4], [ONE, 0, 0, 0]) and not want[4:8].any()
        for base_off, out_off, exp_off in [(0, 0, 0), (1, 3, 1), (3, 1, 3)]:
            bb, ob = _placed(hal, base, base_off), _blank(hal, 4 * n, out_off)
            eb = _placed(hal, exps, exp_off) if table else None
            hal.ext_powers_buf(ob, out_off, bb, base_off, n, eb, exp_off)
            got = _taken(ob, 4 * n, out_off)
            assert np.array_equal(got, want[:4 * n]), (kind, base_off, out_off)
            _free(bb, ob, *([eb] if table else []))


def test_ext_powers_refuses_words_beyond_a_buffer(hal):
    b, o = hal.copy_from(np.zeros(8, np.uint32)), hal.copy_from(np.zeros(16, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_ext_powers_buf: the base at words \[5, \+4\) ends beyond a buffer of 8 words"):
        hal.ext_powers_buf(o, 0, b, 5, 1)
    with pytest.raises(r0.R0HipError, match=r"r0h_ext_powers_buf: the output at words \[1, \+16\) ends beyond a buffer of 16 words"):
        hal.ext_powers_buf(o, 1, b, 0, 4)
    with pytest.raises(r0.R0HipError, match=r"r0h_ext_powers_buf: the exponent table at words \[6, \+3\) ends beyond a buffer of 8 words"):
        hal.ext_powers_buf(o, 0, b, 0, 3, b, 6)
    _free(b, o)


# ------------------------------------------------------------------ b. batch_evaluate_any_points
# The table: [A, (p-1)^4, zero, one, A again, B] -- indices 0 and 4 hold equal words.  Requests (column, point index), in the order sent:
# column 0 at one point; 1 at two; 2 at three and 3 at five (MAX_NP = 2: a second and a third pass, an odd tail); 4 names index 3 twice;
# 5 names 0 and 4, different indices with equal words; 6 asks [0, 1] and 7 asks [1, 0]; 8 the last index.
EVAL_REQUESTS = [(3, 5), (6, 0), (2, 2), (7, 1), (4, 3), (1, 0), (3, 4), (5, 0), (2, 3), (8, 5), (6, 1), (3, 3), (0, 0), (4, 3), (7, 0), (1, 1), (3, 2), (5, 4), (2, 5),
                 (3, 1)]


def test_the_evaluation_requests_are_the_shapes_asked_for():
    by_col = {}
    for c, p in EVAL_REQUESTS:
        by_col.setdefault(c, []).append(p)
    assert [len(by_col[c]) for c in range(9)] == [1, 2, 3, 5, 2, 2, 2, 2, 1]
    assert by_col[4] == [3, 3] and by_col[5] == [0, 4] and by_col[6] == [0, 1] and by_col[7] == [1, 0] and by_col[8] == [5]


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("po2", [0, 6, 9, 10, 12])
def test_evaluate_any_points(hal, po2, kind):
    rng = _rng(110, po2, kind)
    a = point(rng, "random")
    table = np.concatenate([a, point(rng, "top"), point(rng, "zero"), point(rng, "one"), a, point(rng, "random")])
    n_points, cols = 6, 9
    coeffs = family(rng, cols << po2, kind)
    cbuf = hal.copy_from(coeffs)
    which, idx = np.array([c for c, _ in EVAL_REQUESTS], np.uint32), np.array([p for _, p in EVAL_REQUESTS], np.uint32)
    xs = table.reshape(-1, 4)[idx].reshape(-1)
    out = _blank(hal, 4 * which.size)
    hal.batch_evaluate_any(cbuf, po2, which, xs, out)  # the host-challenge form: pinned by test_gpu_stream_edges.py
    want = _taken(out, 4 * which.size)
    out.free()
    if po2 <= 10:
        assert np.array_equal(want, ref.evaluate_any(coeffs, po2, which, xs))
    for off in (0, 1):
        tb, out = _placed(hal, table, off), _blank(hal, 4 * which.size)
        hal.batch_evaluate_any_points(cbuf, po2, which, idx, tb, off, n_points, out)
        assert np.array_equal(_taken(out, 4 * which.size), want), off
        # a table of one point, and one request
        one = _blank(hal, 8)
        hal.batch_evaluate_any_points(cbuf, po2, [2, 7], [0, 0], tb, off + 4 * 5, 1, one)
        assert np.array_equal(_taken(one, 8), np.concatenate([want[4 * 18:4 * 19], _single(hal, cbuf, po2, 7, table[20:24])]))
        _free(tb, out, one)
    cbuf.free()


def _single(hal, cbuf, po2, col, x):
    out = _blank(hal, 4)
    hal.batch_evaluate_any(cbuf, po2, [col], x, out)
    got = _taken(out, 4)
    out.free()
    return got


def test_evaluate_any_points_refuses_an_index_outside_the_table(hal):
    cbuf, tb, out = hal.copy_from(np.zeros(2 << 6, np.uint32)), hal.copy_from(np.zeros(4 * 6, np.uint32)), hal.copy_from(np.zeros(8, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_batch_evaluate_any: request 1 names point 6 of a table of 6"):
        hal.batch_evaluate_any_points(cbuf, 6, [0, 1], [5, 6], tb, 0, 6, out)
    with pytest.raises(r0.R0HipError, match=r"r0h_batch_evaluate_any_points: the point table at words \[1, \+24\) ends beyond a buffer of 24 words"):
        hal.batch_evaluate_any_points(cbuf, 6, [0, 1], [5, 5], tb, 1, 6, out)
    _free(cbuf, tb, out)


# ------------------------------------------------------------------ c. mix_poly_coeffs_mixbuf
def test_one_layout_is_unsorted():
    combo_of = MIX_LAYOUTS[UNSORTED_LAYOUT][0]
    order = sorted(range(len(combo_of)), key=lambda c: combo_of[c])  # (stable)
    assert order == [1, 4, 0, 2, 3] and all(order[k] != k for k in range(5))


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("layout", sorted(MIX_LAYOUTS))
@pytest.mark.parametrize("po2", [0, 3, 8, 12])
def test_mix_poly_coeffs_mixbuf(hal, po2, layout, kind):
    """column c is weighed by mix^(first_exp + c) whatever order the columns are sorted into (`gaps` is the unsorted layout); the
    combos are accumulated into, so they start from non-zero words"""
    rng = _rng(120, po2, layout, kind)
    n = 1 << po2
    combo_of, n_combo = MIX_LAYOUTS[layout]
    combo_of = np.array(combo_of, np.uint32)
    inp = family(rng, combo_of.size * n, kind)
    init = family(rng, 4 * n_combo * n, kind)
    init[init == 0] = 1
    ibuf = hal.copy_from(inp)
    for i, first_exp in enumerate((0, 1, 37)):
        for j, km in enumerate(POINT_KINDS):
            mix, off = point(rng, km), (i + j) % 2
            start = ref.pow4(mix, first_exp)
            host = _placed(hal, init)
            hal.mix_poly_coeffs(host, start, mix, ibuf, combo_of, po2)  # the host-challenge form: pinned by test_gpu_stream_edges.py
            want = _taken(host, init.size)
            if po2 <= 10:
                assert np.array_equal(want, ref.mix_poly(init, start, mix, inp, combo_of, po2))
            mb, combos = _placed(hal, mix, off), _placed(hal, init)
            hal.mix_poly_coeffs_mixbuf(combos, first_exp, mb, off, ibuf, combo_of, po2)
            got = _taken(combos, init.size)
            assert np.array_equal(got, want), (first_exp, km, off)
            for c in set(range(n_combo)) - set(combo_of.tolist()):
                assert np.array_equal(got[4 * c * n:4 * (c + 1) * n], init[4 * c * n:4 * (c + 1) * n])
            _free(host, mb, combos)
    ibuf.free()


# ------------------------------------------------------------------ d. poly_divide_batch, poly_divide_batch_points
def _job_by_job(hal, polys, n, poly_idx, points):
    """r0h_poly_divide applied job by job in the order given (pinned by test_gpu_stream_edges.py): (the polynomials, the remainders)"""
    cur, rems = polys.copy(), []
    one = hal.alloc(4 * n)
    for j, k in enumerate(poly_idx):
        one.upload(cur[4 * n * k:4 * n * (k + 1)])
        rems.append(hal.poly_divide(one, n, points[4 * j:4 * j + 4]))
        cur[4 * n * k:4 * n * (k + 1)] = one.to_host()
    one.free()
    return cur, np.concatenate(rems)


def _report_of(rems):
    bad = [j for j, r in enumerate(np.asarray(rems).reshape(-1, 4)) if r.any()]
    return 1 + bad[0] if bad else 0


def _check_divisions(hal, polys, n, poly_idx, pt_idx, table, plain_ref):
    """both batch forms against the one-job form, job by job, and against each other; the report word against the remainders"""
    poly_idx, pt_idx = list(poly_idx), list(pt_idx)
    points = table.reshape(-1, 4)[pt_idx].reshape(-1)
    want_q, want_rem = _job_by_job(hal, polys, n, poly_idx, points)
    if plain_ref:
        ref_q, ref_rem = ref.divide_batch(polys, n, [(k, points[4 * j:4 * j + 4]) for j, k in enumerate(poly_idx)])
        assert np.array_equal(want_q, ref_q) and np.array_equal(want_rem, ref_rem)
    pb = _placed(hal, polys)
    rem = hal.poly_divide_batch(pb, n, poly_idx, points)
    assert np.all(rem < P)
    assert np.array_equal(rem, want_rem), "remainders differ, or are not in the order given"
    assert np.array_equal(_taken(pb, polys.size), want_q)
    for off in (0, 1):
        pb.upload(polys)
        tb, rb = _placed(hal, table, off), _blank(hal, 1, 2)
        hal.poly_divide_batch_points(pb, n, poly_idx, pt_idx, tb, off, table.size // 4, rb, 2)
        assert np.array_equal(_taken(pb, polys.size), want_q), off
        assert int(_taken(rb, 1, 2, canonical=False)[0]) == _report_of(want_rem)
        assert np.array_equal(_taken(tb, table.size, off), table)
        _free(tb, rb)
    pb.free()
    return want_rem


@pytest.mark.parametrize("kind,n", [(k, n) for n in DIVIDE_SIZES if n <= 1 << 13 for k in FAMILIES if n <= 1 << 10 or k == "random"])
def test_divide_batch_job_tables(hal, n, kind):
    """one job; three passes whose launch order is not the given one; one point twice on one polynomial -- at every scan geometry"""
    rng = _rng(130, n, kind)
    table = np.concatenate([point(rng, k) for k in POINT_KINDS] + [point(rng, "random")])
    polys = family(rng, 3 * 4 * n, kind)
    assert launch_order(THREE_PASSES) != list(range(6))
    for poly_idx, pt_idx in [([1], [0]), (THREE_PASSES, [0, 1, 4, 2, 3, 0]), ([0, 2, 2, 0], [4, 0, 0, 4]), ([1, 1], [1, 1])]:
        rems = _check_divisions(hal, polys, n, poly_idx, pt_idx, table, n <= 1 << 10)
        if kind == "random" and n > 1:
            assert rems.reshape(-1, 4)[0].any()  # random polynomials do not divide: the report names job 0


@pytest.mark.parametrize("n_polys", [65, 130])
@pytest.mark.parametrize("kind", FAMILIES)
def test_divide_batch_job_tables_across_64_jobs(hal, n_polys, kind):
    rng = _rng(140, n_polys, kind)
    table = np.concatenate([point(rng, k) for k in POINT_KINDS] + [point(rng, "random")])
    polys = family(rng, n_polys * 4 * 16, kind)
    order = rng.permutation(n_polys).tolist()  # job j divides polynomial order[j]
    rems = _check_divisions(hal, polys, 16, order, [j % 5 for j in range(n_polys)], table, True).reshape(-1, 4)
    if kind == "random":
        assert len({tuple(r) for r in rems}) == n_polys  # all different: an order mistaken anywhere shows


@pytest.mark.parametrize("case", range(len(report_cases())), ids=[c[0] for c in report_cases()])
def test_report_word(hal, case):
    """polynomials built as q(x) * prod (x - point), so that every remainder is zero, then spoiled so that exactly the planned jobs
    fail (stream_shapes.report_cases; that the plan holds under the reference is test_stream_ref_steps.py's): the word is 0, or 1 +
    the first failing job in the order GIVEN, also where that job is launched later than another that fails, where it is job 63, 64 or
    the last of 65 and 130, and where only the last word of its remainder is not zero.  The word sits at offset 2, its neighbours stay."""
    name, n, poly_idx, pt_idx, table, polys, fails = report_cases()[case]
    points = table.reshape(-1, 4)[pt_idx].reshape(-1)
    _, ref_rem = ref.divide_batch(polys, n, [(k, points[4 * j:4 * j + 4]) for j, k in enumerate(poly_idx)])
    assert [j for j, r in enumerate(ref_rem.reshape(-1, 4)) if r.any()] == fails  # as planned, before the device is asked
    want = 1 + fails[0] if fails else 0
    pb, tb, rb = _placed(hal, polys), _placed(hal, table, 1), _blank(hal, 1, 2)
    hal.poly_divide_batch_points(pb, n, poly_idx, pt_idx, tb, 1, table.size // 4, rb, 2)
    assert int(_taken(rb, 1, 2, canonical=False)[0]) == want, name
    _taken(pb, polys.size)
    pb.upload(polys)
    rem = hal.poly_divide_batch(pb, n, poly_idx, points)
    assert np.array_equal(rem, ref_rem), name
    _free(pb, tb, rb)


def test_report_word_of_no_jobs_is_zero(hal):
    pb, tb, rb = _placed(hal, rnd(_rng(150), 64)), _placed(hal, rnd(_rng(151), 8)), _blank(hal, 1, 2)
    hal.poly_divide_batch_points(pb, 16, [], [], tb, 0, 2, rb, 2)
    assert int(_taken(rb, 1, 2, canonical=False)[0]) == 0
    assert hal.poly_divide_batch(pb, 16, [], []).size == 0
    with pytest.raises(r0.R0HipError, match=r"poly_divide: job 1 names point 2 of a table of 2"):
        hal.poly_divide_batch_points(pb, 16, [0, 0], [1, 2], tb, 0, 2, rb, 2)
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_divide_batch_points: the report word at words \[7, \+1\) ends beyond a buffer of 7 words"):
        hal.poly_divide_batch_points(pb, 16, [0], [1], tb, 0, 2, rb, 7)
    with pytest.raises(r0.R0HipError, match=r"poly_divide: polynomial 1 outside a buffer of 1"):
        hal.poly_divide_batch(pb, 16, [0, 1], rnd(_rng(152), 8))
    _free(pb, tb, rb)


# ------------------------------------------------------------------ e. deep_points
@pytest.mark.parametrize("n_backs", [1, 2, 63, 64])
def test_deep_points(hal, n_backs):
    """64 backs are 65 points: the z^4 lane sits alone in a second workgroup"""
    rng = _rng(160, n_backs)
    wpow = np.concatenate([[ONE, 0, P - 1], rnd(rng, 64)]).astype(np.uint32)[:n_backs]
    for kind in POINT_KINDS:
        z = point(rng, kind)
        want = ref.deep_points(z, wpow)
        for off in (0, 1):
            zb, out = _placed(hal, z, off), _blank(hal, 4 * (n_backs + 1))
            hal.deep_points_buf(out, zb, off, wpow)
            assert np.array_equal(_taken(out, 4 * (n_backs + 1)), want), (kind, off)
            _free(zb, out)


def test_deep_points_refuses_no_backs_and_more_than_64(hal):
    zb, out = hal.copy_from(np.zeros(4, np.uint32)), hal.copy_from(np.zeros(4 * 66, np.uint32))
    for n_backs in (0, 65):
        with pytest.raises(r0.R0HipError, match=r"r0h_deep_points_buf: %d backs \(1 to 64\)" % n_backs):
            hal.deep_points_buf(out, zb, 0, np.full(n_backs, ONE, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_points_buf: the z at words \[1, \+4\) ends beyond a buffer of 4 words"):
        hal.deep_points_buf(out, zb, 1, [ONE])
    _free(zb, out)


# ------------------------------------------------------------------ f. poly_interpolate_regs
N_POINTS = 66
SIZES = [1, 2, 3, 4, 5, 17, 64]
# register sizes per table: every size alone; all of them in one table; then n_regs + 16 lanes that end exactly at a block of 64 (48),
# one short of it (47), one lane into the next block (49), and a second block full (64 registers: lanes 64 .. 79 copy CHECK)
REG_TABLES = {"alone-%d" % s: [s] for s in SIZES}
REG_TABLES["all-sizes"] = SIZES
REG_TABLES.update({"regs-%d" % r: [SIZES[k % 5] for k in range(r)] for r in (47, 48, 49, 64)})


def _reg_table(sizes):
    """(regs as (first tap, taps), point index of every tap): register r's taps are a window of the point table that starts at 3r, so
    neighbouring registers share points and no register names a point twice"""
    regs, tap_pt, first = [], [], 0
    for r, s in enumerate(sizes):
        regs.append((first, s))
        tap_pt += [(3 * r + j) % N_POINTS for j in range(s)]
        first += s
    return regs, tap_pt


_POINTS = {}


def _point_table():
    if not _POINTS:
        _POINTS[0] = distinct_points(_rng(170), N_POINTS)
        _POINTS[0].setflags(write=False)
    return _POINTS[0]


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("name", list(REG_TABLES))
def test_interpolate_regs(hal, name, kind):
    sizes = REG_TABLES[name]
    table = _point_table()
    pts = table.reshape(-1, 4)
    assert len({tuple(p) for p in pts}) == N_POINTS and any(not p.any() for p in pts) and any(np.all(p == P - 1) for p in pts)
    regs, tap_pt = _reg_table(sizes)
    n_taps = len(tap_pt)
    for first, s in regs:  # the interpolant is undefined otherwise
        assert len(set(tap_pt[first:first + s])) == s
    if len(sizes) > 1:  # taps of different registers share points
        assert len(set(tap_pt)) < n_taps
    rng = _rng(171, name, kind)
    eval_u = family(rng, 4 * (n_taps + CHECK), kind)
    want = eval_u.copy()  # CHECK's sixteen openings are copied unchanged
    for first, s in regs:
        xs, ys = pts[tap_pt[first:first + s]].reshape(-1), eval_u[4 * first:4 * (first + s)]
        want[4 * first:4 * (first + s)] = r0.poly_interpolate_host(xs, ys)
        if s <= 17 or (name == "alone-64" and kind == "random"):
            assert np.array_equal(want[4 * first:4 * (first + s)], ref.interpolate(xs, ys))
    eb = hal.copy_from(eval_u)
    listed = regs[::-1] if name == "all-sizes" else regs  # (the order the registers are listed in is not the order of their taps)
    for off in (0, 1):
        tb, out = _placed(hal, table, off), _blank(hal, 4 * (n_taps + CHECK))
        hal.poly_interpolate_regs(out, eb, tb, off, N_POINTS, tap_pt, listed)
        got = _taken(out, 4 * (n_taps + CHECK))
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "offset %d: %d words differ, the first in element %d of %d taps" % (off, bad.size, bad[0] // 4, n_taps)
        _free(tb, out)
    eb.free()


def test_interpolate_regs_refusals(hal):
    """by message, before any launch: no such input reaches a kernel"""
    tb, eb, out = hal.copy_from(np.zeros(4 * 4, np.uint32)), hal.copy_from(np.zeros(4 * 116, np.uint32)), hal.copy_from(np.zeros(4 * 116, np.uint32))
    call = lambda tap_pt, regs: hal.poly_interpolate_regs(out, eb, tb, 0, 4, tap_pt, regs)  # noqa: E731
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: register 1 has 0 taps \(1 to 64\)"):
        call([0, 1, 2], [(0, 2), (2, 0)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: register 0 has 65 taps \(1 to 64\)"):
        call([0] * 100, [(0, 65)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: registers 0 and 1 overlap at tap 1"):
        call([0, 1, 2], [(0, 2), (1, 2)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: register 1 runs past the 3 taps"):
        call([0, 1, 2], [(0, 2), (2, 2)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: tap 2 names point 4 of a table of 4"):
        call([0, 1, 4], [(0, 2), (2, 1)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: the point table at words \[1, \+16\) ends beyond a buffer of 16 words"):
        hal.poly_interpolate_regs(out, eb, tb, 1, 4, [0, 1, 2], [(0, 2), (2, 1)])
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_regs: the evaluations at words \[0, \+468\) ends beyond a buffer of 464 words"):
        call([0] * 101, [(0, 1)])
    _free(tb, eb, out)


# ------------------------------------------------------------------ g. deep_subtract_heads
# (combos, registers as (combo, first tap, taps)): two registers of unequal sizes on combo 0, none on combo 1, a 64-tap register on combo 2
# -- 5 + 0 + 64 + 1 = 70 entries; and the 64-tap register alone before CHECK: 65 entries, 260 pairs, a second workgroup of deep_head_kernel
# (64 entries a block) and of sub_head_kernel (256 pairs a block)
HEAD_TABLES = {"shared": (3, [(0, 0, 3), (2, 8, 64), (0, 3, 5)]), "sixty-five": (1, [(0, 0, 64)])}


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("name", sorted(HEAD_TABLES))
@pytest.mark.parametrize("po2", [6, 9])
def test_subtract_heads(hal, po2, name, kind):
    """the device branch (deep_head_kernel) equals the host branch (head_values_host), and both the reference applied to the combos:
    only the head words change, and the whole buffer is compared"""
    n_combos, regs = HEAD_TABLES[name]
    n_taps = max(f + s for _, f, s in regs)
    rng = _rng(180, po2, name, kind)
    init = family(rng, 4 * (n_combos + 1) << po2, kind)
    coeff_u = family(rng, 4 * (n_taps + CHECK), kind)
    for j, km in enumerate(POINT_KINDS):
        mix = point(rng, km)
        heads = ref.deep_heads(coeff_u, regs, n_taps, n_combos, mix)
        assert (1, 0) not in heads or name != "shared"  # combo 1 has no fix entries
        want = ref.subtract_heads(init, po2, heads)
        changed = np.nonzero(want != init)[0] // 4
        assert all((int(e) >> po2, int(e) & ((1 << po2) - 1)) in heads for e in changed)
        cb = _placed(hal, init)
        hal.deep_subtract_heads(cb, po2, n_combos, regs, n_taps, coeff_u, mix)
        assert np.array_equal(_taken(cb, init.size), want), ("host", km)
        for off_u, off_m in [(0, 1), (1, 0)] if j % 2 else [(0, 0), (3, 1)]:
            cb.upload(init)
            ub, mb = _placed(hal, coeff_u, off_u), _placed(hal, mix, off_m)
            hal.deep_subtract_heads(cb, po2, n_combos, regs, n_taps, ub, mb, off_u, off_m)
            assert np.array_equal(_taken(cb, init.size), want), ("device", km, off_u, off_m)
            _free(ub, mb)
        cb.free()


def test_subtract_heads_refusals(hal):
    cb, ub, mb = hal.copy_from(np.zeros(4 * 2 << 6, np.uint32)), hal.copy_from(np.zeros(4 * 20, np.uint32)), hal.copy_from(np.zeros(4, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_subtract_heads: register 0 names combo 1 of 1"):
        hal.deep_subtract_heads(cb, 6, 1, [(1, 0, 2)], 4, ub, mb)
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_subtract_heads: register 0 has 65 taps"):
        hal.deep_subtract_heads(cb, 6, 1, [(0, 0, 65)], 4, ub, mb)
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_subtract_heads: register 0 runs past the 4 taps"):
        hal.deep_subtract_heads(cb, 6, 1, [(0, 3, 2)], 4, ub, mb)
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_subtract_heads: 2 combos and CHECK's exceed the combos buffer"):
        hal.deep_subtract_heads(cb, 6, 2, [(0, 0, 2)], 4, ub, mb)
    with pytest.raises(r0.R0HipError, match=r"r0h_deep_subtract_heads: the interpolants at words \[1, \+80\) ends beyond a buffer of 80 words"):
        hal.deep_subtract_heads(cb, 6, 1, [(0, 0, 2)], 4, ub, mb, 1, 0)
    _free(cb, ub, mb)


# ------------------------------------------------------------------ h. eval_check_mixbuf
@pytest.fixture(scope="module")
def hand_circuits(hal):
    held = {}
    yield held
    for gc in held.values():
        gc.free()


@pytest.mark.parametrize("po2", [6, 7])
@pytest.mark.parametrize("case", hand.cases() + [("tiny", None)], ids=hand.case_id)
def test_eval_check_mixbuf(hal, hand_circuits, case, po2, monkeypatch):
    """r0h_eval_check with the same poly_mix as host words, on every hand circuit and its cut variants (several kernels share the one
    table of powers) and on tiny; poly_mix of every kind, at word offsets 0 and 1"""
    name = hand.case_id(case)
    if case[0] == "tiny" and case not in hand_circuits:
        hand_circuits[case] = hal.load_circuit(np.fromfile(circuit_path("tiny"), dtype=np.uint32))
    gc = loaded(hal, hand_circuits, case, monkeypatch)
    rng = _rng(190, name, po2)
    words = 16 << po2
    groups = [hal.copy_from(rnd(rng, max(size, 1) * (4 << po2))) for size in gc.group_size]
    glob, mix = rnd(rng, max(gc.n_global, 1)), rnd(rng, max(gc.n_mix, 1))
    for kind in POINT_KINDS:
        pm = point(rng, kind)
        host = _blank(hal, words)
        r0._check(r0.lib().r0h_eval_check(hal.ctx, gc.handle, po2, groups[0].handle, groups[1].handle, groups[2].handle, r0._u32arr(glob)[1], r0._u32arr(mix)[1],
                                          r0._u32arr(pm)[1], host.handle))
        want = _taken(host, words)
        host.free()
        for off in (0, 1):
            mb, check = _placed(hal, pm, off), _blank(hal, words)
            hal.eval_check_mixbuf(gc, po2, groups[0], groups[1], groups[2], glob, mix, mb, off, check)
            assert np.array_equal(_taken(check, words), want), (kind, off)
            _free(mb, check)
    _free(*groups)
    mb = hal.copy_from(np.zeros(5, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_eval_check_mixbuf: the poly_mix at words \[2, \+4\) ends beyond a buffer of 5 words"):
        hal.eval_check_mixbuf(gc, po2, mb, mb, mb, glob, mix, mb, 2, mb)
    mb.free()
