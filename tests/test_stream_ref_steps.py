"""The plain-Python reference of steps 5 and 6 (stream_ref.py: pow4, deep_points, interpolate, deep_heads, divide_batch) against what can
be run without a GPU, and the planned inputs of the report-word tests of test_gpu_device_forms.py against the reference's own division.

Of the host forms only r0h_poly_interpolate_host runs without a device: the host branch of r0h_deep_subtract_heads computes its heads on
the host but ends in an upload and sub_head_kernel, so it is compared with stream_ref.deep_heads on the GPU
(test_gpu_device_forms.py::test_subtract_heads), and the library exports no other hash-free field helper to compare with."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import stream_ref as ref
from field_words import FAMILIES, ONE, P, POINT_KINDS, family, point, rnd
from stream_shapes import FRONT_LOADED, LAST_WORD_ONLY, THREE_PASSES, distinct_points, launch_order, report_cases


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 17, 64])
def test_interpolate_is_the_hosts_and_passes_through_its_points(n, kind):
    rng = np.random.default_rng([1, n, len(kind)])
    xs, ys = distinct_points(rng, n), family(rng, 4 * n, kind)
    want = ref.interpolate(xs, ys)
    assert np.array_equal(r0.poly_interpolate_host(xs, ys), want)
    for i in range(n):
        assert np.array_equal(ref.evaluate4(want, xs[4 * i:4 * i + 4]), ys[4 * i:4 * i + 4]), i


def test_interpolate_host_refuses_what_has_no_interpolant():
    rng = np.random.default_rng(2)
    x = rnd(rng, 4)
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_host: points 0 and 2 are equal"):
        r0.poly_interpolate_host(np.concatenate([x, rnd(rng, 4), x]), rnd(rng, 12))
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_host: 0 points \(1 to 64\)"):
        r0.poly_interpolate_host(np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_host: 65 points \(1 to 64\)"):
        r0.poly_interpolate_host(rnd(rng, 260), rnd(rng, 260))
    with pytest.raises(r0.R0HipError, match=r"r0h_poly_interpolate_host: point 1 not canonical"):
        r0.poly_interpolate_host(rnd(rng, 8), np.array([0, 0, 0, 0, 0, P, 0, 0], np.uint32))


@pytest.mark.parametrize("kind", POINT_KINDS)
def test_pow4_from_the_definition(kind):
    rng = np.random.default_rng([3, len(kind)])
    x = point(rng, kind)
    one = np.array([ONE, 0, 0, 0], np.uint32)
    assert np.array_equal(ref.pow4(x, 0), one)  # zero included
    assert np.array_equal(ref.pow4(x, 1), x)
    cur = one
    for e in range(1, 40):
        cur = ref._flat([ref.mul4(tuple(ref.dec(cur)), tuple(ref.dec(x)))])
        assert np.array_equal(ref.pow4(x, e), cur), e
    big = (1 << 31) + 12345  # x^(a + b) = x^a x^b at an exponent no loop reaches
    prod = ref.mul4(tuple(ref.dec(ref.pow4(x, 1 << 31))), tuple(ref.dec(ref.pow4(x, 12345))))
    assert np.array_equal(ref.pow4(x, big), ref._flat([prod]))
    if kind != "zero":  # the multiplicative group has p^4 - 1 elements
        assert np.array_equal(ref.pow4(x, P**4 - 1), one)
    z4 = ref.deep_points(x, ref.enc([1, 5]))
    assert np.array_equal(z4[:4], x) and np.array_equal(z4[8:], ref.pow4(x, 4))
    assert np.array_equal(z4[4:8], ref._flat([ref.scale4(tuple(ref.dec(x)), 5)]))


def test_deep_heads_on_a_table_small_enough_to_write_out():
    """two registers on combo 0 (2 taps, 1 tap), none on combo 1, mix m, coeff_u = u0 .. u2 then CHECK's c0 .. c15:
    head(0, 0) = u0 + m u2, head(0, 1) = u1, head(2, 0) = sum_j m^(2 + j) c_j, and no entry for combo 1"""
    rng = np.random.default_rng(4)
    cu, mix = rnd(rng, 4 * 19), rnd(rng, 4)
    u, m = ref._ext(ref.dec(cu)), tuple(ref.dec(mix))
    heads = ref.deep_heads(cu, [(0, 0, 2), (0, 2, 1)], 3, 2, mix)
    assert sorted(heads) == [(0, 0), (0, 1), (2, 0)]
    assert heads[(0, 0)] == ref.add4(u[0], ref.mul4(m, u[2])) and heads[(0, 1)] == u[1]
    tot = ref.ZERO4
    for j in range(16):
        tot = ref.add4(tot, ref.mul4(ref._pow4(m, 2 + j), u[3 + j]))
    assert heads[(2, 0)] == tot


def test_the_job_tables_launch_out_of_the_given_order():
    assert launch_order(THREE_PASSES) == [0, 1, 3, 2, 5, 4]
    assert launch_order(FRONT_LOADED) == [0, 3, 4, 1, 2]
    assert launch_order(list(range(130))) == list(range(130))


def test_the_planned_remainders_are_the_references():
    """What makes the report-word tests mean something: under stream_ref.poly_divide, job by job in the order given, the remainders of
    every case are zero except at the jobs it plans to fail -- and the case of the last word fails by that word alone."""
    names = set()
    for name, n, poly_idx, pt_idx, points, polys, fails in report_cases():
        names.add(name)
        pts = points.reshape(-1, 4)
        _, rems = ref.divide_batch(polys, n, [(k, pts[p]) for k, p in zip(poly_idx, pt_idx)])
        rems = rems.reshape(-1, 4)
        assert [j for j in range(len(poly_idx)) if rems[j].any()] == fails, name
        if "last-word-only" in name:
            assert np.array_equal(rems[fails[0]], LAST_WORD_ONLY) and not rems[fails[0]][:3].any(), name
    assert len(names) == len(report_cases())
    # two failures whose launch order is the opposite of the given one
    for table, a, b in ((THREE_PASSES, 2, 3), (THREE_PASSES, 4, 5), (FRONT_LOADED, 1, 4)):
        order = launch_order(table)
        assert a < b and order.index(b) < order.index(a)
