"""The plain-Python reference of the stream operations (stream_ref.py) against the CPU oracle, on every machine: the device tests
of test_gpu_stream_edges.py lean on both, so the two must agree where both can run (n <= 2^10) -- on random words, on the corner
pool, on words that are all p - 1, and at the corner points (p-1)^4, zero and one."""
import numpy as np
import pytest

import stream_ref as ref
from field_words import FAMILIES, ONE, P, POINT_KINDS, family, point


def _rng(*key):
    return np.random.default_rng([int(k) if not isinstance(k, str) else sum(map(ord, k)) for k in key])


def test_words_convert_both_ways(orc):
    assert ref.R == ONE == orc.enc(1)
    vals = [0, 1, 2, P - 1, P - 2, 11, 1 << 30]
    assert [int(w) for w in ref.enc(vals)] == [orc.enc(v) for v in vals]
    assert ref.dec(ref.enc(vals)) == vals
    a, b = [3, P - 1, 0, 77], [P - 1, P - 1, P - 1, P - 1]
    assert np.array_equal(ref.enc(ref.mul4(a, b)), orc.fp4_mul(ref.enc(a), ref.enc(b)))


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("po2", [0, 1, 5, 10])
def test_evaluate(orc, po2, kind):
    rng = _rng(1, po2, kind)
    cols = 3
    coeffs = family(rng, cols << po2, kind)
    which = np.array([c for c in range(cols) for _ in POINT_KINDS], np.uint32)
    xs = np.concatenate([point(rng, k) for _ in range(cols) for k in POINT_KINDS])
    want = orc.batch_evaluate_any(coeffs, po2, which, xs)
    assert np.array_equal(ref.evaluate_any(coeffs, po2, which, xs), want)
    assert np.array_equal(ref.evaluate(coeffs[:1 << po2], xs[:4]), want[:4])


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("po2", [0, 3, 8])
def test_mix_poly_and_sum_extelem(orc, po2, kind):
    rng = _rng(2, po2, kind)
    n = 1 << po2
    combo_of, n_combo = np.array([2, 0, 2, 5, 0], np.uint32), 6
    inp = family(rng, combo_of.size * n, kind)
    for ks in POINT_KINDS:
        for km in POINT_KINDS:
            start, mix = point(rng, ks), point(rng, km)
            init = family(rng, 4 * n_combo * n, kind)
            want = orc.mix_poly_coeffs(init, start, mix, inp, combo_of, po2)
            assert np.array_equal(ref.mix_poly(init, start, mix, inp, combo_of, po2), want), (ks, km)
    assert np.array_equal(ref.sum_extelem(want, n_combo, n), orc.eltwise_sum_extelem(want, n_combo, n))
    if n >= 2:  # the same words as n / 2 elements of twice as many summands
        assert np.array_equal(ref.sum_extelem(want, 2 * n_combo, n // 2), orc.eltwise_sum_extelem(want, 2 * n_combo, n // 2))


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n_out", [1, 3, 64])
def test_fri_fold(orc, n_out, kind):
    rng = _rng(3, n_out, kind)
    inp = family(rng, 4 * 16 * n_out, kind)
    for km in POINT_KINDS:
        mix = point(rng, km)
        assert np.array_equal(ref.fri_fold(inp, mix, n_out), orc.fri_fold(inp, mix, n_out)), km


@pytest.mark.parametrize("kind", FAMILIES)
@pytest.mark.parametrize("n", [1, 2, 128, 1024])
def test_poly_divide(orc, n, kind):
    rng = _rng(4, n, kind)
    v = family(rng, 4 * n, kind)
    for kz in POINT_KINDS:
        z = point(rng, kz)
        q, rem = ref.poly_divide(v, z)
        want_q, want_rem = orc.poly_divide(v, n, z)
        assert np.array_equal(q, want_q) and np.array_equal(rem, want_rem), kz
        # the remainder of a division by (x - z) is the value at z: Horner over extension coefficients, component by component
        val = ref.ZERO4
        for c in range(4):
            part = tuple(ref.dec(ref.evaluate(v[c::4], z)))  # component c of every coefficient, a base-field polynomial
            val = ref.add4(val, ref.mul4(part, tuple(int(k == c) for k in range(4))))
        assert tuple(ref.dec(rem)) == val, kz
