"""The log-derivative argument on the device against the exact reference (logup_ref.py), the host count and the oracle, on generated
LOGUP circuits (logup_circuits.py): multiplicities and the contract's errors, ACCUM and the public totals at every shape of the scan,
seals that prove and verify -- and stop verifying with one multiplicity off -- and the two scans themselves at every geometry."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import logup_circuits as lc
import logup_ref as ref
from test_logup import ERROR_SEED, SEEDS, _error_cases, host_multiplicities, many_lookups_blob

pytestmark = pytest.mark.gpu
P = ref.P
TABLED = [s for s in SEEDS if lc.generate(s).kinds]
SMALL = lc.generate(101, tables=[], n_chain=1, n_public=1, lean=True)     # two accumulators: the largest sizes


def device_multiplicities(hal, gc, po2, data, glob):
    buf = hal.copy_from(data)
    try:
        hal.logup_multiplicities(gc, po2, buf, glob)
        return buf.to_host()
    finally:
        buf.free()


@pytest.mark.parametrize("po2", [16, 17, 21])
@pytest.mark.parametrize("seed", TABLED)
def test_device_multiplicities_equal_the_reference_host_and_oracle(hal, orc, seed, po2):
    c = lc.generate(seed)
    gc = hal.load_circuit(c.words)
    data, glob, _ = c.witness(po2, seed=po2)
    want = ref.multiplicities(c.words, data, glob, po2)
    assert np.array_equal(device_multiplicities(hal, gc, po2, data, glob), want)
    assert np.array_equal(host_multiplicities(c.words, po2, data, glob), want)
    if po2 < 21:
        assert np.array_equal(orc.circuit(c.words).logup_multiplicities(po2, data, glob), want)
    gc.free()


@pytest.mark.parametrize("case", ["numerator 2", "outside R16", "outside AND"])
def test_device_multiplicities_refuse_a_witness_that_breaks_the_contract(hal, case):
    c = lc.generate(ERROR_SEED, tables=[1, 2], n_chain=4)
    gc = hal.load_circuit(c.words)
    data, glob = _error_cases(c, 16)[case]
    with pytest.raises(r0.R0HipError, match="neither 0 nor 1" if case == "numerator 2" else "not in its table"):
        device_multiplicities(hal, gc, 16, data, glob)
    ok, glob, _ = c.witness(16, seed=1)  # the same circuit and context go on working
    assert np.array_equal(device_multiplicities(hal, gc, 16, ok, glob), ref.multiplicities(c.words, ok, glob, 16))
    gc.free()


def test_device_refuses_more_than_p_minus_1_lookups_of_a_table(hal):
    gc = hal.load_circuit(many_lookups_blob(31))
    with pytest.raises(r0.R0HipError, match="p - 1"):
        device_multiplicities(hal, gc, 24, np.zeros(2 << 24, dtype=np.uint32), [])
    gc.free()


def check_accum(hal, orc, c, po2, reference=True):
    gc = hal.load_circuit(c.words)
    oc = orc.circuit(c.words)
    data, glob, mix = c.witness(po2, seed=3)
    code = oc.witgen(po2, 0)[0]
    data = ref.multiplicities(c.words, data, glob, po2)
    cb, db = hal.copy_from(code), hal.copy_from(data)
    want_glob = oc.logup_totals(po2, code, data, glob)
    assert np.array_equal(hal.logup_totals(gc, po2, cb, db, glob), want_glob)
    acc = hal.accum_public(gc, po2, cb, db, want_glob, mix)
    want = oc.accum_public(po2, code, data, want_glob, mix)
    assert np.array_equal(acc.to_host(), want)
    if reference:  # (the reference takes minutes at 2^24 rows: the oracle alone is the check there)
        assert np.array_equal(ref.totals(c.words, po2, code, data, glob), want_glob)
        assert np.array_equal(ref.accum(c.words, po2, code, data, want_glob, mix), want)
    for b in (acc, cb, db):
        b.free()
    gc.free()


@pytest.mark.parametrize("po2", [16, 17])
@pytest.mark.parametrize("seed", TABLED)
def test_device_accumulation_equals_the_reference_and_oracle_with_tables(hal, orc, seed, po2):
    check_accum(hal, orc, lc.generate(seed), po2)


@pytest.mark.parametrize("po2", [20, 21])
def test_device_accumulation_with_tables_at_the_largest_trace_sizes(hal, orc, po2):
    check_accum(hal, orc, lc.generate(TABLED[0], n_chain=1, n_public=1), po2)


@pytest.mark.parametrize("po2", [4, 5, 8, 11, 12, 13])
@pytest.mark.parametrize("seed", [s for s in SEEDS if not lc.generate(s).kinds])
def test_device_accumulation_without_tables_at_every_scan_shape(hal, orc, seed, po2):
    """scan_geom: threads = n (po2 < 8), chunk = n (po2 < 12), one block of chunks, two chunks ..."""
    check_accum(hal, orc, lc.generate(seed), po2)


@pytest.mark.parametrize("po2", [22, 24])
def test_device_accumulation_beyond_256_chunks(hal, orc, po2):
    """more than 256 chunks: every thread of scan_link_kernel takes 4 (2^22) or 16 (2^24) of them"""
    check_accum(hal, orc, SMALL, po2, reference=po2 == 22)


# ---- end to end
E2E = [(TABLED[0], 16), (TABLED[-1], 16), ([s for s in SEEDS if not lc.generate(s).kinds][-1], 10)]


def prove(hal, orc, c, po2, edit=None):
    gc, oc = hal.load_circuit(c.words), orc.circuit(c.words)
    data, glob, _ = c.witness(po2, seed=5, challenges="random")
    code = oc.witgen(po2, 0)[0]
    data = ref.multiplicities(c.words, data, glob, po2)
    glob = ref.totals(c.words, po2, code, data, glob)
    if edit is not None:
        data = edit(data.copy())
    cb, db = hal.copy_from(code), hal.copy_from(data)
    seal = hal.prove_segment(gc, po2, cb, db, glob)
    for b in (cb, db):
        b.free()
    gc.free()
    return seal, oc, (code, data, glob)


@pytest.mark.parametrize("seed,po2", E2E)
def test_a_generated_circuit_proves_and_verifies_as_the_oracle_does(hal, orc, seed, po2):
    c = lc.generate(seed)
    seal, oc, (code, data, glob) = prove(hal, orc, c, po2)
    assert oc.verify(seal) == (0, "ok")
    assert r0.verify_seal(c.words, seal)[0] == 0
    assert np.array_equal(seal, oc.prove(po2, code, data, glob))


@pytest.mark.parametrize("seed,po2", [e for e in E2E if lc.generate(e[0]).kinds])
def test_one_multiplicity_off_by_one_breaks_the_chain(hal, orc, seed, po2):
    c = lc.generate(seed)
    k = c.kinds[-1]

    def edit(d):
        d = d.reshape(-1, 1 << po2)
        d[c.mult[k], 4096] = ref.enc(int(ref.dec(d[c.mult[k], 4096])) + 1)
        return d.reshape(-1)
    seal, oc, _ = prove(hal, orc, c, po2, edit)
    assert oc.verify(seal)[0] == 4
    assert r0.verify_seal(c.words, seal)[0] == 4


# ---- the scans, directly
def _words(rng, n, kind):
    if kind == "extreme":
        return np.asarray(lc.EXTREME, dtype=np.uint32)[rng.integers(0, len(lc.EXTREME), size=4 * n)]
    return rng.integers(0, P, size=4 * n).astype(np.uint32)


def _py_products(w):
    """plain Python: running products of Montgomery Fp4 words"""
    R, RI = (1 << 32) % P, pow(1 << 32, P - 2, P)
    acc, out = [1, 0, 0, 0], []
    for i in range(0, len(w), 4):
        x = [int(v) * RI % P for v in w[i:i + 4]]
        c = [0] * 7
        for a in range(4):
            for b in range(4):
                c[a + b] += acc[a] * x[b]
        acc = [(c[0] + 11 * c[4]) % P, (c[1] + 11 * c[5]) % P, (c[2] + 11 * c[6]) % P, c[3] % P]
        out += [v * R % P for v in acc]
    return np.array(out, dtype=np.uint32)


@pytest.mark.parametrize("kind", ["random", "extreme"])
@pytest.mark.parametrize("n", [1, 2, 16, 256, 512, 4096, 8192, 1 << 20, 1 << 21, 1 << 22, 1 << 24])
def test_prefix_sums_and_products_directly(hal, orc, n, kind):
    rng = np.random.default_rng([n, len(kind)])
    w = _words(rng, n, kind)
    buf = hal.copy_from(w)
    hal.prefix_sums(buf, n)
    want = (np.cumsum(w.reshape(n, 4).astype(np.int64), axis=0) % P).astype(np.uint32).reshape(-1)  # (Montgomery form is linear)
    assert np.array_equal(buf.to_host(), want)
    buf.upload(w)
    hal.prefix_products(buf, n)
    got = buf.to_host()
    buf.free()
    assert np.array_equal(got, orc.prefix_products(w, n))
    if n <= 4096:
        assert np.array_equal(got, _py_products(w))
