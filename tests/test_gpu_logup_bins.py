"""The counting kernel's histogram layout (csrc/logup.hip: one launch per table and half of its 65,536 values, 32,768 LDS bins a
workgroup, flushed by 1,024 threads bin by bin; zero counted by subtraction, gated-off slots on their own) at the values where that
layout can go wrong: every enabled lookup of a table on ONE value at the edges of a half and of the table, everything zero, everything
that can be gated off gated off, and two values either side of each boundary alternating by row.  The device's columns are compared
with the exact reference and the host count; every column sums to the table's enabled slots (its slot count where nothing is gated)."""
import functools

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import logup_circuits as lc
import logup_ref as ref
from test_gpu_logup import TABLED, device_multiplicities
from test_logup import ERROR_SEED, host_multiplicities

pytestmark = pytest.mark.gpu
P = ref.P
CIRCUITS = [("seed %d" % s, s) for s in TABLED] + [("error circuit", None)]
ONE_VALUE = [1, 4095, 4096, 32767, 32768, 65535]   # a 16-bit table index; the AND table's is a + 256 b: 65535 is the pair (255, 255)
# the boundaries of the layout: the two halves (32767 | 32768); the flush's stride of 1,024 bins (1023 | 1024, and the same in the
# upper half: 33791 | 33792); zero, which is not binned, beside the first bin (0 | 1); the last bin beside zero (65535 | 0)
STRADDLE = [(32767, 32768), (1023, 1024), (33791, 33792), (0, 1), (65535, 0)]
WITNESSES = [("all %d" % v, v) for v in ONE_VALUE] + [("all zero", 0), ("all gated off", "gated")] + [("%d and %d by row" % p, p) for p in STRADDLE]


@functools.lru_cache(maxsize=None)
def circuit(seed):
    return lc.generate(ERROR_SEED, tables=[1, 2], n_chain=4) if seed is None else lc.generate(seed)


@pytest.fixture(scope="module")
def loaded(hal):
    """the circuits loaded once for the module (loading compiles a circuit's kernels)"""
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = hal.load_circuit(circuit(seed).words)
        return cache[seed]
    yield get
    for gc in cache.values():
        gc.free()


@functools.lru_cache(maxsize=4)
def base_witness(seed, po2):
    """the generator's witness, decoded: (canonical DATA matrix, public inputs as Montgomery words, the same as canonical ints)"""
    data, glob, _ = circuit(seed).witness(po2, seed=2)
    return ref.dec(data).reshape(-1, 1 << po2).astype(np.int64), glob, [int(x) for x in ref.dec(glob)]


def witness_with(seed, po2, what):
    """c.witness with every enabled lookup's value chosen: `what` is one table index, a pair of them (even rows, odd rows) or "gated":
    every selector set so that its gated lookups are off (an ungated lookup, and a gate whose selector another lookup needs the other
    way round, looks up zero)"""
    n, c = 1 << po2, circuit(seed)
    m, glob, gl = base_witness(seed, po2)
    m = m.copy()
    value = 0
    if what == "gated":
        for i in range(lc.N_SEL):
            kinds = {g[0] for _, g, _ in c.lookups if g is not None and g[1] == i}
            if kinds:
                m[c.sel[i]] = 1 if "not" in kinds else 0
    elif isinstance(what, tuple):
        value = np.where(np.arange(n) % 2 == 0, what[0], what[1])
    else:
        value = what
    v = np.broadcast_to(np.asarray(value, dtype=np.int64), (n,))
    for kind, gate, cols in c.lookups:
        on = np.ones(n, dtype=bool) if gate is None else (m[c.sel[gate[1]]] == 1) == (gate[0] == "sel")
        if kind == 1:
            pivot, k_p, rest = cols
            r = rest.evaluate(m, None, gl) if rest.t else 0
            m[pivot] = (np.where(on, v, 65536 + v) - r) % P * pow(k_p, P - 2, P) % P   # gated off: outside the table
        else:
            a, b, r = cols
            m[a], m[b] = v & 255, v >> 8
            m[r] = np.where(on, m[a] & m[b], (m[a] & m[b]) ^ 1)                          # gated off: not a & b
    return ref.enc(m).reshape(-1), glob


@pytest.mark.parametrize("po2", [16, 17])
@pytest.mark.parametrize("name,what", WITNESSES, ids=[w[0] for w in WITNESSES])
@pytest.mark.parametrize("label,seed", CIRCUITS, ids=[c[0] for c in CIRCUITS])
def test_multiplicities_at_the_edges_of_the_histogram_layout(hal, loaded, label, seed, name, what, po2):
    c = circuit(seed)
    n = 1 << po2
    data, glob = witness_with(seed, po2, what)
    looks = ref.lookups(c.words, po2, data, glob)
    enabled = {k: sum(int((num == 1).sum()) for t, num, _ in looks if t == k) for k in c.kinds}
    if what == "gated":     # only what cannot be gated off is left: the ungated lookups and, of a selector gated both ways, its "sel" side
        for k in c.kinds:
            assert enabled[k] == n * sum(1 for kind, g, _ in c.lookups if kind == k and (g is None or (g[0] == "sel" and _both_ways(c, g[1]))))
    elif not isinstance(what, tuple):   # the witness is what it is meant to be: every enabled lookup is on the one value
        for t, num, value in looks:
            want = what if t == 1 else ref.TAG_AND + what + 65536 * ((what & 255) & (what >> 8))
            assert np.all(value[num == 1] == want)
    want = ref.multiplicities(c.words, data, glob, po2)
    got = device_multiplicities(hal, loaded(seed), po2, data, glob)
    assert np.array_equal(got, want)
    assert np.array_equal(host_multiplicities(c.words, po2, data, glob), want)
    cols = ref.dec(got).reshape(-1, n)
    for k in c.kinds:
        assert int(cols[c.mult[k]].sum()) == enabled[k]
        assert not cols[c.mult[k], 65536:].any()
        if not isinstance(what, (tuple, str)):
            assert int(cols[c.mult[k], what]) == enabled[k]


def _both_ways(c, i):
    return len({g[0] for _, g, _ in c.lookups if g is not None and g[1] == i}) == 2


@pytest.mark.parametrize("case", ["numerator 2", "outside R16", "outside AND"])
def test_the_contract_errors_with_every_other_lookup_in_the_upper_half(hal, loaded, case):
    """the error bits are set by the launches of both halves; here every well-formed lookup is binned by the second one"""
    c = circuit(None)
    n = 1 << 16
    data, glob = witness_with(None, 16, 32768 + 255)
    d = data.reshape(-1, n).copy()
    if case == "numerator 2":
        for s in c.sel:
            d[s, 5] = ref.enc(2)
    elif case == "outside R16":
        cols = next(x for x in c.lookups if x[1] is None and x[0] == 1)[2]
        d[cols[0], 7] = ref.enc((int(ref.dec(d[cols[0], 7])) + 65536 * pow(cols[1], P - 2, P)) % P)
    else:
        cols = next(x for x in c.lookups if x[1] is None and x[0] == 2)[2]
        d[cols[2], 9] = ref.enc(int(ref.dec(d[cols[2], 9])) ^ 1)
    with pytest.raises(ref.LogupError):
        ref.multiplicities(c.words, d.reshape(-1), glob, 16)
    gc = loaded(None)
    with pytest.raises(r0.R0HipError, match="neither 0 nor 1" if case == "numerator 2" else "not in its table"):
        device_multiplicities(hal, gc, 16, d.reshape(-1), glob)
    assert np.array_equal(device_multiplicities(hal, gc, 16, data, glob), ref.multiplicities(c.words, data, glob, 16))
