"""logup_term_kernel inverts once per batch of up to four accumulators (fp4_batch_div, csrc/fp.hpp): table-less generated circuits whose
chain and whose public accumulators fill whole batches, partial ones and several, at the small scan shapes -- ACCUM and the public totals
against the oracle and the exact reference -- and witnesses on which some but not all denominators of a batch are zero (a zero
denominator gives a zero term, as fp4_inv(0) == 0 does: tests/logup_ref.py `_term`)."""
import functools

import numpy as np
import pytest

import logup_circuits as lc
import logup_ref as ref

pytestmark = pytest.mark.gpu
P = ref.P
N_CHAIN = [1, 2, 3, 4, 5, 8, 9]


@functools.lru_cache(maxsize=None)
def generated(n_chain):
    """one to three public accumulators: 2, 3, 1, 2, 3, 3, 1 for the seven chain lengths"""
    return lc.generate(200 + n_chain, tables=[], n_chain=n_chain, n_public=1 + n_chain % 3)


@pytest.fixture(scope="module")
def loaded(hal, orc):
    """-> (device circuit, oracle circuit) of a chain length, loaded once for the module (loading compiles a circuit's kernels)"""
    cache = {}

    def get(n_chain):
        if n_chain not in cache:
            cache[n_chain] = (hal.load_circuit(generated(n_chain).words), orc.circuit(generated(n_chain).words))
        return cache[n_chain]
    yield get
    for gc, _ in cache.values():
        gc.free()


def check(hal, loaded, n_chain, po2, data, glob, mix):
    """totals and ACCUM of the device against the oracle's and the exact reference's"""
    c = generated(n_chain)
    gc, oc = loaded(n_chain)
    code = oc.witgen(po2, 0)[0]
    cb, db = hal.copy_from(code), hal.copy_from(data)
    want_glob = ref.totals(c.words, po2, code, data, glob)
    assert np.array_equal(oc.logup_totals(po2, code, data, glob), want_glob)
    assert np.array_equal(hal.logup_totals(gc, po2, cb, db, glob), want_glob)
    acc = hal.accum_public(gc, po2, cb, db, want_glob, mix)
    want = ref.accum(c.words, po2, code, data, want_glob, mix)
    assert np.array_equal(oc.accum_public(po2, code, data, want_glob, mix), want)
    assert np.array_equal(acc.to_host(), want)
    for buf in (acc, cb, db):
        buf.free()


@pytest.mark.parametrize("po2", [4, 8, 12])
@pytest.mark.parametrize("n_chain", N_CHAIN)
def test_accumulation_in_whole_and_partial_batches(hal, loaded, n_chain, po2):
    """chain links: 1, 2, 3 (one partial batch), 4 (one whole), 5 (4 + 1), 8 (4 + 4), 9 (4 + 4 + 1); the public accumulators are a batch
    of their own of one to three, launched from the middle of the tape"""
    data, glob, mix = generated(n_chain).witness(po2, seed=3)
    check(hal, loaded, n_chain, po2, data, glob, mix)


def zero_denominators(c, po2, code, data, glob, mix):
    """-> bool [accumulator][row]: one of the accumulator's four denominators is zero there (so d01 d23 is), from the reference's own
    evaluation of the forms"""
    pc = ref.parse(c.words)
    cols = ref.Columns(pc, po2, code, data, glob, mix)
    out = []
    for _, frs in pc["accs"]:
        zero = np.zeros(cols.n, dtype=bool)
        for f in frs:
            den = [np.zeros(cols.n, dtype=np.int64)] * 4
            for kind, idx, lf in f["parts"]:
                v = cols.form(lf)
                den = [(den[0] + v) % P] + den[1:] if kind == 0 else ref.add4(den, [v * int(e) % P for e in cols.challenge(kind, idx)])
            zero |= (den[0] == 0) & (den[1] == 0) & (den[2] == 0) & (den[3] == 0)
        out.append(zero)
    return np.array(out)


def batches(c):
    """[a, b) of every batch: the chain's launch and the public accumulators' launch each cut theirs from their first accumulator"""
    n_acc = c.n_chain + c.n_public
    return [(j, min(j + 4, c.n_chain)) for j in range(0, c.n_chain, 4)] + [(j, min(j + 4, n_acc)) for j in range(c.n_chain, n_acc, 4)]


# a mix of zeros (0 is one of EXTREME) makes every denominator that is a mix challenge alone zero on every row and leaves the others;
# the columns and public inputs come from EXTREME as in every witness of the generator.  (n_chain, which batch must be partly zero)
PARTLY_ZERO = [(9, 0), (9, 1), (8, 1), (4, 0), (2, 1)]


@pytest.mark.parametrize("n_chain,batch", PARTLY_ZERO)
@pytest.mark.parametrize("po2", [4, 8])
def test_some_but_not_all_denominators_of_a_batch_are_zero(hal, loaded, n_chain, batch, po2):
    c = generated(n_chain)
    data, glob, mix = c.witness(po2, seed=3)
    mix = np.zeros_like(mix)
    code = loaded(n_chain)[1].witgen(po2, 0)[0]
    zero = zero_denominators(c, po2, code, data, glob, mix)   # the condition, from the reference alone
    a, b = batches(c)[batch]
    per_row = zero[a:b].sum(axis=0)
    assert np.any((per_row > 0) & (per_row < b - a)), "no row on which batch [%d, %d) is partly zero" % (a, b)
    check(hal, loaded, n_chain, po2, data, glob, mix)
