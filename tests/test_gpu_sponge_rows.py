"""The rows of the in-circuit sponge made on the device (csrc/sponge.hip sponge_rows_kernel behind r0h_sponge_trace_device) against the
host's (r0h_sponge_trace, itself pinned to the oracle's and the generator's by tests/test_recursion.py): every word, at the smallest
shapes at which a lane-per-row kernel can go wrong -- a single partial block, the last rows of the trace unused, a trace filled to its
last full permutation, and a real lift's size across many workgroups.  The planted path (r0h_lift / r0h_join / the image proof) is
held to the oracle word for word by tests/test_recursion.py::test_lift_and_join_on_the_device and tests/test_gpu_session.py."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0

P = 2013265921


def _words(count, seed):
    return np.random.default_rng(seed).integers(0, P, count).astype(np.uint32)


def _device_rows(hal, words, po2):
    """into a buffer full of 0xFFFFFFFF: the rows behind the sponge must come back zero, written by the launch itself"""
    n = r0.SPONGE_DATA_COLUMNS << po2
    buf = hal.copy_from(np.full(n, 0xFFFFFFFF, dtype=np.uint32))
    try:
        return hal.sponge_trace_device(words, po2, out=buf)
    finally:
        buf.free()


@pytest.mark.gpu
@pytest.mark.parametrize("po2,count", [(6, 0), (6, 1), (6, 15), (6, 16), (6, 17), (6, 32),  # 1, 1, 1, 1, 2, 2 permutations: at most 60 of 64 rows
                                       (10, 16 * 33 + 1), (10, 16 * 34),                    # 34 permutations: 1,020 of 1,024 rows, the last full block
                                       (17, 50000)])                                       # a real lift's size: 3,125 permutations over 512 workgroups
def test_device_rows_equal_the_hosts(hal, po2, count):
    words = _words(count, 1000 * po2 + count)
    want = r0.sponge_trace(words, po2)
    got = _device_rows(hal, words, po2)
    used = 30 * max(1, -(-count // 16))
    assert got.shape == want.shape == (65, 1 << po2)
    assert not got[:, used:].any() and got[64, :used].all()
    assert np.array_equal(got, want)
    assert np.array_equal(got[:8, used - 1], r0.seal_digest(words))  # the state after the last round is the sponge's digest


@pytest.mark.gpu
def test_device_rows_refuse_what_the_host_refuses_in_the_same_words(hal):
    for words, match in ((np.zeros(16 * 35, dtype=np.uint32), "560 words take 1050 rows, the trace has 2\\^10"),
                         (np.array([P], dtype=np.uint32), "word 0 is not a canonical field element")):
        with pytest.raises(r0.R0HipError, match="r0h_sponge_trace: " + match):
            r0.sponge_trace(words, 10)
        with pytest.raises(r0.R0HipError, match="r0h_sponge_trace_device: " + match):
            hal.sponge_trace_device(words, 10)
    small = hal.alloc(65 << 9)
    with pytest.raises(r0.R0HipError, match="exceed the output buffer"):
        hal.sponge_trace_device(np.zeros(4, dtype=np.uint32), 10, out=small)
    small.free()
