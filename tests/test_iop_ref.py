"""tests/iop_ref.py, the reference of the device transcript, held to what it is written from -- without a GPU: its SHA-256 compression
against hashlib, its SHA-256 generator against tests/sha_suite_ref.py's Sha256Rng on a fixed operation sequence, both slice hashes
against the library's host suites (r0h_hash_elems_host), and the Poseidon2 generator's documented corners on planted states."""
import hashlib

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import iop_ref
import sha_suite_ref

P = iop_ref.P


def _padded(msg):
    bits = 8 * len(msg)
    msg = msg + b"\x80" + b"\x00" * ((55 - len(msg)) % 64) + bits.to_bytes(8, "big")
    return [int.from_bytes(msg[i:i + 4], "big") for i in range(0, len(msg), 4)]


@pytest.mark.parametrize("msg", [b"", b"abc", b"Hello", bytes(range(200))])
def test_the_compression_is_sha256s(msg):
    state, words = list(iop_ref.SHA_IV), _padded(msg)
    for at in range(0, len(words), 16):
        state = iop_ref.sha_compress(state, words[at:at + 16])
    assert b"".join(s.to_bytes(4, "big") for s in state) == hashlib.sha256(msg).digest()


def test_the_sha_generator_is_sha_suite_refs_on_a_fixed_sequence():
    a, b = iop_ref.ShaRng(), sha_suite_ref.Sha256Rng()
    rng = np.random.default_rng(7)
    assert list(a.state()[:16]) == list(b.pool0) + list(b.pool1)
    for step in range(40):
        op = step % 4
        if op == 0:
            d = rng.integers(0, 1 << 32, 8, dtype=np.uint64).astype(np.uint32)
            a.mix(d), b.mix(d)
        elif op == 1:
            assert [a.elem() for _ in range(5)] == [b.random_elem() for _ in range(5)]
        elif op == 2:
            assert [a.bits(n) for n in (1, 11, 19, 32)] == [b.random_bits(n) for n in (1, 11, 19, 32)]
        else:
            w = rng.integers(0, P, int(rng.integers(0, 70)), dtype=np.uint64).astype(np.uint32)
            assert np.array_equal(a.hash_elems(w), sha_suite_ref.hash_elem_slice(w))
        assert list(a.state()) == [int(x) for x in b.pool0] + [int(x) for x in b.pool1] + [b.used]
    assert a.state().size == iop_ref.ShaRng.STATE_WORDS


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 32, 128, 1024])
def test_the_slice_hashes_are_the_librarys_host_suites(orc, n):
    w = np.random.default_rng(n).integers(0, P, n, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(iop_ref.p2_hash_elems(orc, w), r0.hash_elems_host("poseidon2", w))
    assert np.array_equal(iop_ref.sha_hash_elems(w), r0.hash_elems_host("sha-256", w))


def test_the_poseidon2_generators_corners(orc):
    rng = np.random.default_rng(3)
    cells = rng.integers(1, P, 24, dtype=np.uint64).astype(np.uint32)
    # mix with pool_used != 0 permutes first: two permutations, against one from a fresh pool
    d = rng.integers(0, P, 8, dtype=np.uint64).astype(np.uint32)
    g = iop_ref.P2Rng(orc, list(cells) + [5])
    g.mix(d)
    once = orc.poseidon2_mix(cells)
    once[:8] = (once[:8].astype(np.uint64) + d) % P
    assert np.array_equal(g.cells, orc.poseidon2_mix(once)) and g.used == 0
    # bits always takes four elements and keeps the first decoded value that is not zero
    for zeros, want_from in ((1, 1), (3, 3), (4, None)):
        planted = cells.copy()
        planted[:zeros] = 0
        g = iop_ref.P2Rng(orc, list(planted) + [0])
        want = 0 if want_from is None else iop_ref.dec(planted[want_from]) & 0x7FF
        assert g.bits(11) == want and g.used == 4
    # four draws from pool_used = 14 straddle a refill
    planted = cells.copy()
    planted[14:16] = 0
    g = iop_ref.P2Rng(orc, list(planted) + [14])
    assert g.bits(19) == iop_ref.dec(orc.poseidon2_mix(planted)[0]) & 0x7FFFF and g.used == 2
