"""The transcript on the device (r0h_iop_*, csrc/iop.hip) against tests/iop_ref.py under both hash suites: every operation's words and
the generator's state after it; the corners a random seal never shows, on planted states; the refusals, by message; and
r0h_fri_fold_buf against r0h_fri_fold."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import iop_ref

pytestmark = pytest.mark.gpu
P = iop_ref.P
SUITES = ["poseidon2", "sha-256"]


@pytest.fixture(scope="module")
def hals():
    made = {}
    for name in SUITES:
        made[name] = r0.Hal(0)
        made[name].set_hashfn(name)
    yield made
    for h in made.values():
        h.close()


def words(seed, n, below=P):
    return np.random.default_rng(seed).integers(0, below, n, dtype=np.uint64).astype(np.uint32)


def planted(hashfn, seed, used, zeros=()):
    """a generator state of the suite: random canonical words, the given pool_used, zeros where asked"""
    n = iop_ref.make_rng(hashfn, None).STATE_WORDS
    st = words(seed, n, P if hashfn == "poseidon2" else 1 << 32)
    st[:n - 1][st[:n - 1] == 0] = 1
    for z in zeros:
        st[z] = 0
    st[n - 1] = used
    return st


def digest(hashfn, seed):
    return words(seed, 8, P if hashfn == "poseidon2" else 1 << 32)


def same_state(iop, ref):
    assert np.array_equal(iop.state(), ref.state())


@pytest.mark.parametrize("hashfn", SUITES)
def test_a_fresh_states_first_draws(hals, orc, hashfn):
    hal, ref = hals[hashfn], iop_ref.make_rng(hashfn, orc)
    iop, out = hal.iop(), hal.alloc(64)
    same_state(iop, ref)
    iop.draw_ext(out, 4, 3)
    assert np.array_equal(out.to_host(4, 12), iop_ref.draw_ext(ref, 3))
    same_state(iop, ref)
    iop.free(), out.free()


@pytest.mark.parametrize("hashfn", SUITES)
def test_commit_with_the_pool_untouched_and_with_it_used(hals, orc, hashfn):
    hal, ref = hals[hashfn], iop_ref.make_rng(hashfn, orc)
    iop, out = hal.iop(), hal.alloc(16)
    buf = hal.copy_from(np.concatenate([digest(hashfn, 1), digest(hashfn, 2), digest(hashfn, 3)]))
    iop.commit(buf, 8)  # pool_used == 0
    ref.mix(digest(hashfn, 2))
    same_state(iop, ref)
    iop.draw_ext(out, 0, 1)  # pool_used != 0 from here on
    assert np.array_equal(out.to_host(0, 4), iop_ref.draw_ext(ref, 1))
    iop.commit(buf, 16)
    ref.mix(digest(hashfn, 3))
    same_state(iop, ref)
    iop.commit(buf, 0)
    ref.mix(digest(hashfn, 1))
    iop.draw_ext(out, 8, 2)
    assert np.array_equal(out.to_host(8, 8), iop_ref.draw_ext(ref, 2))
    same_state(iop, ref)
    for b in (iop, out, buf):
        b.free()


@pytest.mark.parametrize("hashfn", SUITES)
def test_draws_in_a_row_with_a_refill_inside(hals, orc, hashfn):
    """five extension elements are 20 field elements: more than the 17 that refill a Poseidon2 pool of 16 from its start, and 120 words
    of the SHA-256 pool of eight (9 already step it).  From pool_used = 0, from a pool one short of its end and from one used up."""
    hal = hals[hashfn]
    limit = iop_ref.make_rng(hashfn, None).POOL_LIMIT
    for used in (0, limit - 1, limit):
        st = planted(hashfn, 10 + used, used)
        ref = iop_ref.make_rng(hashfn, orc, st)
        iop, out = hal.iop(), hal.alloc(20)
        iop.set_state(st)
        iop.draw_ext(out, 0, 5)  # 20 elements
        assert np.array_equal(out.to_host(), iop_ref.draw_ext(ref, 5))
        same_state(iop, ref)
        iop.free(), out.free()


def one_bits(hal, st, n_bits):
    """bits(n_bits) of the generator at state `st`, through the query loop with one tree and one query; and the state after it"""
    iop, out = hal.iop(), hal.alloc(4)
    iop.set_state(st)
    iop.draw_queries(1 << n_bits, [1 << n_bits], 1, out, 2)
    got = int(out.to_host(2, 1)[0])
    after = iop.state()
    iop.free(), out.free()
    return got, after


@pytest.mark.parametrize("case,used,zeros", [("first", 0, (0,)), ("first three", 0, (0, 1, 2)), ("all four", 0, (0, 1, 2, 3)), ("behind others", 5, (5, 6)),
                                             ("straddle", 14, ()), ("straddle, zeros before the refill", 14, (14, 15)), ("at the end", 16, ())])
def test_poseidon2_bits_over_planted_states(hals, orc, case, used, zeros):
    """what a random seal never shows (a decoded zero has chance 2^-31): the first decoded draw is zero, the first three, all four;
    and four draws that straddle a refill"""
    st = planted("poseidon2", 40 + used + len(zeros), used, zeros)
    for n_bits in (11, 19):
        ref = iop_ref.P2Rng(orc, st)
        want = ref.bits(n_bits)
        got, after = one_bits(hals["poseidon2"], st, n_bits)
        assert got == want and np.array_equal(after, ref.state()), case
        if case == "all four":
            assert got == 0


@pytest.mark.parametrize("used", [0, 7, 8])
def test_sha256_bits_over_planted_states(hals, used):
    st = planted("sha-256", 60 + used, used)
    for n_bits in (11, 19):
        ref = iop_ref.ShaRng(None, st)
        want = ref.bits(n_bits)
        got, after = one_bits(hals["sha-256"], st, n_bits)
        assert got == want and np.array_equal(after, ref.state())


@pytest.mark.parametrize("hashfn", SUITES)
def test_commit_elems_at_block_edges_read_at_an_offset(hals, orc, hashfn):
    hal = hals[hashfn]
    w = words(5, 1024 + 37)
    buf = hal.copy_from(w)
    for n, at in ((1, 3), (15, 1), (16, 7), (17, 37), (32, 5), (128, 33), (1024, 37), (0, 9)):
        st = planted(hashfn, 70 + n, 3)
        ref = iop_ref.make_rng(hashfn, orc, st)
        iop = hal.iop()
        iop.set_state(st)
        iop.commit_elems(buf, at, n)
        iop_ref.commit_elems(ref, w[at:at + n])
        same_state(iop, ref)
        iop.free()
    buf.free()


@pytest.mark.parametrize("hashfn", SUITES)
@pytest.mark.parametrize("domain,rows", [(1 << 11, [1 << 11] * 4 + [1 << 7]), (1 << 19, [1 << 19] * 4 + [1 << 15, 1 << 11, 1 << 7])])
def test_draw_queries_is_the_host_loop(hals, orc, hashfn, domain, rows):
    hal, ref = hals[hashfn], iop_ref.make_rng(hashfn, orc)
    iop, out = hal.iop(), hal.alloc(len(rows) * 50 + 6)
    d = hal.copy_from(digest(hashfn, 9))
    iop.commit(d, 0)
    ref.mix(digest(hashfn, 9))
    iop.draw_queries(domain, rows, 50, out, 6)
    want = iop_ref.draw_queries(ref, domain, rows, 50)
    got = out.to_host(6, len(rows) * 50).reshape(len(rows), 50)
    assert np.array_equal(got, want)
    assert all(int(got[t].max()) < rows[t] for t in range(len(rows))) and len(set(got[0])) > 40
    same_state(iop, ref)
    for b in (iop, out, d):
        b.free()


@pytest.mark.parametrize("hashfn", SUITES)
def test_a_sequence_of_everything(hals, orc, hashfn):
    """the tail of a proof in small: per round a commit and a fold mix, the final coefficients, the query table"""
    hal, ref = hals[hashfn], iop_ref.make_rng(hashfn, orc, planted(hashfn, 90, 4))
    iop, out = hal.iop(), hal.alloc(8 + 6 * 50)
    iop.set_state(planted(hashfn, 90, 4))
    w = words(11, 256)
    roots = np.concatenate([digest(hashfn, 20), digest(hashfn, 21)])
    buf, rbuf = hal.copy_from(w), hal.copy_from(roots)
    for r in range(2):
        iop.commit(rbuf, 8 * r)
        iop.draw_ext(out, 4 * r, 1)
        ref.mix(roots[8 * r:8 * r + 8])
        assert np.array_equal(out.to_host(4 * r, 4), iop_ref.draw_ext(ref, 1))
    iop.commit_elems(buf, 0, 256)
    iop_ref.commit_elems(ref, w)
    rows = [1 << 13] * 4 + [1 << 9, 1 << 5]
    iop.draw_queries(1 << 13, rows, 50, out, 8)
    assert np.array_equal(out.to_host(8, 300).reshape(6, 50), iop_ref.draw_queries(ref, 1 << 13, rows, 50))
    same_state(iop, ref)
    for b in (iop, out, buf, rbuf):
        b.free()


def test_refusals_by_message(hals):
    p2, sha = hals["poseidon2"], hals["sha-256"]
    iop, siop, buf = p2.iop(), sha.iop(), p2.alloc(16)
    good = planted("poseidon2", 1, 3)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_set_state: the poseidon2 generator's state is 25 words, not 17"):
        iop.set_state(good[:17])
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_set_state: the sha-256 generator's state is 17 words, not 25"):
        siop.set_state(good)
    bad = good.copy()
    bad[23] = P
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_set_state: cell 23 is not a canonical field element"):
        iop.set_state(bad)
    bad = good.copy()
    bad[24] = 17
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_set_state: pool_used 17 is above 16"):
        iop.set_state(bad)
    bad = planted("sha-256", 1, 9)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_set_state: pool_used 9 is above 8"):
        siop.set_state(bad)
    siop.set_state(planted("sha-256", 1, 8))  # (cells of any 32-bit value, a pool used up: fine)
    iop.set_state(planted("poseidon2", 1, 16))
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_commit: words \[9, \+8\) outside a buffer of 16 words"):
        iop.commit(buf, 9)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_commit_elems: words \[4, \+13\) outside a buffer of 16 words"):
        iop.commit_elems(buf, 4, 13)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_draw_ext: words \[13, \+4\) outside a buffer of 16 words"):
        iop.draw_ext(buf, 13, 1)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_draw_queries: words \[0, \+20\) outside a buffer of 16 words"):
        iop.draw_queries(1 << 11, [1 << 11] * 4 + [1 << 7], 4, buf, 0)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_draw_queries: domain 1000 is not a power of two"):
        iop.draw_queries(1000, [1000], 1, buf, 0)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_draw_queries: tree 4 has no rows"):
        iop.draw_queries(1 << 11, [1 << 11] * 4 + [0], 1, buf, 0)
    with pytest.raises(r0.R0HipError, match=r"r0h_iop_draw_queries: 17 trees outside \[1, 16\]"):
        iop.draw_queries(1 << 11, [1 << 11] * 17, 1, buf, 0)
    # a transcript belongs to the suite it was made under: refused, with both names, once its context is on another
    before = iop.state()
    p2.set_hashfn("sha-256")
    try:
        for call in (lambda: iop.commit(buf, 0), lambda: iop.state(), lambda: iop.draw_ext(buf, 0, 1), lambda: iop.set_state(good)):
            with pytest.raises(r0.R0HipError, match=r"r0h_iop_\w+: the transcript was made under the poseidon2 hash suite, its context is now on sha-256"):
                call()
    finally:
        p2.set_hashfn("poseidon2")
    assert np.array_equal(iop.state(), before)
    for b in (iop, siop, buf):
        b.free()


@pytest.mark.parametrize("n_out", [1, 255, 256, 257, 4096])
def test_fri_fold_buf_is_fri_fold(hal, n_out):
    inp = hal.copy_from(words(n_out, 64 * n_out))
    mixes = words(3, 16)
    mbuf = hal.copy_from(mixes)
    want, got = hal.alloc(4 * n_out), hal.alloc(4 * n_out)
    for at in (0, 12):
        hal.fri_fold(want, inp, mixes[at:at + 4], n_out)
        hal.zero(got)
        hal.fri_fold_buf(got, inp, mbuf, at, n_out)
        assert np.array_equal(got.to_host(), want.to_host())
    with pytest.raises(r0.R0HipError, match=r"r0h_fri_fold_buf: the mix at words \[13, \+4\) ends beyond a buffer of 16 words"):
        hal.fri_fold_buf(got, inp, mbuf, 13, n_out)
    for b in (inp, mbuf, want, got):
        b.free()
