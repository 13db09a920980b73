"""The transcript generators and slice hashes of both hash suites restated in Python: the norm the device transcript (r0h_iop_*,
csrc/iop.hip) is held to.  Written from the comment block at the top of csrc/hash_suite.cpp and the host generators below it; no
product code.  The Poseidon2 permutation is the oracle binding's `poseidon2_mix` (tests only); SHA-256 is the compression below,
pinned against hashlib (tests/test_iop_ref.py), where the generator is also compared with tests/sha_suite_ref.py's Sha256Rng.

A generator's `state()` is what r0h_iop_set_state / r0h_iop_state carry: its words as the host holds them, then pool_used.
  Poseidon2   24 cells (Montgomery form), pool_used.  mix(d): permute first when pool_used != 0; cells[0..7] += d mod p; permute;
              pool_used = 0.  elem: permute and reset when pool_used == 16; cells[pool_used++].  bits(n): ALWAYS four elements, decoded;
              the first that is not zero (zero if none), masked to n bits.
  SHA-256     pool0[8], pool1[8], pool_used.  mix(d): pool0 ^= d, step.  step: pool0 = H(pool0 || pool1), pool1 = H(pool0 || pool1) with
              the new pool0, pool_used = 0.  A word steps first when pool_used == 8.  elem folds six words, val = ((val << 32) + w) mod p,
              then Montgomery form.  bits(n): one word, masked.
  slice hash  Poseidon2: rate blocks of 16 words OVERWRITE cells 0..15 (the last zero-padded), one permutation per block, at least one;
              the digest is cells 0..7.  SHA-256: 16-word blocks chained from the IV, the last partial block zero-filled, no length block.
"""
import hashlib

import numpy as np

P = 2013265921
M32 = 0xFFFFFFFF
R_INV = pow(1 << 32, P - 2, P)

_K = [int(x) for x in (
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
    0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
    0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
    0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
    0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
    0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2)]
SHA_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def enc(x):
    return (int(x) << 32) % P


def dec(x):
    return int(x) * R_INV % P


def _rotr(x, n):
    return ((x >> n) | (x << (32 - n))) & M32


def sha_compress(state, message):
    """FIPS 180-4: one compression of `state` (8 words) over `message` (16 words), SHA-256's own word order"""
    w = [int(x) for x in message]
    for i in range(16, 64):
        s0 = _rotr(w[i - 15], 7) ^ _rotr(w[i - 15], 18) ^ (w[i - 15] >> 3)
        s1 = _rotr(w[i - 2], 17) ^ _rotr(w[i - 2], 19) ^ (w[i - 2] >> 10)
        w.append((w[i - 16] + s0 + w[i - 7] + s1) & M32)
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        t1 = (h + (_rotr(e, 6) ^ _rotr(e, 11) ^ _rotr(e, 25)) + ((e & f) ^ (~e & M32 & g)) + _K[i] + w[i]) & M32
        t2 = ((_rotr(a, 2) ^ _rotr(a, 13) ^ _rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c))) & M32
        h, g, f, e, d, c, b, a = g, f, e, (d + t1) & M32, c, b, a, (t1 + t2) & M32
    return [(x + y) & M32 for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def _bswap(x):
    return int.from_bytes(int(x).to_bytes(4, "little"), "big")


def sha_hash_pair(a, b):
    words = [int(x) for x in a] + [int(x) for x in b]
    return [_bswap(s) for s in sha_compress(SHA_IV, [_bswap(x) for x in words])]


def sha_hash_elems(words):
    words = [int(x) for x in words]
    state = list(SHA_IV)
    for at in range(0, len(words), 16):
        block = words[at:at + 16]
        state = sha_compress(state, [_bswap(x) for x in block + [0] * (16 - len(block))])
    return np.array([_bswap(s) for s in state], dtype=np.uint32)


def p2_hash_elems(orc, words):
    words = [int(x) for x in words]
    cells = np.zeros(24, dtype=np.uint32)
    for at in range(0, max(len(words), 1), 16):
        block = words[at:at + 16]
        cells[:16] = block + [0] * (16 - len(block))
        cells = orc.poseidon2_mix(cells)
    return cells[:8].copy()


class P2Rng:
    STATE_WORDS, POOL_LIMIT = 25, 16

    def __init__(self, orc, state=None):
        self.orc = orc
        self.cells = np.zeros(24, dtype=np.uint32)
        self.used = 0
        if state is not None:
            self.cells, self.used = np.array(state[:24], dtype=np.uint32), int(state[24])

    def _permute(self):
        self.cells = self.orc.poseidon2_mix(self.cells)
        self.used = 0

    def mix(self, digest):
        if self.used != 0:
            self._permute()
        for i in range(8):
            self.cells[i] = (int(self.cells[i]) + int(digest[i])) % P
        self._permute()

    def elem(self):
        if self.used == 16:
            self._permute()
        self.used += 1
        return int(self.cells[self.used - 1])

    def bits(self, n):
        val = dec(self.elem())
        for _ in range(3):
            nv = dec(self.elem())
            if val == 0:
                val = nv
        return val & ((1 << n) - 1)

    def hash_elems(self, words):
        return p2_hash_elems(self.orc, words)

    def state(self):
        return np.concatenate([self.cells, [self.used]]).astype(np.uint32)


class ShaRng:
    STATE_WORDS, POOL_LIMIT = 17, 8

    def __init__(self, orc=None, state=None):
        self.pool0 = [int(x) for x in np.frombuffer(hashlib.sha256(b"Hello").digest(), dtype="<u4")]
        self.pool1 = [int(x) for x in np.frombuffer(hashlib.sha256(b"World").digest(), dtype="<u4")]
        self.used = 0
        if state is not None:
            self.pool0, self.pool1, self.used = [int(x) for x in state[:8]], [int(x) for x in state[8:16]], int(state[16])

    def _step(self):
        self.pool0 = sha_hash_pair(self.pool0, self.pool1)
        self.pool1 = sha_hash_pair(self.pool0, self.pool1)
        self.used = 0

    def word(self):
        if self.used == 8:
            self._step()
        self.used += 1
        return self.pool0[self.used - 1]

    def mix(self, digest):
        self.pool0 = [a ^ int(b) for a, b in zip(self.pool0, digest)]
        self._step()

    def elem(self):
        val = 0
        for _ in range(6):
            val = ((val << 32) + self.word()) % P
        return enc(val)

    def bits(self, n):
        return self.word() & ((1 << n) - 1)

    def hash_elems(self, words):
        return sha_hash_elems(words)

    def state(self):
        return np.array(self.pool0 + self.pool1 + [self.used], dtype=np.uint32)


def make_rng(hashfn, orc, state=None):
    return ShaRng(orc, state) if hashfn == "sha-256" else P2Rng(orc, state)


def commit_elems(rng, words):
    rng.mix(rng.hash_elems(words))


def draw_ext(rng, count):
    return np.array([rng.elem() for _ in range(4 * count)], dtype=np.uint32)


def draw_queries(rng, domain, tree_rows, n_queries):
    """the loop of the sequencer's query step (csrc/prover.hip `queries`): the table [n_trees][n_queries]"""
    log_domain = domain.bit_length() - 1
    assert 1 << log_domain == domain
    idx = np.zeros((len(tree_rows), n_queries), dtype=np.uint32)
    for q in range(n_queries):
        pos = rng.bits(log_domain) % domain
        for t, rows in enumerate(tree_rows):
            if t >= 4:
                pos %= rows
            idx[t, q] = pos
    return idx
