"""The SHA-256 hash suite restated in Python / numpy: the norm the library's second suite is held to (no product code, no oracle).

Recalled from risc0-zkp core/hash/sha (`Sha256HashSuite`, `Sha256Rng`) and risc0-sys sha256.h; unpinned, like everything risc0-specific
in this repository (the reference vendors neither crate), so within the repository THIS file is what "the SHA-256 suite" means:

  digest          eight u32 words; word j = bswap32(SHA-256 state word j): the digest's bytes in memory are the standard big-endian
                  digest.  Message word i of a compression = bswap32(input word i).
  hash_pair       one compression of the IV over the 16 words a || b; no padding, no length
  hash_elem_slice risc0 `hash_raw_data_slice`: 16-word blocks chained from the IV, the last partial block zero-filled, no length block,
                  over the 32-bit words as they are stored (Montgomery form); the empty slice gives the IV as a digest
  Sha256Rng       pool0 = SHA-256("Hello"), pool1 = SHA-256("World"), ordinary padded hashes taken as digests; mix(d): pool0 ^= d, step;
                  step: pool0 = hash_pair(pool0, pool1), pool1 = hash_pair(pool0, pool1), used = 0; random_u32 steps first when eight
                  words are used up; random_bits(b) = random_u32 & (2^b - 1); a field element folds six draws
                  val = ((val << 32) + next) mod p (then Montgomery form); an extension element is four field elements

and a transcript replayer (`replay_seal`) that walks a seal in the order csrc/prover.hip writes it, feeds every commitment to the
generator, draws the challenges, derives the query positions and recomputes every Merkle opening up to the committed top layer.
"""
import hashlib

import numpy as np

P = 2013265921
QUERIES, INV_RATE, FRI_FOLD, FRI_MIN_DEGREE, CHECK_SIZE = 50, 4, 16, 256, 16
M32 = 0xFFFFFFFF

K = [0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
     0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
     0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
     0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
     0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
     0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]
IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _rotr(x, n):
    return (x >> n) | (x << (32 - n))  # Python ints: masked by the caller; numpy uint32: wraps by itself


def compress(state, message):
    """FIPS 180-4 compression: state (8) and message (16) are SHA-256's own words.  Works on Python ints and, element-wise, on numpy
    uint32 arrays of one shape (one hash per element)."""
    vec = isinstance(message[0], np.ndarray)
    m = (lambda x: x) if vec else (lambda x: x & M32)
    w = list(message)
    for i in range(16, 64):
        s0 = m(_rotr(w[i - 15], 7)) ^ m(_rotr(w[i - 15], 18)) ^ (w[i - 15] >> 3)
        s1 = m(_rotr(w[i - 2], 17)) ^ m(_rotr(w[i - 2], 19)) ^ (w[i - 2] >> 10)
        w.append(m(w[i - 16] + s0 + w[i - 7] + s1))
    a, b, c, d, e, f, g, h = state
    for i in range(64):
        kk = np.uint32(K[i]) if vec else K[i]
        t1 = m(h + (m(_rotr(e, 6)) ^ m(_rotr(e, 11)) ^ m(_rotr(e, 25))) + ((e & f) ^ (m(~e) & g)) + kk + w[i])
        t2 = m((m(_rotr(a, 2)) ^ m(_rotr(a, 13)) ^ m(_rotr(a, 22))) + ((a & b) ^ (a & c) ^ (b & c)))
        h, g, f, e, d, c, b, a = g, f, e, m(d + t1), c, b, a, m(t1 + t2)
    return [m(x + y) for x, y in zip(state, (a, b, c, d, e, f, g, h))]


def bswap(x):
    if isinstance(x, np.ndarray):
        return x.byteswap()
    return int.from_bytes(int(x).to_bytes(4, "little"), "big")


def _digest(state):
    return np.array([bswap(s) for s in state], dtype=np.uint32)


def hash_pair(a, b):
    words = [int(x) for x in a] + [int(x) for x in b]
    assert len(words) == 16
    return _digest(compress(IV, [bswap(x) for x in words]))


def hash_elem_slice(words):
    words = [int(x) for x in np.asarray(words, dtype=np.uint32).reshape(-1)]
    state = list(IV)
    for at in range(0, len(words), 16):
        block = words[at:at + 16]
        block += [0] * (16 - len(block))
        state = compress(state, [bswap(x) for x in block])
    return _digest(state)


def hash_rows(matrix, rows, cols):
    """digest of every row of a column-major [cols][rows] matrix: [rows, 8] (numpy, all rows at once)"""
    mat = np.asarray(matrix, dtype=np.uint32).reshape(-1)[:rows * cols].reshape(cols, rows)
    with np.errstate(over="ignore"):
        state = [np.full(rows, v, dtype=np.uint32) for v in IV]
        for at in range(0, cols, 16):
            block = [mat[c].byteswap() if c < cols else np.zeros(rows, dtype=np.uint32) for c in range(at, at + 16)]
            state = compress(state, block)
        return np.stack([s.byteswap() for s in state], axis=1)


def hash_fold(nodes, output_size):
    """nodes[i] = hash_pair(nodes[2i], nodes[2i+1]) for output_size <= i < 2 output_size, on a flat array of 8-word digests"""
    nodes = np.asarray(nodes, dtype=np.uint32).copy().reshape(-1, 8)
    pairs = nodes[2 * output_size:4 * output_size].reshape(output_size, 16)
    with np.errstate(over="ignore"):
        state = compress([np.full(output_size, v, dtype=np.uint32) for v in IV], [pairs[:, i].byteswap() for i in range(16)])
    nodes[output_size:2 * output_size] = np.stack([s.byteswap() for s in state], axis=1)
    return nodes.reshape(-1)


def merkle_build(matrix, rows, cols):
    """2 * rows digests: leaves at [rows, 2 rows), root at index 1 (index 0 unused, zero)"""
    nodes = np.zeros((2 * rows, 8), dtype=np.uint32)
    nodes[rows:] = hash_rows(matrix, rows, cols)
    nodes = nodes.reshape(-1)
    size = rows // 2
    while size >= 1:
        nodes = hash_fold(nodes, size)
        size //= 2
    return nodes


def enc(x):
    return (int(x) << 32) % P


def dec(x):
    return int(x) * pow(1 << 32, P - 2, P) % P


class Sha256Rng:
    def __init__(self):
        self.pool0 = np.frombuffer(hashlib.sha256(b"Hello").digest(), dtype="<u4").astype(np.uint32)
        self.pool1 = np.frombuffer(hashlib.sha256(b"World").digest(), dtype="<u4").astype(np.uint32)
        self.used = 0

    def step(self):
        self.pool0 = hash_pair(self.pool0, self.pool1)
        self.pool1 = hash_pair(self.pool0, self.pool1)
        self.used = 0

    def mix(self, digest):
        self.pool0 = self.pool0 ^ np.asarray(digest, dtype=np.uint32)
        self.step()

    def random_u32(self):
        if self.used == 8:
            self.step()
        self.used += 1
        return int(self.pool0[self.used - 1])

    def random_bits(self, bits):
        return self.random_u32() & ((1 << bits) - 1)

    def random_elem(self):
        val = 0
        for _ in range(6):
            val = ((val << 32) + self.random_u32()) % P
        return enc(val)

    def random_ext(self):
        return [self.random_elem() for _ in range(4)]


# ---------------------------------------------------------------- the circuit blob (include/r0hip_circuit.h), as far as a transcript needs it
def parse_blob(blob):
    w = [int(x) for x in np.asarray(blob, dtype=np.uint32)]
    assert w[0] == 0x31433052 and w[1] == 1
    c = {"info": b"R0HIP_SYNTH:v1__", "n_late": 0}
    pos = 3
    for _ in range(w[2]):
        tag, n = w[pos], w[pos + 1]
        p = w[pos + 2:pos + 2 + n]
        if tag == 1:
            c["group_size"] = p[:3]  # ACCUM, CODE, DATA
        elif tag == 2:
            c["n_taps"] = p[0]
        elif tag == 3:
            c["n_global"], c["n_mix"] = p[0], p[1]
        elif tag == 7:
            c["info"] = np.array(p, dtype="<u4").tobytes()
        elif tag == 9:
            c["n_late"] = p[0]
        pos += 2 + n
    return c


def _log2(x):
    n = 0
    while (1 << n) < x:
        n += 1
    return n


class _Tree:
    """What the seal says of one committed matrix: its top layer (the lowest layer of at most QUERIES digests, as MerkleShape in
    csrc/seal_layout.hpp chooses it), folded to the root here."""

    def __init__(self, seal, at, rows, cols):
        self.rows, self.cols = rows, cols
        layers, top_layer = _log2(rows), 0
        for i in range(1, layers):
            if (1 << i) > QUERIES:
                break
            top_layer = i
        self.top_size = 1 << top_layer
        self.top_at = at
        top = np.zeros(2 * self.top_size * 8, dtype=np.uint32)
        top[self.top_size * 8:] = seal[at:at + self.top_size * 8]
        assert seal[at:at + self.top_size * 8].size == self.top_size * 8, "seal truncated in a top layer"
        size = self.top_size // 2
        while size >= 1:
            top = hash_fold(top, size)
            size //= 2
        self.nodes = top.reshape(-1, 8)
        self.root = self.nodes[1]
        self.end = at + self.top_size * 8
        self.path = layers - top_layer
        self.opening_words = cols + 8 * self.path

    def check_opening(self, seal, at, row):
        """the opened row's leaf hash, folded with the path's siblings (left / right by the row's index), is the committed top-layer node"""
        values = seal[at:at + self.cols]
        cur = hash_elem_slice(values)
        node = row + self.rows
        at += self.cols
        while node >= 2 * self.top_size:
            sib = seal[at:at + 8]
            at += 8
            cur = hash_pair(sib, cur) if node & 1 else hash_pair(cur, sib)
            node >>= 1
        return bool(np.array_equal(self.nodes[node], cur))


def replay_seal(blob, seal):
    """Walk `seal` (of the circuit described by `blob`) as csrc/prover.hip wrote it under the SHA-256 suite.  Returns a dict:
    po2, roots (CODE, DATA, ACCUM, CHECK, then the FRI rounds), mix / poly_mix / z / deep_mix / fri_mix (the drawn challenges),
    positions (the QUERIES query rows), openings_ok / openings_total, first_bad (tree, query) or None, and `regions`: name -> (start, end)
    word ranges of the seal (globals, the four tops, coeff_u, each FRI top, final, openings) plus `opening` -> list of
    (tree, query, values start, path start, end)."""
    c = parse_blob(blob)
    seal = np.asarray(seal, dtype=np.uint32)
    rng = Sha256Rng()
    regions = {}
    rng.mix(hash_elem_slice([enc(b) for b in b"RISC0_STARK:v1__"]))
    rng.mix(hash_elem_slice([enc(b) for b in c["info"]]))
    n_global, n_late = c["n_global"], c["n_late"]
    glob = seal[:n_global + 1]
    po2 = dec(glob[n_global])
    assert 9 <= po2 <= 24, "the seal's po2 word reads %d" % po2
    rng.mix(hash_elem_slice(list(glob[:n_global - n_late]) + [glob[n_global]]))
    regions["globals"] = (0, n_global)
    pos = n_global + 1
    n, domain = 1 << po2, INV_RATE << po2
    trees, roots = {}, []

    def commit_tree(name, rows, cols):
        nonlocal pos
        t = _Tree(seal, pos, rows, cols)
        regions[name + "_top"] = (pos, t.end)
        pos = t.end
        rng.mix(t.root)
        roots.append(t.root.copy())
        return t

    trees["code"] = commit_tree("code", domain, c["group_size"][1])
    trees["data"] = commit_tree("data", domain, c["group_size"][2])
    if n_late:
        rng.mix(hash_elem_slice(glob[n_global - n_late:n_global]))
    mix = [rng.random_elem() for _ in range(c["n_mix"])]
    trees["accum"] = commit_tree("accum", domain, c["group_size"][0])
    poly_mix = rng.random_ext()
    trees["check"] = commit_tree("check", domain, CHECK_SIZE)
    z = rng.random_ext()
    n_u = c["n_taps"] + CHECK_SIZE
    regions["coeff_u"] = (pos, pos + 4 * n_u)
    rng.mix(hash_elem_slice(seal[pos:pos + 4 * n_u]))
    pos += 4 * n_u
    deep_mix = rng.random_ext()
    rounds, fri_mix, deg = [], [], n
    while deg > FRI_MIN_DEGREE:
        t = commit_tree("fri%d" % len(rounds), deg * INV_RATE // FRI_FOLD, FRI_FOLD * 4)
        fri_mix.append(rng.random_ext())
        rounds.append(t)
        deg //= FRI_FOLD
    regions["final"] = (pos, pos + 4 * deg)
    rng.mix(hash_elem_slice(seal[pos:pos + 4 * deg]))
    pos += 4 * deg
    positions = [rng.random_bits(_log2(domain)) % domain for _ in range(QUERIES)]
    order = [("accum", trees["accum"]), ("code", trees["code"]), ("data", trees["data"]), ("check", trees["check"])]
    order += [("fri%d" % i, t) for i, t in enumerate(rounds)]
    regions["openings"] = (pos, pos + QUERIES * sum(t.opening_words for _, t in order))
    opening, ok, first_bad = [], 0, None
    for q, row in enumerate(positions):
        for name, t in order:
            if name.startswith("fri"):
                row = row % t.rows
            good = t.check_opening(seal, pos, row)
            opening.append((name, q, pos, pos + t.cols, pos + t.opening_words))
            ok += good
            if not good and first_bad is None:
                first_bad = (name, q)
            pos += t.opening_words
    regions["opening"] = opening
    return {"po2": po2, "roots": roots, "mix": mix, "poly_mix": poly_mix, "z": z, "deep_mix": deep_mix, "fri_mix": fri_mix,
            "positions": positions, "openings_ok": ok, "openings_total": len(opening), "first_bad": first_bad, "regions": regions,
            "words": pos, "seal_words": int(seal.size)}
