"""The session balance (r0h_session_balance_*, include/r0hip.h) restated in numpy from the blob alone -- a helper module for
test_session_balance.py and test_gpu_session_balance.py; no tests of its own.

The blob is read by logup_ref.parse; a tuple's class is the exact vector of its per-identity part sums (canonical integers), one
coordinate per challenge identity in order of first appearance over the accumulators with a public total, and classes are told apart by
refining the partition coordinate by coordinate (balance_ref.check's way): nothing is hashed.

    identities(blob)                      -> [(kind, index)] ((0, 0) is "one")
    segment_tuples(blob, po2, code, data, glob) -> (vectors [tuples, identities], numerators, rows, fractions)
    check(blob, segments, outside=())     -> the full ordered report
        segments: [(source, po2, code, data, glob)] library words; outside: [(source, numerators, values)] canonical integers
        -> [(source, first_row, fraction, net, members, values)] in (source, row, fraction) order of the lowest member"""
import numpy as np

import logup_ref as ref

P = ref.P
OUTSIDE = 255


def public_fractions(c):
    """[(fraction number 4 * accumulator + slot, fraction)] of the accumulators whose `final` is a public input, in blob order"""
    return [(4 * j + s, f) for j, (final, frs) in enumerate(c["accs"]) if final is not None for s, f in enumerate(frs)]


def _identities(c):
    ids = {}
    for _, f in public_fractions(c):
        for kind, idx, _ in f["parts"]:
            ids.setdefault((kind, idx if kind else 0), len(ids))
    return ids


def identities(blob):
    return list(_identities(ref.parse(blob)))


def segment_tuples(blob, po2, code, data, glob):
    c = ref.parse(blob)
    cols = ref.Columns(c, po2, code, data, glob, None)
    ids = _identities(c)
    vecs, nums, rows, which = [np.zeros((0, max(len(ids), 1)), dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)]
    for fi, f in public_fractions(c):
        num = cols.form(f["num"])
        r = np.nonzero(num)[0]
        if not len(r):
            continue
        v = np.zeros((len(r), max(len(ids), 1)), dtype=np.int64)
        for kind, idx, lf in f["parts"]:
            k = ids[(kind, idx if kind else 0)]
            v[:, k] = (v[:, k] + cols.form(lf)[r]) % P
        vecs.append(v)
        nums.append(num[r])
        rows.append(r.astype(np.int64))
        which.append(np.full(len(r), fi, dtype=np.int64))
    return np.concatenate(vecs), np.concatenate(nums), np.concatenate(rows), np.concatenate(which)


def check(blob, segments, outside=()):
    n_ids = max(len(identities(blob)), 1)
    vecs, nums, keys = [], [], []
    for source, po2, code, data, glob in segments:
        v, num, rows, which = segment_tuples(blob, po2, code, data, glob)
        vecs.append(v)
        nums.append(num)
        keys.append(np.uint64(source) << np.uint64(32) | (rows.astype(np.uint64) << np.uint64(8)) | which.astype(np.uint64))
    for source, numerators, values in outside:
        num = np.asarray(numerators, dtype=np.int64).reshape(-1)
        v = np.asarray(values, dtype=np.int64).reshape(len(num), -1) if len(num) else np.zeros((0, n_ids), dtype=np.int64)
        live = np.nonzero(num)[0]       # a numerator of zero is no tuple; the others keep their index in the list as their row
        vecs.append(v[live])
        nums.append(num[live])
        keys.append(np.uint64(source) << np.uint64(32) | (live.astype(np.uint64) << np.uint64(8)) | np.uint64(OUTSIDE))
    if not nums or not sum(len(x) for x in nums) or not identities(blob):
        return []
    vecs, nums, keys = np.concatenate(vecs), np.concatenate(nums), np.concatenate(keys)
    inv = np.zeros(len(nums), dtype=np.int64)
    for k in range(vecs.shape[1]):   # (class ids below 2^32, coordinates below 2^31: the pair is exact in an int64)
        _, inv = np.unique(inv << 31 | vecs[:, k], return_inverse=True)
        inv = inv.reshape(-1).astype(np.int64)
    k = int(inv.max()) + 1
    total = np.zeros(k, dtype=np.int64)   # numerators below 2^31: exact for fewer than 2^32 members of a class
    np.add.at(total, inv, nums)
    members = np.bincount(inv, minlength=k)
    first = np.full(k, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(first, inv, keys)
    lowest = np.zeros(k, dtype=np.int64)  # a member of each class, for its vector (class-constant)
    lowest[inv] = np.arange(len(inv))
    bad = np.nonzero(total % P)[0]
    bad = bad[np.argsort(first[bad])]
    return [(int(first[u]) >> 32, (int(first[u]) >> 8) & 0xFFFFFF, int(first[u]) & 255, int(total[u] % P), int(min(members[u], 0xFFFFFFFF)),
             tuple(int(x) for x in vecs[lowest[u]])) for u in bad]
