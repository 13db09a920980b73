"""The balance of a log-derivative argument's chain links (r0h_logup_check_balance, include/r0hip.h) restated in numpy from the blob
alone -- a helper module for test_balance.py and test_gpu_balance.py; no tests of its own.

The blob is read by logup_ref.parse; a tuple's class is the exact vector of its per-identity part sums (canonical integers), and classes
are told apart by np.unique over whole vectors: nothing is hashed.  check() returns the full ordered list.  (On the trace circuit at
2^16 rows np.unique(axis=0) over 1.6 million vectors takes seven seconds; check() therefore refines the partition identity by
identity -- class id so far and the next coordinate, packed exactly into one int64 -- which gives the same partition in one second;
whole_vectors=True takes np.unique(axis=0) itself, and test_balance.py holds the two against each other.)"""
import numpy as np

import logup_ref as ref

P = ref.P


def chain_fractions(c):
    """[(fraction number 4 * accumulator + slot, fraction)] of the chain links, in blob order"""
    return [(4 * j + s, f) for j, (final, frs) in enumerate(c["accs"]) if final is None for s, f in enumerate(frs)]


def tuples(blob, po2, code, data, glob):
    """-> (vectors [tuples, identities], numerators, rows, fractions): every tuple of the chain links, canonical int64"""
    c = ref.parse(blob)
    cols = ref.Columns(c, po2, code, data, glob, None)
    frs = chain_fractions(c)
    ids = {}
    for _, f in frs:
        for kind, idx, _ in f["parts"]:
            ids.setdefault((kind, idx if kind else 0), len(ids))
    vecs, nums, rows, which = [], [], [], []
    for fi, f in frs:
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
    if not vecs:
        return np.zeros((0, 1), dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(vecs), np.concatenate(nums), np.concatenate(rows), np.concatenate(which)


def check(blob, po2, code, data, glob, whole_vectors=False):
    """-> [(fraction, first_row, net, members)] of the classes whose numerators do not sum to 0 mod p, in (first_row, fraction) order"""
    vecs, nums, rows, which = tuples(blob, po2, code, data, glob)
    if not len(nums):
        return []
    if whole_vectors:
        _, inv = np.unique(vecs, axis=0, return_inverse=True)
        inv = inv.reshape(-1)
    else:
        inv = np.zeros(len(nums), dtype=np.int64)
        for k in range(vecs.shape[1]):   # (class ids below 2^32, coordinates below 2^31: the pair is exact in an int64)
            _, inv = np.unique(inv << 31 | vecs[:, k], return_inverse=True)
            inv = inv.reshape(-1).astype(np.int64)
    k = int(inv.max()) + 1
    total = np.zeros(k, dtype=np.int64)           # numerators below 2^31, at most 2^32 tuples: exact only below 2^63 / 2^31 = 2^32 members
    np.add.at(total, inv, nums)
    members = np.bincount(inv, minlength=k)
    first = np.full(k, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, inv, rows << 32 | which)
    bad = np.nonzero(total % P)[0]
    bad = bad[np.argsort(first[bad])]
    return [(int(first[u] & 0xFFFFFFFF), int(first[u] >> 32), int(total[u] % P), int(min(members[u], 0xFFFFFFFF))) for u in bad]
