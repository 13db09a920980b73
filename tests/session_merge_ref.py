"""Export and merge of the session balance (r0h_session_balance_export / _merge, include/r0hip.h) restated from the header's text on top
of tests/session_balance_ref.py -- a helper module for test_session_merge.py, test_distributed_session_merge.py and
test_gpu_session_merge.py; no tests of its own.

A class table is a plain dict: fingerprint -> [net, members, (source, row, fraction) of the lowest member, values].

    fingerprint(ids, values)                 the header's key of a class: two linear hashes under the splitmix64 weights
    table(blob, segments, outside=())        the table of one handle that had these additions (session_balance_ref's inputs)
    merge(a, b)                              -> a new table: sums mod p, members saturating, lowest member, values of whoever had it first
    export(t, n_ids)                         -> the 64-byte records in ascending key order (numpy structured array)
    report(t) / message(t)                   what r0h_session_balance_report / _message say of a handle that holds t"""
import numpy as np

import session_balance_ref as sr

P = sr.P
M64 = (1 << 64) - 1
SATURATED = 0xFFFFFFFF
DTYPE = np.dtype([("key", "<u8"), ("net", "<u4"), ("members", "<u4"), ("source", "<u4"), ("first_row", "<u4"), ("fraction", "<u4"), ("n_values", "<u4"), ("values", "<u4", (8,))])


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def weight(j, identity):
    h = splitmix64((splitmix64(identity) + 0xBA1A9CE * (j + 1)) & M64)
    return 1 + (((h >> 32) * (P - 1)) >> 32)


def identity_words(blob):
    """the handle's identities as kind << 32 | index, 0 for "one" """
    return [(kind << 32 | index) if kind else 0 for kind, index in sr.identities(blob)]


def fingerprint(ids, values):
    h = [sum(weight(j, i) * int(v) for i, v in zip(ids, values)) % P for j in (0, 1)]
    return (h[0] << 31 | h[1]) + 1


def _insert(t, key, net, members, first, values):
    if key not in t:
        t[key] = [0, 0, first, tuple(int(v) for v in values)]
    c = t[key]
    c[0] = (c[0] + int(net)) % P
    c[1] = min(c[1] + int(members), SATURATED)
    c[2] = min(c[2], first)


def table(blob, segments, outside=()):
    ids = identity_words(blob)
    t = {}
    if not ids:
        return t
    for source, po2, code, data, glob in segments:
        vecs, nums, rows, which = sr.segment_tuples(blob, po2, code, data, glob)
        for v, num, r, f in zip(vecs, nums, rows, which):
            _insert(t, fingerprint(ids, v), num, 1, (int(source), int(r), int(f)), v)
    for source, numerators, values in outside:
        num = np.asarray(numerators, dtype=np.int64).reshape(-1)
        vals = np.asarray(values, dtype=np.int64).reshape(len(num), -1) if len(num) else np.zeros((0, len(ids)), dtype=np.int64)
        for i in np.nonzero(num)[0]:
            _insert(t, fingerprint(ids, vals[i]), num[i], 1, (int(source), int(i), sr.OUTSIDE), vals[i])
    return t


def merge(a, b):
    t = {k: list(c) for k, c in a.items()}
    for key, (net, members, first, values) in b.items():
        _insert(t, key, net, members, first, values)
    return t


def from_records(records):
    """an exported list as a table (a key that comes twice is combined, as a merge into an empty handle would)"""
    t = {}
    for e in records:
        _insert(t, int(e["key"]), e["net"], e["members"], (int(e["source"]), int(e["first_row"]), int(e["fraction"])), e["values"][:int(e["n_values"])])
    return t


def export(t, n_ids):
    out = np.zeros(len(t), dtype=DTYPE)
    for e, key in zip(out, sorted(t)):
        net, members, (source, row, fraction), values = t[key]
        e["key"], e["net"], e["members"], e["source"], e["first_row"], e["fraction"], e["n_values"] = key, net, members, source, row, fraction, n_ids
        e["values"][:n_ids] = values
    return out


def tuples(t):
    return min(sum(c[1] for c in t.values()), SATURATED)


def report(t):
    bad = sorted((c for c in t.values() if c[0]), key=lambda c: c[2])
    return [(first[0], first[1], first[2], net, members, values) for net, members, first, values in bad]


def message(t):
    bad = report(t)
    if not bad:
        return None
    source, row, fraction, net, members, values = bad[0]
    return "session fraction %d does not balance: net %d over %d tuples, first in source %d at row %d, class (%s); %d classes in all" % (
        fraction, net, members, source, row, ", ".join(str(v) for v in values), len(bad))
