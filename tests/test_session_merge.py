"""r0h_session_balance_export / _merge on host handles (needs no GPU) against the restatement in tests/session_merge_ref.py: the additions
of one session split over two and three handles and merged back in every order and tree-wise must give, word for word, what one handle
with every addition gives; classes closed across handles, the lowest member on the merged-in side, saturation, the edges of the lists
and every refusal by its entry index.  tests/test_gpu_session_merge.py runs the device's side of the same contract."""
import itertools

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import circuit_path

import logup_ref as ref
import session_balance_circuits as sc
import session_merge_ref as mr
from test_session_balance import bump, outside_of

P = ref.P


def additions(kind="pairs", sizes=(4, 6, 5, 5), seed=11, broken=False):
    """one session's additions: segments that balance among themselves, two more whose producers stand alone, and the outside list
    that cancels those (the verifier's side of a generated circuit) -> (blob, [("segment", seg) | ("outside", list)])"""
    c, segments = sc.session(kind, list(sizes), seed=seed)
    _, alone = sc.session(kind, [5, 4], seed=seed + 1, consumers=False)
    alone = [(len(sizes) + k,) + s[1:] for k, s in enumerate(alone)]
    outside = outside_of(c.words, alone, source=r0.SESSION_SOURCE_JOURNAL)
    if broken:   # a produced pair altered in segment 1: its consumer elsewhere and the altered tuple stand alone
        row = next(r for r in range(1 << sizes[1]) if ref.dec(segments[1][3][sc.slot(segments, 1, 4, r)]) == 1)
        segments = bump(segments, 1, 0, row)
    return c.words, [("segment", s) for s in segments + alone] + [("outside", outside)]


def feed(sb, adds):
    for what, a in adds:
        if what == "segment":
            sb.add(*a)
        else:
            sb.add_tuples(*a)
    return sb


def ref_table(blob, adds):
    return mr.table(blob, [a for what, a in adds if what == "segment"], [a for what, a in adds if what == "outside"])


def same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def holds(sb, t, n_ids):
    """the handle says what a handle that holds table `t` says: report, message, tuples, classes and its own export"""
    assert sb.report() == mr.report(t)
    assert sb.message() == mr.message(t)
    stats = sb.stats()
    assert (stats[0], stats[3]) == (mr.tuples(t), len(t))
    assert same(sb.export(), mr.export(t, n_ids))


PATTERNS = {2: ([0, 1, 0, 1, 0, 1, 0], [0, 0, 0, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 1, 0, 1, 1]),
            3: ([0, 1, 2, 0, 1, 2, 0], [0, 0, 1, 1, 2, 2, 2], [2, 2, 2, 2, 2, 2, 1], [1, 2, 0, 0, 2, 1, 0])}


@pytest.mark.parametrize("broken", [False, True], ids=["balanced", "one cell altered"])
@pytest.mark.parametrize("n_handles", [2, 3])
def test_split_additions_merge_to_the_single_handle_in_every_order(n_handles, broken):
    blob, adds = additions(broken=broken)
    n_ids = len(mr.identity_words(blob))
    whole = ref_table(blob, adds)
    single = feed(r0.SessionBalance(blob), adds)
    holds(single, whole, n_ids)
    assert (mr.report(whole) == []) != broken and (not broken or len(mr.report(whole)) == 2)
    want = (single.report(), single.message(), single.stats()[0], single.stats()[3], single.export().tobytes())
    for pattern in PATTERNS[n_handles]:
        shares = [[a for a, h in zip(adds, pattern) if h == k] for k in range(n_handles)]
        tables = [ref_table(blob, s) for s in shares]

        def fresh():
            return [feed(r0.SessionBalance(blob), s) for s in shares]
        for k, sb in enumerate(fresh()):
            holds(sb, tables[k], n_ids)
        for order in itertools.permutations(range(n_handles)):      # the first receives the others' exports in this order
            handles = fresh()
            exports = [h.export() for h in handles]
            t = tables[order[0]]
            for k in order[1:]:
                handles[order[0]].merge(exports[k])
                t = mr.merge(t, tables[k])
                holds(handles[order[0]], t, n_ids)
            got = handles[order[0]]
            assert (got.report(), got.message(), got.stats()[0], got.stats()[3], got.export().tobytes()) == want
        handles = fresh()                                           # tree-wise: the last into the one before it, and so on down to the first
        for k in range(n_handles - 1, 0, -1):
            handles[k - 1].merge(handles[k].export())
        got = handles[0]
        assert (got.report(), got.message(), got.stats()[0], got.stats()[3], got.export().tobytes()) == want
        if n_handles == 3:                                          # ... and the two outer ones into the middle, which then goes into a fresh handle
            handles = fresh()
            handles[1].merge(handles[0].export())
            handles[1].merge(handles[2].export())
            got = r0.SessionBalance(blob)
            got.merge(handles[1].export())
            assert (got.report(), got.message(), got.stats()[0], got.stats()[3], got.export().tobytes()) == want


def test_a_class_is_closed_across_handles():
    c, segments = sc.session("pairs", [5, 5], seed=3)
    a, b = (feed(r0.SessionBalance(c.words), [("segment", s)]) for s in segments)
    ea, eb = a.export(), b.export()
    nets_a, nets_b = dict(zip(ea["key"].tolist(), ea["net"].tolist())), dict(zip(eb["key"].tolist(), eb["net"].tolist()))
    crossing = [k for k in nets_a if k in nets_b and {nets_a[k], nets_b[k]} == {1, P - 1}]     # produced on one handle, consumed on the other
    assert crossing and a.report() and b.report()
    members = {k: int(ea["members"][ea["key"] == k][0]) + int(eb["members"][eb["key"] == k][0]) for k in crossing}
    a.merge(eb)
    b.merge(ea)
    assert a.report() == [] and b.report() == [] and a.message() is None
    merged = a.export()
    assert same(merged, b.export())
    for k in crossing:
        e = merged[merged["key"] == k][0]
        assert e["net"] == 0 and e["members"] == members[k] == 2
    holds(a, mr.table(c.words, segments), 3)


def test_the_lowest_member_may_lie_on_the_merged_in_handle():
    c, segments = sc.session("pairs", [5, 4, 5], seed=4)
    row = next(r for r in range(32) if ref.dec(segments[0][3][sc.slot(segments, 0, 4, r)]) == 1)
    bad = bump(segments, 0, 0, row)
    receiver = feed(r0.SessionBalance(c.words), [("segment", s) for s in bad[1:]])
    other = feed(r0.SessionBalance(c.words), [("segment", bad[0])])
    receiver.merge(other.export())
    whole = mr.table(c.words, bad)
    holds(receiver, whole, 3)
    first = receiver.report()[0]
    assert first[0] == 0 and (first[1], first[2]) == (row, 4) and "first in source 0 at row %d" % row in receiver.message()


def one_class(blob, values, net=1, members=1, first=(0, 0, 4)):
    ids = mr.identity_words(blob)
    e = np.zeros(1, dtype=r0.SESSION_CLASS_DTYPE)
    e["key"], e["net"], e["members"], e["n_values"] = mr.fingerprint(ids, values), net, members, len(ids)
    e["source"], e["first_row"], e["fraction"] = first
    e["values"][0, :len(ids)] = values
    return e


def test_members_saturate_through_a_merge():
    blob = sc.Circuit("pairs").words
    sb = r0.SessionBalance(blob)
    sb.merge(one_class(blob, [1, 5, 9], net=7, members=0xFFFFFFF0, first=(3, 2, 4)))
    assert sb.export()["members"][0] == 0xFFFFFFF0 and sb.stats()[0] == 0xFFFFFFF0
    sb.merge(one_class(blob, [1, 5, 9], net=P - 6, members=0x20, first=(2, 9, 5)))
    e = sb.export()[0]
    assert (e["net"], e["members"], e["source"], e["first_row"], e["fraction"]) == (1, 0xFFFFFFFF, 2, 9, 5) and sb.stats()[0] == 0xFFFFFFFF
    assert sb.report() == [(2, 9, 5, 1, 0xFFFFFFFF, (1, 5, 9))]
    t = mr.merge(mr.from_records(one_class(blob, [1, 5, 9], net=7, members=0xFFFFFFF0, first=(3, 2, 4))), mr.from_records(one_class(blob, [1, 5, 9], net=P - 6, members=0x20, first=(2, 9, 5))))
    holds(sb, t, 3)
    again = r0.SessionBalance(blob)
    again.merge(sb.export())                    # a saturated count travels as it is
    again.merge(sb.export())
    assert again.export()["members"][0] == 0xFFFFFFFF and again.export()["net"][0] == 2


def test_the_edges_of_the_lists():
    blob, adds = additions()
    empty = r0.SessionBalance(blob)
    out = empty.export()
    assert out.dtype == r0.SESSION_CLASS_DTYPE and len(out) == 0 and empty.export(capacity=4)[1] == 0      # export from an empty handle
    full = feed(r0.SessionBalance(blob), adds)
    before = full.export()
    full.merge(out)                                                                                        # merge of an empty list
    r0._check(r0.lib().r0h_session_balance_merge(full.handle, None, 0))
    assert same(full.export(), before) and same(full.export(), full.export())                              # export twice: the same bytes
    empty.merge(before)                                                                                    # merge into a never-used handle
    holds(empty, ref_table(blob, adds), 3)
    assert same(empty.export(), before)
    lowest, n = full.export(capacity=3)                                                                    # capacity below the class count
    assert n == len(before) > 3 and same(lowest, before[:3]) and full.export(capacity=0)[1] == n
    assert np.all(np.diff(before["key"].astype(np.uint64)) > 0) and np.all(before["n_values"] == 3) and np.all(before["values"][:, 3:] == 0)
    twice = r0.SessionBalance(blob)                                                                        # a key present twice in one list
    part = before[:5]
    twice.merge(np.concatenate([part, part[::-1]]))
    got = twice.export()
    assert np.array_equal(got["key"], part["key"]) and np.array_equal(got["members"], 2 * part["members"])
    assert np.array_equal(got["net"], 2 * part["net"].astype(np.int64) % P) and np.array_equal(got["values"], part["values"])
    holds(twice, mr.merge(mr.from_records(part), mr.from_records(part)), 3)
    raw = r0.SessionBalance(blob)                                                                          # the records as plain bytes
    raw.merge(np.frombuffer(before.tobytes(), dtype=np.uint8))
    assert same(raw.export(), before)
    tiny = r0.SessionBalance(np.fromfile(circuit_path("tiny"), dtype=np.uint32))                           # no public-total accumulators: no classes
    assert len(tiny.export()) == 0
    tiny.merge(tiny.export())


def test_refusals_by_entry_index():
    blob, adds = additions()
    good = feed(r0.SessionBalance(blob), adds).export()
    sb = r0.SessionBalance(blob)

    def refused(field, value, text, at=2, k=None):
        bad = good[:4].copy()
        if k is None:
            bad[field][at] = value
        else:
            bad[field][at, k] = value
        with pytest.raises(r0.R0HipError, match="r0h_session_balance_merge: " + text):
            sb.merge(bad)
    refused("n_values", 2, r"entry 2 has 2 values, the handle has 3 identities")
    refused("n_values", 4, r"entry 1 has 4 values, the handle has 3 identities", at=1)
    refused("key", 0, r"entry 3 has key 0", at=3)
    refused("net", P, r"net of entry 2 is not canonical")
    refused("values", P, r"value 1 of entry 0 is not canonical", at=0, k=1)
    refused("values", 0xFFFFFFFF, r"value 2 of entry 2 is not canonical", k=2)
    refused("fraction", 256, r"entry 2 has fraction 256: more than 255")
    refused("first_row", 1 << 24, r"entry 2 has first row 16777216: not below 2\^24")
    refused("values", (int(good["values"][2, 1]) + 1) % P, r"the key of entry 2 is not the fingerprint of its values", k=1)     # one value word altered
    refused("key", int(good["key"][2]) + 1, r"the key of entry 2 is not the fingerprint of its values")
    assert len(sb.export()) == 0 and sb.stats()[0] == 0                 # a refused list leaves nothing behind
    trace = r0.SessionBalance(np.fromfile(circuit_path("trace"), dtype=np.uint32))      # an export from a circuit with another identity count
    trace.add_tuples(0, [1], [[1, 2, 3, 4, 5]])
    other = trace.export()
    assert len(other) == 1 and other["n_values"][0] == 5
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_merge: entry 0 has 5 values, the handle has 3 identities"):
        sb.merge(other)
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_merge: entry 0 has 3 values, the handle has 5 identities"):
        trace.merge(good)
    with pytest.raises(r0.R0HipError, match=r"r0h_session_balance_merge: \d+ classes in one call: more than 2\^24"):
        r0._check(r0.lib().r0h_session_balance_merge(sb.handle, good.ctypes.data_as(r0._vp), (1 << 24) + 1))     # (the count is refused before an entry is read)
    with pytest.raises(r0.R0HipError, match="SessionBalance.merge: 65 bytes"):
        sb.merge(np.zeros(65, dtype=np.uint8))
    sb.merge(good)                                                      # the handle goes on working
    assert same(sb.export(), good)


def test_add_session_wants_a_session_and_the_symbols_are_exported():
    """a session needs a device, so the refusal of a session that is not the trace circuit's is tests/test_gpu_session_merge.py's; here:
    the entry points exist and refuse what they can be given without one"""
    for name in ("r0h_session_balance_export", "r0h_session_balance_merge", "r0h_session_balance_add_session", "r0h_session_journal"):
        assert name in r0.EXPORTED_SYMBOLS
    sb = r0.SessionBalance(sc.Circuit("pairs").words)
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_add_session: NULL argument"):
        r0._check(r0.lib().r0h_session_balance_add_session(sb.handle, None))
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_export: NULL argument"):
        r0._check(r0.lib().r0h_session_balance_export(sb.handle, None, 0, None))
