"""r0h_session_balance_export / _merge / _add_session on the device against the host handle and tests/session_merge_ref.py.

Device handles at 2^9 rows, the smallest size tests/test_gpu_session_balance.py runs the device path at: the compaction kernel's export
against the host's, merges of 300, 600 and 1,100 distinct classes that stay below, cross once and cross twice the load of 1/2 of the
1,024-slot first table, and lists that go from one kind of handle to the other.  Then the trace circuit's small session of
tests/test_session_balance.py (segment_po2 = 9) in two shares in one process: every share's own additions, the verifier's side on one
share, the exports merged both ways -- honest, and with the forgeries an honest executor cannot make planted where they can be: a journal
word and another ELF on the verifier's side of a real session, a boundary value between two segments in witnesses fed share by share;
the same with every segment evicted, and through driver.prove_elf_sharded with a world of one rank."""
import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from hyperfridge_r0_amd import driver
from conftest import circuit_path

import session_balance_circuits as sc
import session_merge_ref as mr
from test_session_balance import trace_session  # noqa: F401
from test_session_merge import same

pytestmark = pytest.mark.gpu
PO2 = r0.TRACE_MIN_PO2
WORDS = [7, 0x01020304]
P = mr.P


def device_add(hal, sb, gc, segment):
    source, po2, code, data, glob = segment
    data_buf = hal.copy_from(data)
    code_buf = hal.copy_from(code) if code is not None else None
    try:
        sb.add(source, po2, code_buf, data_buf, glob, circuit=gc)
    finally:
        data_buf.free()
        if code_buf is not None:
            code_buf.free()


def agree(device, host, t=None, n_ids=3):
    assert device.report() == host.report() and device.message() == host.message()
    assert (device.stats()[0], device.stats()[3]) == (host.stats()[0], host.stats()[3])
    assert same(device.export(), host.export())
    if t is not None:
        assert same(device.export(), mr.export(t, n_ids)) and device.report() == mr.report(t) and device.stats()[3] == len(t)


@pytest.fixture(scope="module")
def pairs(hal):
    """the generated circuit and a session of 2^9 + 2^9 + 2^10 rows whose every tuple is a class of its own: 2,048 classes"""
    c, segments = sc.session("pairs", [9, 9, 10], seed=5, fill=1.0, consumers=False)
    gc = hal.load_circuit(c.words)
    host = r0.SessionBalance(c.words)
    for s in segments:
        host.add(*s)
    classes = host.export()
    assert len(classes) == 2048
    yield c.words, gc, segments, classes
    gc.free()


def test_the_device_exports_what_the_host_exports(hal, pairs):
    blob, gc, segments, _ = pairs
    c2, balanced = sc.session("pairs", [9, 4, 9], seed=6)
    assert np.array_equal(c2.words, blob)
    for segs in (segments[:1], balanced, balanced[::-1]):
        host, device = r0.SessionBalance(blob), r0.SessionBalance(blob, hal)
        assert len(device.export()) == 0 and device.export(capacity=3)[1] == 0            # a handle never used
        for s in segs:
            host.add(*s)
            device_add(hal, device, gc, s)
            agree(device, host)
        agree(device, host, mr.table(blob, segs))
        assert same(device.export(), device.export())
        lowest, n = device.export(capacity=5)
        assert n == host.stats()[3] and same(lowest, host.export()[:5])
        host.free()
        device.free()


@pytest.mark.parametrize("n, slots", [(300, 1024), (600, 2048), (1100, 4096)])
def test_merges_below_across_and_twice_across_the_first_tables_load(hal, pairs, n, slots):
    blob, gc, segments, classes = pairs
    part = classes[(np.arange(n) * 7) % len(classes)] if n < 700 else classes[:n]
    assert len(np.unique(part["key"])) == n
    host, device = r0.SessionBalance(blob), r0.SessionBalance(blob, hal)
    device.merge(classes[:0])                                                             # an empty list into a handle never used
    assert device.stats()[1:] == (1024, 0, 0)
    host.merge(part)
    device.merge(part)
    assert device.stats() == (n, slots, 1 if slots > 1024 else 0, n)
    agree(device, host, mr.from_records(part))
    host.merge(part[::-1][:n // 2])                                                       # classes that are held already: no new slot
    device.merge(part[::-1][:n // 2])
    assert device.stats()[3] == n
    agree(device, host, mr.merge(mr.from_records(part), mr.from_records(part[::-1][:n // 2])))
    device_add(hal, device, gc, segments[0])                                              # ... and the handle goes on taking segments
    host.add(*segments[0])
    agree(device, host)
    host.free()
    device.free()


def test_lists_go_from_one_kind_of_handle_to_the_other(hal, pairs):
    blob, gc, _, _ = pairs
    _, segs = sc.session("pairs", [9, 9], seed=8)
    whole = mr.table(blob, segs)
    host, device = r0.SessionBalance(blob), r0.SessionBalance(blob, hal)
    host.add(*segs[0])
    device_add(hal, device, gc, segs[1])
    assert host.report() and device.report()
    from_host, from_device = host.export(), device.export()
    assert same(from_device, mr.export(mr.table(blob, segs[1:]), 3))
    host.merge(from_device)
    device.merge(from_host)
    agree(device, host, whole)
    assert device.report() == []
    twice = np.concatenate([from_host, from_host[::-1]])                                   # a key twice in one list, two lanes on one slot
    host.merge(twice)
    device.merge(twice)
    agree(device, host)
    sat = from_host[:2].copy()
    sat["members"] = 0xFFFFFFF0
    for sb in (host, device):
        sb.merge(sat)
        sb.merge(sat)
    agree(device, host)
    assert np.all(device.export()["members"][np.isin(device.export()["key"], sat["key"])] == 0xFFFFFFFF)
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_merge: the key of entry 1 is not the fingerprint of its values"):
        bad = from_host[:3].copy()
        bad["values"][1, 2] = (int(bad["values"][1, 2]) + 1) % P
        device.merge(bad)
    agree(device, host)                                                                    # a refused list leaves nothing behind
    host.free()
    device.free()


# ---- the trace circuit's session in two shares
@pytest.fixture(scope="module")
def trace(hal):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    yield gc, blob
    gc.free()


@pytest.fixture(autouse=True)
def nothing_left_behind(hal):
    yield
    hal.set_session_device_limit(0)
    assert hal.session_held_bytes() == 0


def begin_shares(hal, gc, ts, limit):
    hal.set_session_device_limit(limit)
    try:
        return [hal.session_begin(gc, ts.elf, WORDS, segment_po2=9, part=k, parts=2) for k in range(2)]
    finally:
        hal.set_session_device_limit(0)     # (taken per session when it began)


def gathered(hal, blob, sessions, elf, journal, verifier_on=0):
    """a handle per share with the share's own additions, the verifier's side on one of them, the exports merged both ways"""
    handles = [r0.SessionBalance(blob, hal) for _ in sessions]
    for k, (sb, ses) in enumerate(zip(handles, sessions)):
        sb.add_session(ses)
        if k == verifier_on:
            sb.add_verifier_side(elf, journal)
    exports = [sb.export() for sb in handles]
    handles[0].merge(exports[1])
    handles[1].merge(exports[0])
    return handles, exports


def host_handle(ts, segments, elf, journal):
    sb = r0.SessionBalance(ts.blob)
    for s in segments:
        sb.add(*s)
    sb.add_verifier_side(elf, journal)
    return sb


@pytest.mark.parametrize("limit", [0, 1], ids=["resident", "every segment evicted"])
def test_a_session_in_two_shares_balances_is_named_and_still_finishes(hal, trace, trace_session, limit):  # noqa: F811
    gc, blob = trace
    ts = trace_session
    sessions = begin_shares(hal, gc, ts, limit)
    try:
        assert sessions[0].journal == sessions[1].journal == ts.journal and sessions[0].n_segments == len(ts.segments) >= 3
        # honest: each share alone is open, both merged handles balance and hold what one handle with every addition holds
        handles, exports = gathered(hal, blob, sessions, ts.elf, ts.journal)
        want = host_handle(ts, ts.segments, ts.elf, ts.journal)
        assert len(exports[0]) and len(exports[1]) and want.message() is None
        for sb in handles:
            assert sb.message() is None and sb.report() == []
            agree(sb, want)
            sb.free()
        # a journal word and another ELF: the verifier's side goes to the share that does NOT hold the named segment
        journal = bytes([ts.journal[0] ^ 1]) + ts.journal[1:]
        for elf, jrn in ((ts.elf, journal), (ts.other_elf, ts.journal)):
            want = host_handle(ts, ts.segments, elf, jrn)
            first = want.report()[0]
            assert want.message() and first[0] < len(ts.segments)                          # a segment's own tuple is the lowest member named
            handles, exports = gathered(hal, blob, sessions, elf, jrn, verifier_on=(first[0] + 1) % 2)
            for sb in handles:
                assert sb.message() == want.message()
                agree(sb, want)
                sb.free()
        # the session is as it was: it finishes under the records of both shares and verifies with the ELF
        records = np.zeros((sessions[0].n_segments, r0.SESSION_RECORD_WORDS), dtype=np.uint32)
        for ses in sessions:
            idx, rec = ses.records()
            records[idx] = rec
        receipts = [ses.finish(records)[0] for ses in sessions]
        if limit:
            assert hal.last_session_device()["evicted"] >= 1
        merged = r0.Receipt.merge(receipts)
        assert merged.verify(blob, {PO2: hal.code_root(gc, PO2)}, None, elf=ts.elf)[:2] == (0, "ok")
        with pytest.raises(r0.R0HipError, match="r0h_session_balance_add_session: segment 0 is finished"):
            sb = r0.SessionBalance(blob, hal)
            sb.add_session(sessions[0])
    finally:
        for ses in sessions:
            ses.close()


def test_a_boundary_value_altered_between_two_shares(hal, trace, trace_session):  # noqa: F811
    """segment 1 finds another value than segment 0 left: producer and consumer sit in different shares"""
    gc, blob = trace
    ts = trace_session
    alter, addr = ts.boundary_alteration()
    segments = ts.witnesses(edit=alter)
    want = host_handle(ts, segments, ts.elf, ts.journal)
    handles = [r0.SessionBalance(blob, hal) for _ in range(2)]
    for s in segments:
        device_add(hal, handles[s[0] % 2], gc, s)
    handles[0].add_verifier_side(ts.elf, ts.journal)
    exports = [sb.export() for sb in handles]
    handles[0].merge(exports[1])
    handles[1].merge(exports[0])
    named = [w for w in want.report() if w[5][1] == (-addr) % P]
    assert named and {w[0] for w in named} >= {0, 1}
    for sb in handles:
        assert sb.message() == want.message() is not None
        agree(sb, want)
        sb.free()


class _AlteredJournal:
    """stands where the Hal stands in driver.prove_elf_sharded: its sessions say another journal than the guest wrote (an honest
    executor cannot), so that the verifier's side the driver adds does not cancel the run's COMMIT rows"""

    def __init__(self, hal, journal):
        self.hal, self.ctx, self.journal = hal, hal.ctx, journal

    def session_begin(self, *args, **kwargs):
        ses = self.hal.session_begin(*args, **kwargs)
        journal = self.journal

        class Altered(r0.Session):
            @property
            def journal(self):
                return journal
        handle, ses.handle = ses.handle, None
        return Altered(handle)


def test_the_driver_with_a_world_of_one_rank(hal, trace, trace_session):  # noqa: F811
    gc, blob = trace
    ts = trace_session
    env = driver.DistEnv(backend=None)
    assert env.world == 1
    plain, image_id, _ = driver.prove_elf_sharded(env, hal, gc, ts.elf, WORDS, segment_po2=9)
    timings = {}
    checked, image_id2, _ = driver.prove_elf_sharded(env, hal, gc, ts.elf, WORDS, segment_po2=9, check_session=True, timings=timings)
    assert checked.to_json() == plain.to_json() and image_id2 == image_id                  # honest: the same receipt, byte for byte
    assert timings["exported_bytes"] == 64 * timings["exported_classes"] > 0 and {"add_ms", "export_ms", "exchange_ms", "merge_ms", "report_ms"} <= set(timings)
    journal = bytes([ts.journal[0] ^ 1]) + ts.journal[1:]
    want = host_handle(ts, ts.segments, ts.elf, journal).message()
    assert want is not None
    with pytest.raises(r0.R0HipError) as err:
        driver.prove_elf_sharded(env, _AlteredJournal(hal, journal), gc, ts.elf, WORDS, segment_po2=9, check_session=True)
    assert str(err.value) == "r0h_prove_elf: " + want                                      # the single-rank check's words
    assert hal.session_held_bytes() == 0                                                   # the session was closed


def test_add_session_refuses_what_is_not_a_trace_session_or_not_a_device_handle(hal, trace, trace_session):  # noqa: F811
    gc, blob = trace
    ts = trace_session
    small_blob = np.fromfile(circuit_path("small"), dtype=np.uint32)
    small = hal.load_circuit(small_blob, entry.code_object_path("small"))
    ses = hal.session_begin(small, ts.elf, WORDS, segment_po2=9)
    try:
        with pytest.raises(r0.R0HipError, match="r0h_session_balance_add_session: the session's circuit is not the trace circuit"):
            r0.SessionBalance(small_blob, hal).add_session(ses)
    finally:
        ses.close()
        small.free()
    ses = hal.session_begin(gc, ts.elf, WORDS, segment_po2=9, part=1, parts=2)
    try:
        with pytest.raises(r0.R0HipError, match="r0h_session_balance_add_session: this handle was made without a context"):
            r0.SessionBalance(blob).add_session(ses)
        with pytest.raises(r0.R0HipError, match="the circuit is not the one the handle was made with"):
            r0.SessionBalance(small_blob, hal).add_session(ses)
    finally:
        ses.close()
