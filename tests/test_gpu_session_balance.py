"""r0h_session_balance_* on the device against the host handle and the numpy restatement (tests/session_balance_ref.py): the cases of
tests/test_session_balance.py with a device handle beside the host one, so every case asserts device == host == reference -- split
sessions at fewer rows than a wave, one workgroup's and several; the table's growth with the rehash kernel three and four times over;
tuples from outside through the list kernel; the refusals; the trace circuit's honest session and its forgeries with their exact
messages -- then the sequencer's switch and the command line."""
import json
import os
import subprocess

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from conftest import ROOT, circuit_path

import session_balance_circuits as sc  # noqa: E402
import test_session_balance as cases  # noqa: E402
from test_session_balance import FORGERIES, SPLITS, HostSide, trace_session  # noqa: E402,F401

pytestmark = pytest.mark.gpu
PO2 = r0.TRACE_MIN_PO2


class DeviceSide:
    """a device handle fed with the cases' host words: every segment is uploaded for its addition and freed after it"""

    def __init__(self, hal, blob, loaded):
        self.hal = hal
        self.sb = r0.SessionBalance(blob, hal)        # (what the handle refuses, it refuses before a circuit is loaded)
        key = np.asarray(blob, dtype=np.uint32).tobytes()
        if key not in loaded:
            trace = key == np.fromfile(circuit_path("trace"), dtype=np.uint32).tobytes()
            loaded[key] = hal.load_circuit(blob, entry.code_object_path("trace") if trace else None)
        self.circuit = loaded[key]

    def add(self, segment):
        source, po2, code, data, glob = segment
        data_buf = self.hal.copy_from(data)
        code_buf = self.hal.copy_from(code) if code is not None else None
        try:
            self.sb.add(source, po2, code_buf, data_buf, glob, circuit=self.circuit)
        finally:
            data_buf.free()
            if code_buf is not None:
                code_buf.free()

    def close(self):
        self.sb.free()


@pytest.fixture(scope="module")
def both(hal):
    """-> make_sides(blob): a host handle and a device handle; the circuits loaded on the way live as long as the module"""
    loaded = {}
    yield lambda blob: [HostSide(blob), DeviceSide(hal, blob, loaded)]
    for c in loaded.values():
        c.free()


@pytest.mark.parametrize("sizes", SPLITS, ids=str)
def test_split_sessions_balance_and_one_altered_cell_names_its_segment(both, sizes):
    cases.case_split(both, sizes)


@pytest.mark.parametrize("paired", [False, True], ids=["own classes", "paired"])
def test_the_table_grows_and_reports_between_additions(both, paired):
    seen = []

    def stats(side, tuples):
        if isinstance(side, DeviceSide):
            got, slots, grows, occupied = side.sb.stats()
            assert got == tuples and slots >= max(1024, 2 * tuples) and slots & (slots - 1) == 0 and occupied == min(tuples, 2176)
            seen.append((tuples, slots, grows))
    cases.case_growth(both, paired, stats)
    assert seen[:4] == [(512, 1024, 0), (640, 2048, 1), (1152, 4096, 2), (2176, 8192, 3)]     # 512, 1,024 and 2,048 tuples are passed
    assert seen[-1][2] >= 2 and (not paired or seen[-1] == (4352, 16384, 4))


def test_tuples_from_outside(both):
    cases.case_outside(both)


def test_refusals(hal, both):
    cases.case_refusals(both)
    c, segments = sc.session("pairs", [4], seed=1)
    host, device = both(c.words)
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_add_host: this handle was made with a context"):      # the wrong form for the handle's kind
        r0._check(r0.lib().r0h_session_balance_add_host(device.sb.handle, 0, 4, None, segments[0][3].ctypes.data_as(r0._vp), None))
    buf = hal.copy_from(segments[0][3])
    with pytest.raises(r0.R0HipError, match="buffers too small for 2\\^5 rows"):
        device.sb.add(0, 5, None, buf, segments[0][4], circuit=device.circuit)
    other = both(sc.Circuit("zero part").words)[1]
    with pytest.raises(r0.R0HipError, match="the circuit is not the one the handle was made with"):
        device.sb.add(0, 4, None, buf, segments[0][4], circuit=other.circuit)
    device.sb.add(0, 4, None, buf, segments[0][4], circuit=device.circuit)        # the handle goes on working
    assert device.sb.report() == [] and device.sb.stats()[0] == 24
    buf.free()
    for s in (host, device, other):
        s.close()


def test_an_honest_trace_session_balances(both, trace_session):
    cases.case_trace_honest(both, trace_session)


@pytest.mark.parametrize("what", FORGERIES)
def test_a_forged_trace_session_is_named_in_the_sequencers_words(both, trace_session, what):
    """the sequencer's negative path cannot be reached with an honest executor: its text is r0h_session_balance_message's, which
    cases.agree holds, word for word, against the reference's lowest class on every handle"""
    cases.case_trace_forgery(both, trace_session, what)


def test_the_sequencers_switch(hal, trace_session):
    ts = trace_session
    gc = hal.load_circuit(ts.blob, entry.code_object_path("trace"))
    words = [7, 0x01020304]
    try:
        receipt, image_id, cycles = hal.prove_elf(gc, ts.elf, words, segment_po2=9)        # off by default: nothing is checked
        assert len(receipt.seals()) == len(ts.segments) >= 3
        assert "check_session" not in [n for n, _ in hal.last_profile()]
        hal.set_check_session(True)
        checked, image_id2, _ = hal.prove_elf(gc, ts.elf, words, segment_po2=9)
        assert "check_session" in [n for n, _ in hal.last_profile()]
        assert checked.to_json() == receipt.to_json() and image_id2 == image_id             # on, honest: the same receipt, byte for byte
        roots = {PO2: hal.code_root(gc, PO2)}
        assert checked.verify(ts.blob, roots, None, elf=ts.elf)[:2] == (0, "ok")
        with pytest.raises(r0.R0HipError, match="r0h_session_begin: r0h_ctx_set_check_session is on and this is part 0 of 2"):
            hal.session_begin(gc, ts.elf, words, segment_po2=9, part=0, parts=2)
        hal.set_check_session(False)
        hal.session_begin(gc, ts.elf, words, segment_po2=9, part=0, parts=2).close()        # off: ranks share sessions as before
    finally:
        hal.set_check_session(False)
        gc.free()


def test_cli_round_trip(tmp_path, trace_session):
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    (tmp_path / "guest.elf").write_bytes(trace_session.elf)
    np.array([7, 0x01020304], dtype=np.uint32).tofile(str(tmp_path / "input.bin"))
    receipts = []
    for extra in ([], ["--check-session", "1"]):
        out = subprocess.run([prove, circuit_path("trace"), "--code-object", entry.code_object_path("trace"), "--elf", str(tmp_path / "guest.elf"), "--input", str(tmp_path / "input.bin"),
                              "--po2", "9", "--receipt-out", str(tmp_path / "receipt.json")] + extra, capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        info = json.loads(out.stdout.splitlines()[-1])
        assert info["receipts_verified_with_the_elf"] == 1 and info["segments"] >= 3, out.stdout + out.stderr
        receipts.append((tmp_path / "receipt.json").read_text())
    assert receipts[0] == receipts[1]
