"""Sessions whose evicted segments keep the top of their DATA tree (r0h_ctx_set_session_tree_tops) and are committed again without
hashing.  The two small sessions of tests/test_gpu_session_eviction.py, every segment a 2^16-row trace: a 2^18-row domain, whose top at
six levels is (2 * 2^18 >> 6) digests = 262,144 bytes.  Every case holds the receipt byte for byte against the session proved with no
limit, and after every case nothing of a session is left on the device."""
import json
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

from test_gpu_session_eviction import PO2, circuit, nothing_left_behind, session, six, three  # noqa: E402,F401
from test_session_balance import trace_session  # noqa: E402,F401

pytestmark = pytest.mark.gpu
LEVELS = 6
TOP_BYTES = ((2 * (4 << PO2)) >> LEVELS) * 32


def prove(hal, s, limit, levels=LEVELS):
    hal.set_session_device_limit(limit)
    hal.set_session_tree_tops(levels)
    try:
        receipt, image_id, _ = hal.prove_elf(s.gc, s.elf, s.words, segment_po2=s.po2)
    finally:
        hal.set_session_device_limit(0)
        hal.set_session_tree_tops(0)
    return receipt, image_id, hal.last_session_device(), hal.last_session_tree_tops()


def test_the_top_of_a_trace_segment_is_a_quarter_mebibyte():
    assert TOP_BYTES == 262144


@pytest.mark.parametrize("which", ["three", "six"])
def test_every_segment_evicted_is_replayed_from_its_top(hal, request, which):
    s = request.getfixturevalue(which)
    receipt, image_id, dev, tops = prove(hal, s, 1)
    assert receipt.to_json() == s.json and image_id == s.image_id
    assert receipt.verify(s.blob, {PO2: hal.code_root(s.gc, PO2)}, None, elf=s.elf)[:2] == (0, "ok")
    assert dev["evicted"] == dev["replayed"] == tops["replayed_from_top"] == s.n
    assert tops["levels"] == LEVELS and tops["tops_bytes"] == s.n * TOP_BYTES
    assert dev["peak_counted_bytes"] == 0 and dev["rows_bytes"] == s.roomy["rows_bytes"]


@pytest.mark.parametrize("levels", [1, 8])
def test_other_levels_give_the_same_receipt(hal, three, levels):
    receipt, _, dev, tops = prove(hal, three, 1, levels)
    assert receipt.to_json() == three.json
    assert tops == {"replayed_from_top": three.n, "tops_bytes": three.n * (((2 * (4 << PO2)) >> levels) * 32), "levels": levels}


def test_levels_above_eight_are_refused_by_name(hal):
    with pytest.raises(r0.R0HipError, match=r"r0h_ctx_set_session_tree_tops: levels 9 outside \[0, 8\]"):
        hal.set_session_tree_tops(9)


def test_tops_without_a_device_limit_change_nothing(hal, six):
    receipt, _, dev, tops = prove(hal, six, 0)
    assert receipt.to_json() == six.json
    assert dev["evicted"] == dev["replayed"] == 0 and tops == {"replayed_from_top": 0, "tops_bytes": 0, "levels": 0}
    assert dev["peak_counted_bytes"] == six.unlimited["peak_counted_bytes"] and dev["rows_bytes"] == 0


def test_a_limit_of_one_segment_keeps_one(hal, six):
    receipt, _, dev, tops = prove(hal, six, six.per_segment + 1)
    assert receipt.to_json() == six.json
    assert dev["evicted"] == dev["replayed"] == tops["replayed_from_top"] == six.n - 1
    assert 0 < dev["peak_counted_bytes"] <= six.per_segment + 1 and tops["tops_bytes"] == (six.n - 1) * TOP_BYTES


def test_between_the_phases_a_session_holds_its_rows_and_its_tops(hal, six):
    """two shares on one GPU: the form that shows the middle"""
    hal.set_session_device_limit(1)
    hal.set_session_tree_tops(LEVELS)
    sessions = [hal.session_begin(six.gc, six.elf, six.words, segment_po2=six.po2, part=k, parts=2) for k in range(2)]
    hal.set_session_device_limit(0)  # (both taken per session when it began)
    hal.set_session_tree_tops(0)
    records = np.zeros((six.n, r0.SESSION_RECORD_WORDS), dtype=np.uint32)
    for ses in sessions:
        idx, rec = ses.records()
        records[idx] = rec
    assert hal.session_held_bytes() == six.roomy["rows_bytes"] + six.n * TOP_BYTES
    receipts, from_top = [], 0
    for ses in sessions:
        receipts.append(ses.finish(records)[0])
        from_top += hal.last_session_tree_tops()["replayed_from_top"]
        ses.close()
    assert r0.Receipt.merge(receipts[::-1]).to_json() == six.json and from_top == six.n
    assert hal.session_held_bytes() == 0


def test_with_the_image_circuit_set(hal, three):
    iblob = np.fromfile(circuit_path("image"), dtype=np.uint32)
    ic = hal.load_circuit(iblob, entry.code_object_path("image"))
    hal.set_image_circuit(ic)
    try:
        want, _, _, _ = prove(hal, three, 0, 0)
        receipt, image_id, dev, tops = prove(hal, three, 1)
    finally:
        hal.set_image_circuit(None)
        ic.free()
    assert want.image_proof is not None and np.array_equal(receipt.image_proof, want.image_proof)
    assert receipt.to_json() == want.to_json() != three.json and tops["replayed_from_top"] == three.n
    assert [np.array_equal(a, b) for (_, a), (_, b) in zip(receipt.seals(), r0.Receipt.parse(three.json).seals())] == [True] * three.n
    assert receipt.verify_image(three.blob, {PO2: hal.code_root(three.gc, PO2)}, iblob, image_id)[:2] == (0, "ok")


def test_the_session_check_sees_segments_that_kept_their_tops(hal, three):
    hal.set_check_session(True)
    try:
        receipt, _, dev, tops = prove(hal, three, 1)
        assert "check_session" in [n for n, _ in hal.last_profile()]
    finally:
        hal.set_check_session(False)
    assert receipt.to_json() == three.json and dev["evicted"] == tops["replayed_from_top"] == three.n


def test_a_session_given_up_between_its_phases_leaves_nothing(hal, three):
    hal.set_session_device_limit(1)
    hal.set_session_tree_tops(LEVELS)
    ses = hal.session_begin(three.gc, three.elf, three.words, segment_po2=three.po2)
    hal.set_session_device_limit(0)
    hal.set_session_tree_tops(0)
    held = hal.session_held_bytes()
    assert held == three.roomy["rows_bytes"] + three.n * TOP_BYTES
    _, records = ses.records()
    records[0, 0] ^= 1
    with pytest.raises(r0.R0HipError, match="record 0 is not the one this rank committed"):
        ses.finish(records)
    assert hal.session_held_bytes() == held
    ses.close()
    assert hal.session_held_bytes() == 0
    receipt, _, _, tops = prove(hal, three, 1)  # and the context goes on working
    assert receipt.to_json() == three.json and tops["replayed_from_top"] == three.n


def test_cli_round_trip(tmp_path, three):
    prove_cli = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    (tmp_path / "guest.elf").write_bytes(three.elf)
    np.array(three.words, dtype=np.uint32).tofile(str(tmp_path / "input.bin"))
    out = subprocess.run([prove_cli, circuit_path("trace"), "--code-object", entry.code_object_path("trace"), "--elf", str(tmp_path / "guest.elf"), "--input",
                          str(tmp_path / "input.bin"), "--po2", "9", "--receipt-out", str(tmp_path / "receipt.json"), "--session-device-limit-gb", "0.000001",
                          "--session-keep-tree-tops", str(LEVELS)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    info = json.loads(out.stdout.splitlines()[-1])
    assert info["receipts_verified_with_the_elf"] == 1 and info["segments"] == info["evicted_segments"] == info["segments_replayed_from_their_tree_top"] == three.n, out.stdout
    assert (tmp_path / "receipt.json").read_text() == three.json
