"""The surface of a proof's enqueued first half and of the two-call image proof without a GPU: the new entry points are in the header,
the Rust bindings, the library and the harness, and the harness refuses the columns form before it calls the library."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

SYMBOLS = ("r0h_proof_begin_committed_enqueue", "r0h_proof_begin_committed_top_enqueue", "r0h_proof_data_root_device", "r0h_prove_segment_committed_enqueue",
           "r0h_prove_segment_collect", "r0h_accum_mixbuf", "r0h_prove_image_enqueue", "r0h_prove_image_collect", "r0h_prove_image_abort")
METHODS = ("proof_begin_enqueue", "proof_data_root", "proof_data_root_device", "prove_segment_enqueue", "prove_segment_collect", "accum_mixbuf", "prove_image_enqueue",
           "prove_image_collect", "prove_image_abort")


def test_header_bindings_library_and_harness_name_the_entry_points():
    import hyperfridge_r0_amd as r0
    header = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for symbol in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert "pub fn %s(" % symbol in rust, symbol
        assert getattr(r0.lib(), symbol) is not None and symbol in r0.EXPORTED_SYMBOLS
    for method in METHODS:
        assert callable(getattr(r0.Hal, method))


def test_the_columns_form_is_refused_by_the_harness_before_any_library_call():
    import hyperfridge_r0_amd as r0

    class NotACommit:
        handle = None

    for method in (r0.Hal.proof_begin_enqueue, r0.Hal.prove_segment_enqueue):
        with pytest.raises(r0.R0HipError, match="the columns form commits CODE with a read-back that waits: .*r0h_code_commit_new"):
            method(None, None, 9, NotACommit(), None, [])


CLI = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")


def test_the_session_switch_is_on_every_surface():
    import hyperfridge_r0_amd as r0
    header = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for symbol in ("r0h_ctx_set_session_enqueue_begin", "r0h_last_session_phase1"):
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert "pub fn %s(" % symbol in rust, symbol
        assert getattr(r0.lib(), symbol) is not None and symbol in r0.EXPORTED_SYMBOLS
    assert callable(r0.Hal.set_session_enqueue_begin) and callable(r0.Hal.last_session_phase1)
    text = open(os.path.join(ROOT, "tools", "bench_session.py")).read()
    assert '"--session-enqueue-begin"' in text and "set_session_enqueue_begin" in text


def test_help_names_the_flag():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--session-enqueue-begin 0|1" in out.stdout and "R0H_SESSION_ENQUEUE_BEGIN" in out.stdout


def test_any_other_value_is_a_usage_error_before_the_blob_is_opened(tmp_path):
    elf = tmp_path / "guest.elf"
    elf.write_bytes(b"\x7fELF")
    for value in ("2", "on", "-1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--elf", str(elf), "--session-enqueue-begin", value], capture_output=True, text=True)
        assert out.returncode == 2, (value, out.returncode, out.stderr)
        assert "--session-enqueue-begin is 0 or 1" in out.stderr and "cannot open" not in out.stderr
    out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--session-enqueue-begin", "1"], capture_output=True, text=True)   # no --elf: no session
    assert out.returncode == 2 and "goes with --elf" in out.stderr
    for value in ("0", "1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--elf", str(elf), "--session-enqueue-begin", value], capture_output=True, text=True)
        assert out.returncode == 1 and "cannot open" in out.stderr
