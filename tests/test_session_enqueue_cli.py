"""The surface of r0h_ctx_set_session_enqueue without a GPU: the new entry points are in the header, the Rust bindings, the library and
the harness; r0h_prove --help names --session-enqueue, and a value other than 0 or 1 (or the flag without --elf) is a usage error,
exit status 2, before the blob is opened."""
import os
import re
import subprocess

from conftest import ROOT

CLI = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
SYMBOLS = ("r0h_proof_late_device", "r0h_logup_totals_device", "r0h_accum_public_device", "r0h_ctx_set_session_enqueue", "r0h_last_session_phase2")


def test_header_bindings_library_and_harness_name_the_entry_points():
    import hyperfridge_r0_amd as r0
    header = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for symbol in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert "pub fn %s(" % symbol in rust, symbol
        assert getattr(r0.lib(), symbol) is not None and symbol in r0.EXPORTED_SYMBOLS
    # beside r0h_proof_late, as the late step's other form
    assert 0 < header.index("const char* r0h_proof_late_device(") - header.index("const char* r0h_proof_late(") < 3000
    for method in ("proof_late_device", "logup_totals_device", "accum_public_device", "set_session_enqueue", "last_session_phase2"):
        assert callable(getattr(r0.Hal, method))


def test_help_names_the_flag():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--session-enqueue 0|1" in out.stdout and "R0H_SESSION_ENQUEUE" in out.stdout


def test_any_other_value_is_a_usage_error_before_the_blob_is_opened(tmp_path):
    elf = tmp_path / "guest.elf"
    elf.write_bytes(b"\x7fELF")
    for value in ("2", "on", "-1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--elf", str(elf), "--session-enqueue", value], capture_output=True, text=True)
        assert out.returncode == 2, (value, out.returncode, out.stderr)
        assert "--session-enqueue is 0 or 1" in out.stderr and "cannot open" not in out.stderr
    out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--session-enqueue", "1"], capture_output=True, text=True)   # no --elf: no session
    assert out.returncode == 2 and "goes with --elf" in out.stderr
    for value in ("0", "1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--elf", str(elf), "--session-enqueue", value], capture_output=True, text=True)
        assert out.returncode == 1 and "cannot open" in out.stderr


def test_the_session_benchmark_takes_the_flag():
    text = open(os.path.join(ROOT, "tools", "bench_session.py")).read()
    assert '"--session-enqueue"' in text and "set_session_enqueue" in text
