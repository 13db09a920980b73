"""The surface of r0h_ctx_set_merkle_fused_tops without a GPU: the new entry points are in the header, the Rust bindings, the library and
the harness; r0h_prove --help names --merkle-fused-tops, and a value other than 0 or 1 is refused, exit status 1, before the blob is
opened or a device touched; the plan of the fused launches is clean under AddressSanitizer and UndefinedBehaviorSanitizer
(tools/fuzz/run_merkle_fused_check.sh: a stand-alone host program)."""
import os
import re
import subprocess

from conftest import ROOT

CLI = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
SYMBOLS = ("r0h_hash_fold_top", "r0h_ctx_set_merkle_fused_tops")


def test_header_bindings_library_and_harness_name_the_entry_points():
    import hyperfridge_r0_amd as r0
    header = open(os.path.join(ROOT, "include", "r0hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for symbol in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert "pub fn %s(" % symbol in rust, symbol
        assert getattr(r0.lib(), symbol) is not None and symbol in r0.EXPORTED_SYMBOLS
    assert "OFF BY DEFAULT" in header[header.index("r0h_ctx_set_merkle_fused_tops(ctx, on != 0)"):header.index("const char* r0h_hash_fold_top(")]
    for method in ("hash_fold_top", "set_merkle_fused_tops"):
        assert callable(getattr(r0.Hal, method))


def test_help_names_the_flag():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--merkle-fused-tops 0|1" in out.stdout and "R0H_MERKLE_FUSED_TOPS" in out.stdout


def test_any_other_value_is_refused_before_the_blob_is_opened(tmp_path):
    for value in ("2", "on", "-1", ""):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--merkle-fused-tops", value], capture_output=True, text=True)
        assert out.returncode == 1, (value, out.returncode, out.stderr)
        assert out.stderr == "r0h_prove: --merkle-fused-tops is 0 or 1, not %s\n" % value
    for value in ("0", "1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--merkle-fused-tops", value], capture_output=True, text=True)
        assert out.returncode == 1 and "cannot open" in out.stderr and "--merkle-fused-tops" not in out.stderr


def test_the_benchmarks_take_the_flag():
    for tool in ("bench_session.py", "bench_recursion.py"):
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert '"--merkle-fused-tops"' in text and "set_merkle_fused_tops" in text, tool
    assert "hal.hash_fold_top(nodes, 8192)" in open(os.path.join(ROOT, "tools", "bench_ops.py")).read()


def test_the_plan_is_clean_under_asan_and_ubsan(tmp_path):
    out = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "run_merkle_fused_check.sh"), str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    assert "merkle fused check: no report" in out.stdout and "split 7" in out.stdout
