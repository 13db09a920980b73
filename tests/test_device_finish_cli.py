"""r0h_prove --device-finish 0|1 (r0h_ctx_set_device_finish of every context the run makes): named by --help, and any other value is a
usage error, exit status 2, before the blob is opened, let alone a device touched.  No GPU."""
import os
import subprocess

from conftest import ROOT, circuit_path

CLI = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")


def test_help_names_the_switch():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--device-finish 0|1" in out.stdout


def test_any_other_value_is_a_usage_error_before_the_blob_is_opened(tmp_path):
    for value in ("2", "on", "-1", ""):
        # (a circuit file that does not exist: the value is refused before the blob is opened)
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--device-finish", value], capture_output=True, text=True)
        assert out.returncode == 2, (value, out.returncode, out.stderr)
        assert "--device-finish is 0 or 1" in out.stderr and "cannot open" not in out.stderr
    out = subprocess.run([CLI, circuit_path("tiny"), "--device-finish", "2"], capture_output=True, text=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES=""))
    assert out.returncode == 2 and "--device-finish is 0 or 1, not 2" in out.stderr


def test_the_two_values_get_past_the_usage_check(tmp_path):
    for value in ("0", "1"):
        out = subprocess.run([CLI, str(tmp_path / "missing.r0c"), "--device-finish", value], capture_output=True, text=True)
        assert out.returncode == 1 and "cannot open" in out.stderr


def test_the_library_and_the_harness_name_the_switch_and_the_two_halves():
    import hyperfridge_r0_amd as r0
    for symbol in ("r0h_ctx_set_device_finish", "r0h_proof_finish_enqueue", "r0h_proof_finish_collect"):
        assert getattr(r0.lib(), symbol) is not None
    for method in ("set_device_finish", "proof_finish_enqueue", "proof_finish_collect"):
        assert callable(getattr(r0.Hal, method))
