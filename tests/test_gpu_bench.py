"""bench.py keeps the driver's contract: one JSON line with the agreed keys (checked on a small, fast configuration); a plain run
(no --full) times only the headline and can write what it computed (--dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--po2", "12",
                          "--circuit", "small", "--cpu-po2", "10", "--contexts", "2", "--full"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "segments/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["vs_baseline"] is None
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["data"] == "synthetic" and d["dtype"] == "u32"
    assert "workload" in d["config"] and "model" not in d["config"]
    assert abs(d["value"] - 2 * 2 / (d["ms_per_step"] * 2 / 1e3)) / d["value"] < 0.02  # value = segments / time
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-4
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["value"] > 0 and "sample" in c


def test_the_rccl_path_of_the_driver_runs_with_one_rank():
    """The multi-GPU runs go through torch.distributed with backend "nccl" (= RCCL): process group bound to the rank's device, barrier
    around the timed region, MAX / SUM all-reduces of device tensors.  A one-GPU box cannot hold two RCCL ranks, but it can hold one:
    R0H_FORCE_PROCESS_GROUP=1 builds the group for a single rank, so the very calls the 8-GPU run makes are executed here."""
    env = dict(os.environ, R0H_FORCE_PROCESS_GROUP="1", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29631")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--po2", "12", "--circuit", "small",
                          "--cpu-po2", "0", "--contexts", "2", "--backend", "nccl"], capture_output=True, text=True, cwd=ROOT, env=env, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.strip()][-1])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["steps"] == 2


def _npy(dirpath):
    import numpy as np
    files = sorted(os.listdir(dirpath))
    assert files and all(f.endswith(".npy") for f in files), files
    assert sum(os.path.getsize(os.path.join(dirpath, f)) for f in files) <= 64 << 20
    out = {f[:-4]: np.load(os.path.join(dirpath, f)) for f in files}
    for name, a in out.items():
        assert a.dtype == np.float64 and np.array_equal(a, np.round(a)), name  # words and bytes, exact
    return out


def test_plain_run_times_the_headline_only_and_dumps_its_seals(tmp_path):
    """Without --full the line keeps its keys, but what a plain run does not measure is null; --dump-outputs writes every
    context's seal of the last timed step, and each is a seal the host verifier accepts."""
    import numpy as np
    import hyperfridge_r0_amd as r0
    from conftest import circuit_path
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--po2", "12",
                          "--circuit", "small", "--contexts", "2", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "segments/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3 / 1e3)) / d["value"] < 0.02
    for key in ("roofline", "cpu_baseline", "kernels_ms_per_segment", "value_with_code_committed_in_every_proof", "value_with_witgen_in_timed_region"):
        assert d[key] is None, key
    got = _npy(str(tmp_path))
    assert sorted(got) == ["lane0_seal", "lane1_seal"]
    blob = np.fromfile(circuit_path("small"), dtype=np.uint32)
    for name, seal in got.items():
        assert seal.size == d["config"]["seal_words"] and r0.verify_seal(blob, seal.astype(np.uint32))[0] == 0, name
    assert not np.array_equal(got["lane0_seal"], got["lane1_seal"])  # each context proves its own witness


def test_plain_run_of_the_headline_dumps_the_receipt_of_its_last_step(tmp_path):
    """The default workload (sessions of the camt53 guest), one timed step: the dumped receipt is the session's -- its journal is
    the reference receipt fixture's, its image id the ELF's, and every seal of it is accepted by the host verifier."""
    import numpy as np
    import hyperfridge_r0_amd as r0
    from conftest import circuit_path
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import guest_camt53
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0", "--contexts", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 1 and d["warmup"] == 0 and d["unit"] == "segments/s" and d["ms_per_step"] > 0 and d["value"] > 0
    for key in ("roofline", "cpu_baseline", "synthetic_bench_circuit", "receipts_verified_with_the_elf", "journal_is_the_reference_receipt_fixtures"):
        assert d[key] is None, key
    got = _npy(str(tmp_path))
    assert sorted(got) == ["image_id", "session0_claim_digests", "session0_image_proof", "session0_journal", "session0_seal_index_and_words", "session0_seals"]
    image, _, _ = guest_camt53.elf_and_input(form=1)
    assert bytes(got["image_id"].astype(np.uint8)) == r0.compute_image_id(image)
    want = bytes(json.load(open(os.path.join(ROOT, "tests", "golden", "reference_receipt_6bb95807_latest.json")))["journal"]["bytes"])
    assert bytes(got["session0_journal"].astype(np.uint8)) == want
    index = got["session0_seal_index_and_words"].astype(np.int64)
    assert len(index) == d["config"]["segments_per_session"] == len(got["session0_claim_digests"])
    assert list(index[:, 0]) == list(range(len(index))) and index[:, 1].sum() == got["session0_seals"].size
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    seals = np.split(got["session0_seals"].astype(np.uint32), np.cumsum(index[:, 1])[:-1])
    assert all(r0.verify_seal(blob, s)[0] == 0 for s in seals)
