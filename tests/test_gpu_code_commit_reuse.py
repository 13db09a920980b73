"""The CODE group depends on (circuit, po2, hash suite) only, so a context commits it once and every later session reads it
(r0h_ctx::code_commits).  A short guest with the trace circuit at the minimum segment size, one prover lane so that every kernel
of the session is counted on the context whose kernel timing is on: the second prove_elf launches fewer hash_rows_kernels than
the first by exactly the number of distinct segment sizes (one CODE tree each); changing the hash suite and loading the circuit
again both bring the launches back; the receipts are the words a fresh context gives; and a context closed with commitments
cached gives their device memory back at the close."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

pytestmark = pytest.mark.gpu
WORDS = [7, 0x01020304]
SEGMENT_PO2 = 11  # every segment is proved at 2^TRACE_MIN_PO2 rows


def short_guest():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from bench_session import elf_of
    from test_rv32im import _guest
    return elf_of(_guest(300), 0x400)


def prove_counted(hal, circuit, elf):
    hal.kernel_timing(True)
    receipt, _, _ = hal.prove_elf(circuit, elf, WORDS, segment_po2=SEGMENT_PO2)
    launches = hal.kernel_stats()["hash_rows_kernel"]["launches"]
    hal.kernel_timing(False)
    return receipt, launches


@pytest.fixture()
def one_lane(monkeypatch):
    monkeypatch.setenv("R0H_SESSION_LANES", "1")


def test_the_second_session_reads_the_first_one_s_code_commitment(one_lane, orc):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    elf = short_guest()
    fresh = r0.Hal(0)
    fc = fresh.load_circuit(blob, entry.code_object_path("trace"))
    want, _, _ = fresh.prove_elf(fc, elf, WORDS, segment_po2=SEGMENT_PO2)
    want_json = want.to_json()
    sizes = {r0.verify_seal(blob, seal)[2] for _, seal in want.seals()}
    roots = {size: fresh.code_root(fc, size) for size in sizes}
    fc.free()
    fresh.close()

    hal = r0.Hal(0)
    tc = hal.load_circuit(blob, entry.code_object_path("trace"))
    first, n_first = prove_counted(hal, tc, elf)
    second, n_second = prove_counted(hal, tc, elf)
    print("hash_rows_kernel launches: first %d, second %d, distinct sizes %d" % (n_first, n_second, len(sizes)))
    assert n_first - n_second == len(sizes) >= 1
    for receipt in (first, second):
        assert receipt.to_json() == want_json
        assert receipt.verify(blob, roots, None, elf=elf)[:2] == (0, "ok")
    # the suite is changed and changed back: the commitments went with it, the next session commits again
    hal.set_hashfn("sha-256")
    hal.set_hashfn("poseidon2")
    third, n_third = prove_counted(hal, tc, elf)
    assert n_third == n_first and third.to_json() == want_json
    # other Poseidon2 constants: the entry was hashed with the old table and is made again (the receipt is another one); the old
    # table back: made again once more, and the receipt is the first one's
    rc, diag = orc.poseidon2_consts()
    rc2 = rc.copy()
    rc2[0] = (int(rc2[0]) + 1) % 2013265921
    hal.poseidon2_set_consts(rc2, diag)
    other, n_other = prove_counted(hal, tc, elf)
    hal.poseidon2_set_consts(rc, diag)
    back, n_back = prove_counted(hal, tc, elf)
    assert n_other == n_first and n_back == n_first and other.to_json() != want_json and back.to_json() == want_json
    # the circuit is loaded again: the commitments went with the old handle
    _, n_cached = prove_counted(hal, tc, elf)
    tc.free()
    tc = hal.load_circuit(blob, entry.code_object_path("trace"))
    fourth, n_fourth = prove_counted(hal, tc, elf)
    assert n_cached == n_second and n_fourth == n_first and fourth.to_json() == want_json
    assert fourth.verify(blob, roots, None, elf=elf)[:2] == (0, "ok")
    # a session proved in two shares, split into begin and finish, whose commitment is dropped in between (suite changed and back):
    # the shares still own it, and merged they are the receipt above
    n_seg = len(want.seals())
    assert n_seg >= 2
    shares = [hal.session_begin(tc, elf, WORDS, segment_po2=SEGMENT_PO2, part=k, parts=2) for k in range(2)]
    records = np.zeros((n_seg, r0.SESSION_RECORD_WORDS), dtype=np.uint32)
    for ses in shares:
        idx, rec = ses.records()
        records[idx] = rec
    hal.set_hashfn("sha-256")
    hal.set_hashfn("poseidon2")
    merged = r0.Receipt.merge([ses.finish(records)[0] for ses in shares])
    assert merged.to_json() == want_json
    for ses in shares:
        ses.close()
    tc.free()
    hal.close()


CHILD = """
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
sys.path.insert(0, os.path.join(%r, "tools"))
import numpy as np
import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
import torch
from bench_session import elf_of
from test_rv32im import _guest
blob = np.fromfile(entry.circuit_blob_path("trace"), dtype=np.uint32)
elf = elf_of(_guest(300), 0x400)
def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]
""" % (ROOT, ROOT, ROOT)


def test_closing_a_context_with_cached_commitments_frees_them():
    """A child process, as in test_gpu_teardown: an abort at teardown is an exit status.  The device's free memory is read with the
    commitment cached, after the close (the circuit still alive, so the context's own state stays) and after the circuit has gone.
    The close alone must give back the commitment's two large buffers, the 4x evaluations and the tree nodes (whole multiples of the
    2 MiB the device's allocator hands out; the CODE columns and the coefficients, 1.5 MiB each for the trace circuit, come out of
    chunks it may share and keep), and a second round must end where the first one ended: nothing is left per context."""
    body = """
        n = 1 << r0.TRACE_MIN_PO2
        ends = []
        for cycle in range(2):
            hal = r0.Hal(0)
            tc = hal.load_circuit(blob, entry.code_object_path("trace"))
            code_cols = tc.group_size[r0.GROUP_CODE]
            hal.prove_elf(tc, elf, [7, 0x01020304], segment_po2=11)
            cached = free_bytes()
            hal.close()
            closed = free_bytes()
            tc.free()
            ends.append(free_bytes())
            large = code_cols * 4 * n * 4 + 2 * 4 * n * 32
            print("cycle", cycle, "freed at close", closed - cached, "evaluations + nodes", large, "end", ends[-1])
            assert closed - cached >= large, (closed - cached, large)
        assert abs(ends[1] - ends[0]) < large // 2, ends
        print("no buffer left")
    """
    out = subprocess.run([sys.executable, "-c", CHILD + textwrap.dedent(body)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert out.returncode == 0 and "no buffer left" in out.stdout and "terminate" not in out.stderr, (out.stdout[-2000:], out.stderr[-2000:])
