"""The correction schedule compiled into the Poseidon2 kernels (csrc/poseidon2_dot_schedule.hpp) is the one the rule gives for the
table of include/r0hip_poseidon2_consts.h, recomputed here in Python integers; and the dot-product routines themselves, compiled for
the host with every bound asserted in 128-bit arithmetic, run clean under AddressSanitizer and UndefinedBehaviorSanitizer at the exact
worst case and on random states (tools/fuzz/run_p2_dot_check.sh: a stand-alone program, no GPU, nothing preloaded)."""
import os
import subprocess

import pytest

import p2_dot_ref as ref
from conftest import ROOT


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    work = str(tmp_path_factory.mktemp("p2_dot_check"))
    out = subprocess.run([os.path.join(ROOT, "tools", "fuzz", "run_p2_dot_check.sh"), work], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0, out.stdout
    return os.path.join(work, "p2_dot_check"), out.stdout


def test_the_rule_gives_258_corrections_and_little_slack():
    _, diag = ref.header_tables()
    rows = ref.dot_rows(diag)
    tight, safe = ref.schedule(rows), ref.safe_schedule()
    assert ref.corrections(tight) == 258 and ref.corrections(safe) == 550
    assert ref.covers(tight, rows) and ref.covers(safe, rows)
    every_word_at_the_top = [[ref.P - 1] * len(k) for k in rows]
    assert ref.covers(safe, every_word_at_the_top) and not ref.covers(tight, every_word_at_the_top)
    assert ref.schedule(every_word_at_the_top) == [m & ~(1 << ref.END) | (len(k) % 2 == 0) << ref.END for m, k in zip(safe, rows)]
    minus_one = ref.dot_rows([ref.P - 1] * ref.CELLS)  # the uncovered diagonal of tests/test_gpu_p2_dot_schedule.py
    assert ref.covers(safe, minus_one) and not ref.covers(tight, minus_one)
    assert ref.covers(tight, ref.dot_rows([diag[0] // 2] + diag[1:]))  # ... and its covered one


def test_the_compiled_masks_are_the_rules(checker):
    program, _ = checker
    lines = subprocess.run([program, "--masks"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    got = {"tight": {}, "safe": {}}
    for line in filter(None, lines):
        name, row, mask = line.split()
        got[name][int(row)] = int(mask, 16)
    _, diag = ref.header_tables()
    assert [got["tight"][r] for r in range(ref.ROWS)] == ref.schedule(ref.dot_rows(diag))
    assert [got["safe"][r] for r in range(ref.ROWS)] == ref.safe_schedule()


def test_the_host_build_of_the_dot_products_runs_clean_under_the_sanitizers(checker):
    _, report = checker
    assert "p2 dot check: no report (258 + 550 corrections per permutation" in report, report
