"""CPU side of the witness checker (r0h_check_witness): term numbering, the generated text, the names, the command line, and the
numpy reference the GPU tests hold the device against (tests/check_ref.py) pinned on the trace circuit -- silent on honest host
witnesses, and naming what tools/gen_circuit.py check_trace_rows names on the forgeries tests/test_trace_circuit.py constructs."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_circuit  # noqa: E402
import check_ref  # noqa: E402
import trace_circuit as tc  # noqa: E402
import trace_corners as corners  # noqa: E402
from test_trace_circuit import _run  # noqa: E402
from trace_corners import COL, P, R_INV, canonical  # noqa: E402

CIRCUITS = ("tiny", "small", "bench", "recursion", "trace", "image")
# sha256 of r0h_circuit_emit_hip's text per circuit, recorded from the build of the commit before the checker existed: adding the
# second emit mode must not move a byte of eval_check
EVAL_CHECK_SHA256 = {
    "tiny": "8dd920df399630886bd09b363afaa6cc8006c089750881ef817ec09dbe08a563",
    "small": "b869c6baf45869f7e208d322ed9b07ca201f748f92734cf340bbf5532df8ef5f",
    "bench": "4b2a24c4f1cd099b5a1445939769b5b0b564f19d34b48a60ede9e25e6631a5af",
    "recursion": "10b7121dc8ae28809ffc72770ea8fc9960dd47c9fa0a65c1c42dff84f585ed36",
    "trace": "25c760bef0c453d0dc3f2ac398b8b53ad07c59336a629c3f915761704c4a7dc0",
    "image": "7a4110f0e9df0116395d0b0047f931195794bdbce6af4655251bbdde4a82928e",
}
# the same for r0h_circuit_emit_hip_check's text, recorded from the build of the commit before the generator moved out of circuit.hip
# (no R0H_EC_* variable set): neither the move nor the one function that now writes a term's value for both emitters moved a byte
CHECK_WITNESS_SHA256 = {
    "tiny": "573511f972e6e6440f436528d5cd97040ebe647344cbb9b41cfc28cf893f4869",
    "small": "5359c75a3c05934656fd44a5fd7326f475fca81067fcd4e7192b0637414e0099",
    "bench": "3960542b8ff1b07cef305e2c647406e33dfc4ff31ac9b0db8e4af7a18d90feee",
    "recursion": "21f1613ba62167ba333b7846eecb7fbf210421f9a0b7a8de3a9905b5c3a07dd6",
    "trace": "d1c2f566f1b1fd93d51f7c6ad6858b752b59c0b0cf3e566a4d84a1d3bca2e4ed",
    "image": "1512c2dc54759170fa1670e5574da7675b791739fd76df3bd3dc39d4d3281899",
}


def blob_of(name):
    return np.fromfile(circuit_path(name), dtype=np.uint32)


@pytest.mark.parametrize("name", CIRCUITS)
def test_terms_are_the_and_eqz_steps_and_eval_check_text_is_the_parents(name):
    blob = blob_of(name)
    pr = check_ref.Program(blob)
    src = r0.emit_check_witness_source(blob)
    assert src == r0.emit_check_witness_source(blob)
    n_terms = int(src.split("// terms: ")[1].split(",")[0])
    assert n_terms == pr.n_and_eqz == len(pr.terms)
    # every term is tallied exactly once, under its own number, in kernels numbered from 0
    tallied = sorted(int(x.split("u,")[0]) for x in src.split("  tally(table, ")[1:])
    assert tallied == list(range(n_terms))
    kernels = [x.split("(")[0] for x in src.split("void check_witness_")[1:]]
    assert kernels == [str(k) for k in range(len(kernels))] and kernels
    # the terms behind the accumulation switch are the reference's late terms
    late = set()
    for part in src.split("  if (with_accum) {\n")[1:]:
        late |= {int(x.split("u,")[0]) for x in ("\n" + part).split("\n  }\n")[0].split("  tally(table, ")[1:]}
    assert late == {t for t in range(n_terms) if pr.late[t]}
    assert hashlib.sha256(r0.emit_eval_check_source(blob).encode()).hexdigest() == EVAL_CHECK_SHA256[name]
    assert hashlib.sha256(src.encode()).hexdigest() == CHECK_WITNESS_SHA256[name]


def test_n_terms_is_exported_and_a_bad_blob_is_refused():
    assert "r0h_circuit_n_terms" in r0.EXPORTED_SYMBOLS and "r0h_check_witness" in r0.EXPORTED_SYMBOLS
    bad = blob_of("tiny").copy()
    bad[0] ^= 1
    with pytest.raises(r0.R0HipError):
        r0.emit_check_witness_source(bad)


@pytest.mark.parametrize("name", ("tiny", "trace"))
def test_the_checker_text_compiles_for_gfx950(name, tmp_path):
    src = tmp_path / (name + ".check.hip")
    src.write_text(r0.emit_check_witness_source(blob_of(name)))
    out = subprocess.run(["/opt/rocm/bin/hipcc", "--genco", "--offload-arch=gfx950", "-O3", "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "check.hsaco"), str(src)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    scratch = [int(line.split(":")[-1].split("[")[0]) for line in out.stderr.splitlines() if "ScratchSize" in line]
    assert scratch and max(scratch) == 0, "the checker spills: %r" % scratch


def test_term_names_follow_the_generators_constraint_lists():
    for name in CIRCUITS:
        if name in ("bench", "recursion"):
            continue  # (minutes of Python to regenerate; their names are ordinals like tiny's and small's)
        names = gen_circuit.term_names(name)
        assert len(names) == check_ref.Program(blob_of(name)).n_and_eqz
        if name in ("tiny", "small"):
            assert names == ["term:%d" % t for t in range(len(names))]
    _, cons = gen_circuit.trace_constraints()
    assert gen_circuit.term_names("trace") == [c[0] for c in cons] and len(set(c[0] for c in cons)) == len(cons)
    # a constraint's variable is its term's AndEqz operand, and `touches ACCUM` is the reference's `late`
    pr = check_ref.Program(blob_of("trace"))
    assert [v for v, gates in pr.terms] == [c[1] for c in cons] and all(not gates for _, gates in pr.terms)
    assert pr.late == [bool(c[3]) for c in cons]
    import image_circuit
    _, icons = image_circuit.constraints(gen_circuit.Builder, gen_circuit.E, gen_circuit.fp4_mul_sym)
    assert gen_circuit.term_names("image") == [c[0] for c in icons]


def test_the_command_line_documents_the_switch():
    out = subprocess.run([os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove"), "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--check-witness 1" in out.stdout and "--term-names" in out.stdout


@pytest.mark.parametrize("prog", sorted(corners.PROGRAMS))
def test_the_reference_is_silent_on_honest_trace_witnesses(orc, prog):
    """the host witness (r0h_vm_trace_witness) of every corner program, with the oracle's CODE columns, totals and accumulation: no
    term of the trace circuit objects, before the mix (no ACCUM) or after it"""
    blob = blob_of("trace")
    po2 = r0.TRACE_MIN_PO2
    vm = corners.run(corners.PROGRAMS[prog](), expect=(0, 0x00050003) if prog == "ecall" else (0, 0))
    data, glob = vm.trace_witness(0, po2)
    oc = orc.circuit(blob)
    code = oc.witgen(po2, 0)[0]
    assert check_ref.check(blob, po2, code, data, glob) == {}
    if prog == "alu":  # the accumulation under a challenge, once
        rng = np.random.default_rng(5)
        glob = glob.copy()
        glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = [orc.enc(int(v)) for v in rng.integers(0, P, 16)]
        full = oc.logup_totals(po2, code, data, glob)
        mix = np.array([orc.enc(int(v)) for v in rng.integers(0, P, oc.n_mix)], dtype=np.uint32)
        accum = oc.accum_public(po2, code, data, full, mix)
        assert check_ref.check(blob, po2, code, data, full, accum, mix) == {}
        accum[3 * (1 << po2) + 77] ^= 1  # one ACCUM cell: only terms that wait for the accumulation may object
        got = check_ref.check(blob, po2, code, data, full, accum, mix)
        pr = check_ref.Program(blob)
        assert got and all(pr.late[t] for t in got)
        # the single-cell mutations the GPU test makes of this witness: the early terms alone meet the cap of one silent in ten
        sites = check_ref.mutations(blob, po2, seed=13, count=10, columns=[COL[c] for c in check_ref.TRACE_MUTATION_COLUMNS], rows=len(vm.preflight(0)))
        assert [r for _, r, _ in sites[:2]] == [0, (1 << po2) - 1]
        silent = 0
        for col, row, word in sites:
            bad = data.copy()
            bad[col * (1 << po2) + row] = word
            silent += not check_ref.check(blob, po2, code, bad, glob)
        assert silent * 10 <= len(sites)


@pytest.mark.parametrize("name,po2", [("tiny", 9), ("small", 10)])
def test_the_reference_on_the_synthetic_circuits_and_the_mutation_plan(orc, name, po2):
    """honest synthetic witnesses (the oracle's witgen and accumulation) satisfy every term; the single-cell mutations the GPU test
    makes (check_ref.mutations: derived DATA columns, rows 0 and N - 1 among them) are caught by the reference alone -- the cap
    of one silent mutation in ten is met here, before any device is involved"""
    blob = blob_of(name)
    oc = orc.circuit(blob)
    code, data, glob = oc.witgen(po2, 7)
    mix = np.array([orc.enc(int(v)) for v in np.random.default_rng(1).integers(0, P, oc.n_mix)], dtype=np.uint32)
    accum = oc.accum(po2, code, data, mix)
    assert check_ref.check(blob, po2, code, data, glob, accum, mix) == {}
    assert check_ref.check(blob, po2, code, data, glob) == {}
    sites = check_ref.mutations(blob, po2, seed=11, count=20)
    assert {r for _, r, _ in sites} >= {0, (1 << po2) - 1}
    silent = 0
    for col, row, word in sites:
        bad = data.copy()
        bad[col * (1 << po2) + row] = word
        got = check_ref.check(blob, po2, code, bad, glob, accum, mix)
        silent += not got
        early = check_ref.check(blob, po2, code, bad, glob)
        pr = check_ref.Program(blob)
        assert early == {t: v for t, v in got.items() if not pr.late[t]}
    assert silent * 10 <= len(sites)


def test_the_reference_names_what_check_trace_rows_names_on_the_known_forgeries():
    blob = blob_of("trace")
    names = gen_circuit.term_names("trace")
    po2 = r0.TRACE_MIN_PO2
    vm, base = _run()
    rows = vm.preflight(0)
    n, N = len(rows), 1 << po2
    data, glob = vm.trace_witness(0, po2)
    m0 = canonical(data, po2)
    g = [int(x) * R_INV % P for x in glob]
    code = np.array(tc.code_columns(N), dtype=np.uint64)
    mid = n // 2
    rd = next(r for r, w in enumerate(rows) if w.mem_kind == r0.MEM_READ)
    br = next(r for r, w in enumerate(rows) if (w.insn & 0x7f) == 0x63 and w.next_pc != w.pc + 4)
    alu = next(r for r, w in enumerate(rows) if (w.insn & 0x7f) == 0x13 and r > 4)
    forgeries = [
        [("next_pc", mid, 0x5000)], [("cycle", mid, mid + 1)], [("live", mid, 0)], [("live", N - 1, 1)], [("mem_wr", mid, 2)],
        [("after_lo", rd, (rows[rd].mem_after & 0xffff) ^ 1)], [("opc_branch", br, 0)],
        [("next_pc", br, rows[br].pc + 8), ("pc", br + 1, rows[br].pc + 8)], [("next_pc", alu, rows[alu].pc + 8), ("pc", alu + 1, rows[alu].pc + 8)],
        [("opc_jal", alu, 1)], [("pc", 0, 0x5000)],
    ]
    expected_somewhere = {"run:pc", "run:cycle", "run:after_live", "bit:mem_wr", "mem:keeps_lo", "next:branch", "next:plain"}
    seen = set()
    for edits in forgeries:
        m = m0.copy()
        for c, r, v in edits:
            m[COL[c], r] = v % P
        want = {nm: rws for nm, rws in gen_circuit.check_trace_rows(m, g, first_only=False) if not nm.startswith("sum:")}
        got = check_ref.check(blob, po2, code, m, g, montgomery=False)
        assert {names[t] for t in got} == set(want), edits
        for t, (count, first) in got.items():
            assert (count, first) == (len(want[names[t]]), want[names[t]][0]), (edits, names[t])
        assert want, edits
        seen |= set(want)
    assert expected_somewhere <= seen
    # the public inputs are read too
    bad = list(g)
    bad[9] = 0x5000
    assert "end:pc" in {names[t] for t in check_ref.check(blob, po2, code, m0, bad, montgomery=False)}
