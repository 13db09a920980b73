"""The single-cell forgery sweep of the trace circuit, its parts that need no GPU: what a witness claims (tests/trace_claims.py) is
what the executor ran; the plan (tests/trace_forgeries.py) reaches every instruction kind and every special row; the criterion --
an edit is caught, or the claim is what it was -- notices a hole planted into the checker; and a seeded sample of the plan's sites
is judged with tools/gen_circuit.check_trace_rows, one edit at a time (a numpy check of 2^16 rows takes about a second: the whole
plan, some 48,000 edits, is test_gpu_trace_forgeries.py's job on the device) -- and by trace_forgeries.local_judge, which looks at
the edited row and its neighbours alone, agrees with check_trace_rows on the sample and walks the whole plan here in seconds.

Single-cell edits find cells nothing constrains; they do not find a consistent lie told in several cells at once --
trace_corners.dead_lie and test_trace_circuit's kind-by-kind test keep that job."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_circuit  # noqa: E402
import trace_circuit as tc  # noqa: E402
import trace_claims as tcl  # noqa: E402
import trace_forgeries as tf  # noqa: E402
from trace_corners import COL, F, P  # noqa: E402


def session_extra(h):
    """the verifier's side of the one-segment session as check_trace_rows takes it: (address, low, high, tag, numerator)"""
    return [((-v[1]) % P, (-v[2]) % P, (-v[3]) % P, (-v[4]) % P, num) for num, v in h.verifier_side()]


def judge(h, work, col, row, new, ignore=lambda name: False):
    """names of what check_trace_rows (constraints, chain fractions, the session's fractions) says of `work` -- the honest witness,
    edited in place at one cell and restored -- with the multiplicities recounted; a value outside its table is 'lookup ...'"""
    old = work[COL[col], row]
    work[COL[col], row] = new
    try:
        try:
            tc.multiplicities(work, h.g)
        except ValueError as e:
            return [str(e).split(":")[0]]
        return [name for name, _ in gen_circuit.check_trace_rows(work, h.g, session_extra=session_extra(h)) if not ignore(name)]
    finally:
        work[COL[col], row] = old


def claim_changes(h, work, col, row, new):
    before = tcl.claims(work, h.n_rows, h.n_bounds, only=[row])
    old = work[COL[col], row]
    work[COL[col], row] = new
    after = tcl.claims(work, h.n_rows, h.n_bounds, only=[row])
    work[COL[col], row] = old
    return before != after


@pytest.mark.parametrize("prog", tf.ORDER)
def test_an_honest_witness_claims_what_the_executor_ran(prog):
    h = tf.honest(prog)
    got, want = tcl.claims(h.m, h.n_rows, h.n_bounds), tcl.executed(h.rows, h.bounds)
    assert got["blank"] == [] and sorted(got["rows"]) == list(range(h.n_rows)) and sorted(got["bounds"]) == list(range(h.n_rows, h.n_rows + h.n_bounds))
    for part in ("rows", "bounds"):
        assert got[part] == want[part], next((r, got[part][r], want[part][r]) for r in want[part] if got[part][r] != want[part][r])
    # ... and a claim is not blind: another value in a claimed cell is another claim, an auxiliary cell is none
    r = h.n_rows // 2
    assert claim_changes(h, h.m, "rs1_lo", r, 12345) and claim_changes(h, h.m, "rdA", r, (int(h.m[COL["rdA"], r]) + 1) % 4)
    assert claim_changes(h, h.m, "live", h.n_rows + h.n_bounds, 1) and claim_changes(h, h.m, "after_hi", h.n_rows + 1, 77)
    assert not claim_changes(h, h.m, "dl4", r, 9) and not claim_changes(h, h.m, "zinv", r, 9) and not claim_changes(h, h.m, "pc", tf.N - 1, 4)


def test_the_plan_reaches_every_kind_and_every_special_row():
    kinds = {}
    for prog in tf.ORDER:
        h = tf.honest(prog)
        sites = tf.site_rows(prog)
        rows = [r for r, _ in sites]
        assert rows == sorted(set(rows))
        assert {0, h.n_rows - 1, h.n_rows, h.n_rows + h.n_bounds // 2, h.n_rows + h.n_bounds - 1, h.n_rows + h.n_bounds, tf.N - 1} <= set(rows)
        assert h.n_rows < h.n_rows + h.n_bounds // 2 < h.n_rows + h.n_bounds - 1 < tf.N - 2
        for r, what in sites:
            if what.startswith("kind"):
                assert 0 < r < h.n_rows - 1
                kind = tf.kind_of(h.rows[r])
                rd = (int(h.rows[r, F["insn"]]) >> 7) & 31
                assert ("rd = x0" in what) == (kind[0] in tf.WRITES_RD and rd == 0)
                kinds.setdefault(kind, []).append((prog, rd))
    assert all(len(v) <= 2 and len({p for p, _ in v}) == 1 for v in kinds.values())       # each kind in one program: once, and once more with rd = x0
    seen = {k for k in kinds if k[0] != 0x73}
    # what test_what_an_instruction_computes_is_constrained_kind_by_kind requires of its own programs
    assert {0x37, 0x17, 0x6F, 0x67, 0x63, 0x03, 0x23, 0x13, 0x33} <= {k[0] for k in seen} and len(seen) >= 45, sorted(seen)
    assert {(0x33, f3, 1) for f3 in range(8)} <= seen and {(0x33, 0, 0x20), (0x33, 5, 0x20), (0x13, 5, 0x20), (0x13, 1, 0)} <= seen
    assert {(0x03, f3, 0) for f3 in (0, 1, 2, 4, 5)} | {(0x23, f3, 0) for f3 in range(3)} | {(0x63, f3, 0) for f3 in (0, 1, 4, 5, 6, 7)} <= seen
    # the ecalls: both transfers moving a word and falling through, CYCLES (HALT is every program's last live row: a site of its own)
    assert {(0x73, 0, 2 * fn + moves) for fn, moves in ((1, 0), (1, 1), (2, 0), (2, 1), (3, 0))} <= set(kinds)
    assert all(tf.kind_of(tf.honest(prog).rows[-1]) == (0x73, 0, 0) for prog in tf.ORDER)
    assert any(rd == 0 for v in kinds.values() for _, rd in v if len(v) == 2)
    # columns and values
    assert len(tf.COLUMNS) == 126 and sum(len(b) for b in tf.BLOCKS) == 126 and len(tf.BLOCKS) == 4 and tf.GLOBALS == list(range(8, 20))
    edits = tf.plan("memory")
    assert edits == tf.plan("memory") and all(new != old and 0 <= new < P for _, _, _, _, old, new in edits)
    by_cell = {}
    for col, row, _, kind, old, new in edits:
        by_cell.setdefault((col, row), {})[kind] = (old, new)
    assert len(by_cell) == 126 * len(tf.site_rows("memory"))
    for (col, row), v in by_cell.items():
        assert len({new for _, new in v.values()}) == len(v) and "random" in v
        if "+1" in v:
            assert v["+1"][1] == (v["+1"][0] + 1) % P
        if "outside" in v:
            assert v["outside"][1] == {True: 2, col in tf.DIGITS: 4, col in tf.BYTES: 256, col in tf.HALVES: 65536}[True]
    assert by_cell[("live", tf.N - 1)]["outside"] == (0, 2) and "outside" not in by_cell[("live", 0)]     # (there old + 1 is 2 already)


def test_the_criterion_catches_a_planted_hole(monkeypatch):
    """A checker that has lost the mem:* constraints and the sum:mem:* fractions lets a load change the word it read: `after_lo` on a
    load row is then silent AND claim-changing -- the verdict that fails the sweep.  The real circuit catches the same cell."""
    h = tf.honest("memory")
    row = next(r for r, w in enumerate(h.rows.tolist()) if (w[F["insn"]] & 0x7F) == 0x03 and (w[F["insn"]] >> 12) & 7 == 2 and r > 20)
    new = int(h.m[COL["after_lo"], row]) ^ 1
    work = h.m.copy()
    got = judge(h, work, "after_lo", row, new)
    assert "mem:keeps_lo" in got and any(x.startswith("sum:mem:") for x in got)
    assert claim_changes(h, work, "after_lo", row, new)
    assert tcl.verdict(bool(got), False, True) == "caught"
    gen_circuit.check_trace_rows(h.m, h.g)   # (fills the cache)
    b, cons = gen_circuit._TRACE_CACHE[0]
    monkeypatch.setattr(gen_circuit, "_TRACE_CACHE", [(b, [c for c in cons if not c[0].startswith("mem:")])])
    mem_sum = lambda name: name.startswith("sum:") and all(part.startswith("mem:") for part in name[4:].split("|"))  # noqa: E731
    holed = judge(h, work, "after_lo", row, new, ignore=mem_sum)
    assert holed == [], holed
    assert tcl.verdict(bool(holed), tcl.claims(h.m, h.n_rows, h.n_bounds, only=[row]), tcl.claims(_edited(h, "after_lo", row, new), h.n_rows, h.n_bounds, only=[row])) == "HOLE"
    assert np.array_equal(work, h.m)


def _edited(h, col, row, new):
    m = h.m.copy()
    m[COL[col], row] = new
    return m


def test_a_seeded_sample_of_the_plan_is_caught_or_claims_nothing_new():
    rng = np.random.default_rng(2026)
    judged, silent = 0, []
    for prog, count in (("mext", 5), ("alu", 5), ("memory", 5), ("control", 4), ("ecall", 5)):
        h = tf.honest(prog)
        work = h.m.copy()
        if prog == "ecall":   # the session's other side is the right one: the honest segment balances with its image and its journal
            assert len(h.journal) > 8 and gen_circuit.check_trace_rows(work, h.g, session_extra=session_extra(h)) == []
        edits = tf.plan(prog)
        for k in rng.choice(len(edits), count, replace=False):
            col, row, what, kind, old, new = edits[int(k)]
            got = judge(h, work, col, row, new)
            changes = claim_changes(h, work, col, row, new)
            terms, fractions = tf.local_judge(prog, [edits[int(k)]])[0]          # the row-local judge says the same
            if got[:1] and got[0].startswith("lookup "):
                assert got[0][len("lookup "):] in fractions
            else:
                assert terms == {name for name in got if not name.startswith("sum:")} and bool(fractions) == any(name.startswith("sum:") for name in got)
            print("forgery", prog, col, row, what, kind, old, "->", new, "caught by" if got else "silent", got[:4], "claim changes" if changes else "")
            assert got or not changes, ("a silent, claim-changing edit", prog, col, what, row, new)
            judged += 1
            if not got:
                silent.append((prog, col, row))
        for k, old, new in tf.global_plan(prog)[:1] if prog == "control" else ():      # a public input: always a claim of its own
            g = list(h.g)
            g[k] = new
            assert gen_circuit.check_trace_rows(h.m, g) != []
            judged += 1
    assert judged == 25 and len(silent) < judged // 2, silent


def test_the_whole_plan_judged_row_by_row():
    """every edit of the plan, all four values per cell, through trace_forgeries.local_judge: caught, or the claim is what it was"""
    edits_in_all, silent = 0, {}
    for prog in tf.ORDER:
        h = tf.honest(prog)
        edits = tf.plan(prog)
        for e, (terms, fractions) in zip(edits, tf.local_judge(prog, edits)):
            if not (terms or fractions):
                silent[e[0]] = silent.get(e[0], 0) + 1
                assert not claim_changes(h, h.m, e[0], e[1], e[5]), ("a silent, claim-changing edit", prog) + e
        edits_in_all += len(edits)
    print("row-local sweep:", edits_in_all, "edits,", sum(silent.values()), "silent;", silent)
    assert edits_in_all > 40000 and 0 < sum(silent.values()) * 10 < edits_in_all
