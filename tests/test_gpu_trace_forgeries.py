"""The single-cell forgery sweep of the trace circuit on the device: every cell of the plan (tests/trace_forgeries.py -- five corner
programs, one live row per instruction kind, the first and last live row, three boundary rows, a blank row and row N - 1; all 126
DATA columns a forger does not recount, and the public inputs 8..19) is edited ONE AT A TIME in the device witness, the
multiplicities are recounted (r0h_logup_multiplicities), and r0h_check_witness (early terms), r0h_logup_check_balance and -- on
boundary rows, COMMIT rows and for the session's own flags -- the session balance of the one-segment closing session judge it.

  a. soundness at one cell: every edit is caught, or the witness claims what it claimed before (tests/trace_claims.py);
  b. the device's tables are the references' (check_ref.check term for term, balance_ref and session_balance_ref class for class) on
     batched witnesses that carry hundreds of plan edits each and an edited cell in each of the 40 ACCUM columns;
  c. over the whole sweep every one of the 302 terms and the 40 fractions is reported, but for the literal table UNREACHABLE.

One verdict per edit: several edits in one witness can cancel in a tuple class and pass for silent.  Single-cell edits find cells
nothing constrains; they do not find a consistent lie told in several cells at once -- trace_corners.dead_lie and
test_trace_circuit's kind-by-kind test keep that job.  Timings and the table of silent cells: profiles/r26/trace_forgeries.md."""
import json
import os
import sys
import time

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import __graft_entry__ as entry
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import balance_ref  # noqa: E402
import check_ref  # noqa: E402
import gen_circuit  # noqa: E402
import session_balance_ref as sr  # noqa: E402
import trace_claims as tcl  # noqa: E402
import trace_forgeries as tf  # noqa: E402
from trace_corners import COL, P  # noqa: E402

pytestmark = pytest.mark.gpu
PO2, N = tf.PO2, tf.N
R = (1 << 32) % P
TERMS = gen_circuit.term_names("trace")
FRACTIONS = gen_circuit.fraction_names("trace", public_totals=True)
# the values swept per cell, in tf.VALUE_KINDS' order of preference: what keeps a case (a program's block of 32 columns) within a few
# seconds -- the time of an edit grows with the program's live rows (profiles/r26/trace_forgeries.md)
SWEPT = {"mext": ("+1",), "alu": ("+1", "outside"), "memory": tf.VALUE_KINDS, "control": tf.VALUE_KINDS, "ecall": tf.VALUE_KINDS}
# the cells the session's fractions read: there the session balance is consulted whatever the other checkers say
SESSION_COLUMNS = {"bnd", "cact", "fimg", "addr3", "after_lo", "after_hi", "before_lo", "before_hi", "old_lo", "old_hi", "dl2"}
# (column, what the row is) of every silent, claim-changing cell the sweep is known to find: none
KNOWN_OPEN = []
# the terms no single edit of an honest witness of these programs can make non-zero, and why
UNREACHABLE = {
    "exit:full_kind": "gated by last * live and G_TERM (1 + f2 - G_KIND): row N - 1 is blank, so live = 1 there meets f2 = 0 and G_KIND = 1 -- it takes a second cell",
    "exit:full_none": "gated by last * live and (1 - G_TERM) G_KIND: the programs end in HALT, G_TERM = 1 -- it takes live at row N - 1 AND a public input",
}
assert len(UNREACHABLE) <= 13 and len(TERMS) == 302 and len(FRACTIONS) == 40
DENSITY, VACUOUS = 2, 3    # at least half the values a cell can have are distinct; fewer than a third of a case's edits may be silent


def word(v):
    return np.array([int(v) * R % P], dtype=np.uint32)


@pytest.fixture(scope="module")
def trace(hal):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    gc.load_check(entry.check_code_object_path("trace"))
    code, unused, _ = hal.witgen(gc, PO2, 0)
    unused.free()
    state = dict(blob=blob, gc=gc, code=code, code_words=code.to_host(), programs={}, swept={}, batches={})
    yield state
    for p in state["programs"].values():
        p.data.free()
    code.free()
    gc.free()


class Program:
    """a corner program's honest witness on the device, and the checkers' verdicts on it"""

    def __init__(self, hal, trace, prog):
        self.hal, self.t, self.h = hal, trace, tf.honest(prog)
        h, gc = self.h, trace["gc"]
        self.data, glob = hal.trace_witgen(h.rows, h.bounds, PO2, circuit=gc)
        assert np.array_equal(self.data.to_host(), h.data) and np.array_equal(glob, h.glob)    # the plan's old values are the device's
        self.glob = glob.copy()
        self.glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = np.random.default_rng(26).integers(0, P, 16).astype(np.uint32)
        side = h.verifier_side()
        self.outside = (r0.SESSION_SOURCE_IMAGE, [num for num, _ in side], [v for _, v in side])
        self.work = h.m.copy()
        self.cact = set(int(r) for r in np.nonzero(h.m[COL["cact"]])[0])
        self.clock = {}
        assert self.judge() == ([], [], [])

    def timed(self, what, fn, *args, **kw):
        t0 = time.perf_counter()
        try:
            return fn(*args, **kw)
        finally:
            self.clock[what] = self.clock.get(what, 0.0) + time.perf_counter() - t0

    def chain(self):
        """the chain's unbalanced classes: the lowest 64 in one call, all of them in another where there are more"""
        args = (self.t["gc"], PO2, self.t["code"], self.data, self.glob)
        found, n = self.hal.logup_check_balance(*args, capacity=64)
        return found if n <= 64 else self.hal.logup_check_balance(*args)

    def session(self, glob=None):
        sb = r0.SessionBalance(self.t["blob"], self.hal)
        try:
            sb.add(0, PO2, self.t["code"], self.data, self.glob if glob is None else glob, circuit=self.t["gc"])
            sb.add_tuples(*self.outside)
            return sb.report()
        finally:
            sb.free()

    def judge(self, glob=None, session=True):
        glob = self.glob if glob is None else glob
        return (self.hal.check_witness(self.t["gc"], PO2, self.t["code"], self.data, glob),
                self.hal.logup_check_balance(self.t["gc"], PO2, self.t["code"], self.data, glob), self.session(glob) if session else [])

    def recount(self):
        self.hal.logup_multiplicities(self.t["gc"], PO2, self.data, self.glob)

    def edit(self, col, row, what, kind, old, new):
        """one cell edited, judged, restored -> what the checkers said"""
        at = COL[col] * N + row
        self.timed("upload", self.data.upload, word(new), at)
        lookup = False
        try:
            self.timed("recount", self.recount)
        except r0.R0HipError as e:
            assert "looks up a value that is not in its table" in str(e)
            lookup = True
        early = self.timed("check_witness", self.hal.check_witness, self.t["gc"], PO2, self.t["code"], self.data, self.glob)
        chain = self.timed("check_balance", self.chain)
        # the session's sum: on boundary rows, COMMIT rows and for its own flags, where its fractions read the cell or nobody else objected
        ask = (self.h.n_rows <= row < self.h.n_rows + self.h.n_bounds or row in self.cact or col in ("bnd", "cact", "fimg")) and (
            col in SESSION_COLUMNS or not (lookup or early or chain))
        sess = self.timed("session_balance", self.session) if ask else []
        self.timed("upload", self.data.upload, word(old), at)
        if lookup:   # the refusal leaves the context as it was: the honest witness, recounted, is clean
            self.timed("after a refusal", self.recount)
            assert self.timed("after a refusal", self.hal.check_witness, self.t["gc"], PO2, self.t["code"], self.data, self.glob) == []
        out = dict(col=col, row=row, what=what, kind=kind, new=new, lookup=lookup, session=ask, terms={t for t, _, _ in early},
                   fractions={f for f, _, _, _ in chain} | {f for _, _, f, _, _, _ in sess if f < sr.OUTSIDE})
        out["caught"] = bool(lookup or early or chain or sess)
        if not out["caught"]:
            before = tcl.claims(self.work, self.h.n_rows, self.h.n_bounds, only=[row])
            self.work[COL[col], row] = new
            out["hole"] = tcl.verdict(False, before, tcl.claims(self.work, self.h.n_rows, self.h.n_bounds, only=[row])) == "HOLE"
            self.work[COL[col], row] = old
        return out


def program(hal, trace, prog):
    if prog not in trace["programs"]:
        trace["programs"][prog] = Program(hal, trace, prog)
    return trace["programs"][prog]


def swept(hal, trace, prog, block):
    """the verdicts on the program's edits of the block's columns (block 0: the public inputs as well), judged once a module"""
    if (prog, block) not in trace["swept"]:
        p = program(hal, trace, prog)
        t0, p.clock = time.perf_counter(), {}
        edits = [p.edit(*e) for e in tf.plan(prog, tf.BLOCKS[block], SWEPT[prog])]
        seconds = time.perf_counter() - t0
        publics = []
        for k, old, new in tf.global_plan(prog) if block == 0 else ():
            glob = p.glob.copy()
            glob[k] = word(new)[0]
            early, chain, sess = p.judge(glob)
            publics.append(dict(k=k, caught=bool(early or chain or sess), terms={t for t, _, _ in early},
                                fractions={f for f, _, _, _ in chain} | {f for _, _, f, _, _, _ in sess if f < sr.OUTSIDE}))
        p.recount()
        assert p.judge() == ([], [], []) and np.array_equal(p.data.to_host(), p.h.data)      # everything was put back
        trace["swept"][(prog, block)] = (edits, publics, seconds, {k: round(v, 3) for k, v in p.clock.items()})
    return trace["swept"][(prog, block)]


# ---- a. soundness at one cell
@pytest.mark.parametrize("block", range(len(tf.BLOCKS)))
@pytest.mark.parametrize("prog", tf.ORDER)
def test_every_single_cell_edit_is_caught_or_claims_nothing_new(hal, trace, prog, block):
    edits, publics, seconds, clock = swept(hal, trace, prog, block)
    silent = {}
    for e in edits:
        if not e["caught"]:
            silent[e["col"]] = silent.get(e["col"], 0) + 1
    print("sweep " + json.dumps(dict(prog=prog, block=block, values=" ".join(SWEPT[prog]), columns=tf.BLOCKS[block][0] + ".." + tf.BLOCKS[block][-1], edits=len(edits), publics=len(publics),
                                     seconds=round(seconds, 3), ms_per_edit=round(1e3 * seconds / len(edits), 3), refused_by_the_recount=sum(e["lookup"] for e in edits),
                                     session_consulted=sum(e["session"] for e in edits), seconds_in=clock, silent=silent)))
    assert len(edits) >= len(tf.site_rows(prog)) * len(tf.BLOCKS[block]) * len(SWEPT[prog]) // DENSITY and len(publics) == (12 if block == 0 else 0)
    holes = [(e["col"], e["what"], e["row"], e["new"]) for e in edits if e.get("hole")]
    assert {(c, w) for c, w, _, _ in holes} <= set(KNOWN_OPEN), "silent, claim-changing edits (column, kind, row, value): %s" % holes[:20]
    assert all(q["caught"] for q in publics), [q["k"] for q in publics if not q["caught"]]    # a public input is a claim of its own
    # the device's verdict on every edit is the row-local reference's: the same terms by name, caught or not
    for e, (terms, fractions) in zip(edits, tf.local_judge(prog, tf.plan(prog, tf.BLOCKS[block], SWEPT[prog]))):
        assert {TERMS[t] for t in e["terms"]} == terms and e["caught"] == bool(terms or fractions), (e["col"], e["what"], e["row"], e["new"], sorted(terms), sorted(fractions))
    assert sum(not e["caught"] for e in edits) * VACUOUS < len(edits)                              # (not vacuous: most cells are constrained)


# ---- b. the device's tables are the references'
N_BATCHES, BATCH_EDITS = 3, 300


def fired(results):
    return set().union(*[e["terms"] for e in results]), set().union(*[e["fractions"] for e in results])


def compare(p, accum_edits=False):
    """the device's three tables on the witness as it stands against the references' -> (terms, fractions) reported"""
    hal, t = p.hal, p.t
    gc, code = t["gc"], t["code"]
    full = hal.logup_totals(gc, PO2, code, p.data, p.glob)
    mix = np.random.default_rng(5).integers(0, P, gc.n_mix).astype(np.uint32)
    accum = hal.accum_public(gc, PO2, code, p.data, full, mix)
    try:
        if accum_edits:   # one cell of each ACCUM column, on rows of their own: every accum:* term sees one
            assert gc.group_size[check_ref.G_ACCUM] == 40
            for k in range(40):
                at = k * N + 1000 + 17 * k
                accum.upload(np.array([(int(accum.to_host(at, 1)[0]) + 1) % P], dtype=np.uint32), at)
        words = p.data.to_host()
        want = check_ref.check(t["blob"], PO2, t["code_words"], words, full, accum.to_host(), mix)
        got = {term: (rows, first) for term, rows, first in hal.check_witness(gc, PO2, code, p.data, full, accum, mix)}
        assert got == want, sorted(set(got.items()) ^ set(want.items()))[:8]
        early = {term: (rows, first) for term, rows, first in hal.check_witness(gc, PO2, code, p.data, full)}
        late = check_ref.Program(t["blob"]).late
        assert early == {term: v for term, v in want.items() if not late[term]}
    finally:
        accum.free()
    chain = balance_ref.check(t["blob"], PO2, t["code_words"], words, p.glob)
    assert hal.logup_check_balance(gc, PO2, code, p.data, p.glob) == chain
    sess = sr.check(t["blob"], [(0, PO2, t["code_words"], words, p.glob)], [p.outside])
    assert p.session() == sess
    return set(want), {f for f, _, _, _ in chain} | {f for _, _, f, _, _, _ in sess if f < sr.OUTSIDE}


def batch_plan(results, which):
    """batch `which` of a program's judged edits: for every term and fraction some edit fired, two of the edits that did (dealt out
    over the batches), filled up with every k-th edit of the plan; one edit per cell"""
    cells = {}
    cover = {}
    for i, e in enumerate(results):
        for key in [("t", t) for t in e["terms"]] + [("f", f) for f in e["fractions"]]:
            if len(cover.setdefault(key, [])) < 2:
                cover[key].append(i)
    dealt = sorted({i for v in cover.values() for i in v})
    for j, i in enumerate(dealt):
        if j % N_BATCHES == which:
            cells.setdefault((results[i]["col"], results[i]["row"]), results[i])
    stride = max(1, len(results) // BATCH_EDITS)
    for e in results[which::stride]:
        cells.setdefault((e["col"], e["row"]), e)
    return list(cells.values())


def batch(hal, trace, prog, which):
    """-> (terms, fractions) the batch's comparison reported, compared once a module"""
    if (prog, which) not in trace["batches"]:
        p = program(hal, trace, prog)
        results = [e for block in range(len(tf.BLOCKS)) for e in swept(hal, trace, prog, block)[0]]
        if which == "rest":   # what fired in (a) and in none of the batches: those edits alone, as they were judged
            have = [batch(hal, trace, prog, k) for k in range(N_BATCHES)]
            terms, fractions = set().union(*[h[0] for h in have]), set().union(*[h[1] for h in have])
            todo = [e for e in results if e["terms"] - terms or e["fractions"] - fractions]
            singles = []
            while todo and len(singles) < 6:
                e = todo[0]
                singles.append(e)
                terms, fractions = terms | e["terms"], fractions | e["fractions"]
                todo = [x for x in todo if x["terms"] - terms or x["fractions"] - fractions]
            assert not todo, "more than six edits fire what no batch contains: %s" % [(x["col"], x["row"], x["new"]) for x in todo[:8]]
            plans = [[e] for e in singles]
        else:
            plans = [batch_plan(results, which)]
            assert len(plans[0]) >= min(BATCH_EDITS, len(results) // 2) // 2
        got_terms, got_fractions = set(), set()
        for edits in plans:
            for e in edits:
                p.data.upload(word(e["new"]), COL[e["col"]] * N + e["row"])
            if which != N_BATCHES - 1:
                try:
                    p.recount()
                except r0.R0HipError:
                    pass   # (several edits of one row together may leave a table: counted or not, both sides read the same words)
            else:         # the last batch keeps the honest counts, and two table rows nobody looks up are counted once
                for col, row in (("m16", 40000), ("mand", 40000)):
                    assert p.h.m[COL[col], row] == 0
                    p.data.upload(word(1), COL[col] * N + row)
            terms, fractions = compare(p, accum_edits=which == N_BATCHES - 1)
            got_terms, got_fractions = got_terms | terms, got_fractions | fractions
            p.data.upload(p.h.data)
        assert p.judge() == ([], [], [])
        trace["batches"][(prog, which)] = (got_terms, got_fractions, [len(x) for x in plans])
    return trace["batches"][(prog, which)]


@pytest.mark.parametrize("which", list(range(N_BATCHES)) + ["rest"])
@pytest.mark.parametrize("prog", tf.ORDER)
def test_batched_edits_give_the_references_tables(hal, trace, prog, which):
    terms, fractions, sizes = batch(hal, trace, prog, which)
    print("batch", prog, which, "edits", sizes, "terms", len(terms), "fractions", len(fractions))
    if which == N_BATCHES - 1:
        assert {TERMS[t] for t in terms} >= {n for n in TERMS if n.startswith("accum:")} and {"table:r16", "table:and"} <= {FRACTIONS[f] for f in fractions}
    if which == "rest":   # together the batches contain whatever fired anywhere in (a)
        have = [batch(hal, trace, prog, k) for k in list(range(N_BATCHES)) + ["rest"]]
        want = fired([e for block in range(len(tf.BLOCKS)) for e in swept(hal, trace, prog, block)[0]])
        got = set().union(*[h[0] for h in have]), set().union(*[h[1] for h in have])
        assert want[0] <= got[0] and want[1] <= got[1], ([TERMS[t] for t in want[0] - got[0]], [FRACTIONS[f] for f in want[1] - got[1]])


# ---- c. coverage
def test_every_term_and_every_fraction_is_reported_somewhere_in_the_sweep(hal, trace):
    terms, fractions, edits, silent, lookups, seconds, holes = set(), set(), 0, {}, 0, 0.0, set()
    for prog in tf.ORDER:
        for block in range(len(tf.BLOCKS)):
            results, publics, s, _ = swept(hal, trace, prog, block)
            t, f = fired(results + publics)
            terms, fractions, edits, seconds = terms | t, fractions | f, edits + len(results) + len(publics), seconds + s
            lookups += sum(e["lookup"] for e in results)
            holes |= {(e["col"], e["what"]) for e in results if e.get("hole")}
            for e in results:
                if not e["caught"]:
                    silent.setdefault(e["col"], set()).add((prog, e["row"]))
        for which in list(range(N_BATCHES)) + ["rest"]:
            t, f, _ = batch(hal, trace, prog, which)
            terms, fractions = terms | t, fractions | f
    unfired = [n for k, n in enumerate(TERMS) if k not in terms]
    print("coverage " + json.dumps(dict(edits=edits, seconds=round(seconds, 2), refused_by_the_recount=lookups, silent_edits_cells={c: len(v) for c, v in sorted(silent.items())},
                                        terms=len(terms), fractions=len(fractions), unfired=unfired, fractions_unfired=[n for k, n in enumerate(FRACTIONS) if k not in fractions])))
    assert holes == set(KNOWN_OPEN)     # the table is exact: a cell that has been closed leaves it
    assert sorted(unfired) == sorted(UNREACHABLE), "unfired terms against the table: %s" % sorted(set(unfired) ^ set(UNREACHABLE))
    assert fractions == set(range(len(FRACTIONS))), [n for k, n in enumerate(FRACTIONS) if k not in fractions]
