"""The session balance on the host (r0h_session_balance_* with a host handle; needs no GPU) against the numpy restatement
(tests/session_balance_ref.py): tuple circuits whose producers and consumers sit in different segments (tests/session_balance_circuits.py),
the table's growth as seen from outside, tuples given from outside, the refusals, and the trace circuit's session sum on an honest run
of at least three segments and on the forgeries tests/test_trace_circuit.py proves by hand.  tests/test_gpu_session_balance.py runs the
same cases with a device handle beside the host one: the case functions here take the handles to feed."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT, circuit_path

sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_circuit  # noqa: E402
import trace_circuit as tc  # noqa: E402
from trace_corners import COL, R_INV, canonical  # noqa: E402

import logup_ref as ref  # noqa: E402
import session_balance_circuits as sc  # noqa: E402
import session_balance_ref as sr  # noqa: E402
import session_by_hand as sbh  # noqa: E402

P = ref.P
PO2 = r0.TRACE_MIN_PO2
IMAGE, JOURNAL = r0.SESSION_SOURCE_IMAGE, r0.SESSION_SOURCE_JOURNAL


class HostSide:
    """a host handle fed with the cases' segments ((source, po2, code words or None, DATA words, public inputs))"""

    def __init__(self, blob):
        self.sb = r0.SessionBalance(blob)

    def add(self, segment):
        self.sb.add(*segment)

    def close(self):
        self.sb.free()


def host_sides(blob):
    return [HostSide(blob)]


def agree(sides, want):
    """every handle reports `want`, whole and cut to the lowest entry, and says it in the sequencer's words"""
    for s in sides:
        assert s.sb.report() == want
        assert s.sb.report(capacity=1) == (want[:1], len(want))
        if want:
            source, row, fraction, net, members, values = want[0]
            assert s.sb.message() == "session fraction %d does not balance: net %d over %d tuples, first in source %d at row %d, class (%s); %d classes in all" % (
                fraction, net, members, source, row, ", ".join(str(v) for v in values), len(want))
        else:
            assert s.sb.message() is None


def run(make_sides, blob, segments, outside=()):
    """the session through every handle -> the reference's report"""
    sides = make_sides(blob)
    for seg in segments:
        for s in sides:
            s.add(seg)
    for source, numerators, values in outside:
        for s in sides:
            s.sb.add_tuples(source, numerators, values)
    want = sr.check(blob, segments, outside)
    agree(sides, want)
    for s in sides:
        s.close()
    return want


def bump(segments, k, column, row):
    """the session with one DATA word of segment k changed (by one)"""
    source, po2, code, data, glob = segments[k]
    data = data.copy()
    at = sc.slot(segments, k, column, row)
    data[at] = ref.enc((int(ref.dec(data[at])) + 1) % P)
    return segments[:k] + [(source, po2, code, data, glob)] + segments[k + 1:]


# ---- 1. balanced split sessions and the split sums
SPLITS = ([4], [8, 4], [4, 12, 8])


def case_split(make_sides, sizes):
    c, segments = sc.session("pairs", sizes, seed=len(sizes))
    assert sr.identities(c.words) == [(2, 4), (0, 0), (2, 8)]
    assert run(make_sides, c.words, segments) == []
    k = len(sizes) - 1
    row = next(r for r in range(1 << sizes[k]) if ref.dec(segments[k][3][sc.slot(segments, k, 4, r)]) == 1)   # a row that produces
    bad = bump(segments, k, 0, row)
    want = run(make_sides, c.words, bad)
    a0, a1 = (int(ref.dec(segments[k][3][sc.slot(segments, k, col, row)])) for col in (0, 1))
    assert len(want) == 2 and sorted(w[3] for w in want) == [1, P - 1] and all(w[4] == 1 for w in want)
    produced = next(w for w in want if w[3] == 1)
    assert produced == (k, row, 4, 1, 1, (1, (-(a0 + 1)) % P, (-a1) % P))
    assert next(w for w in want if w[3] == P - 1)[5] == (1, (-a0) % P, (-a1) % P) and next(w for w in want if w[3] == P - 1)[2] == 5
    assert run(make_sides, c.words, bad[::-1]) == want      # the order of the additions makes no difference, word for word


@pytest.mark.parametrize("sizes", SPLITS, ids=str)
def test_split_sessions_balance_and_one_altered_cell_names_its_segment(sizes):
    case_split(host_sides, sizes)


# ---- 2. growth: 512, then 1,024, then 2,048 tuples are passed
def case_growth(make_sides, paired, stats=None):
    """every tuple a class of its own (producers only), or every class paired in the end (the consumers come in later additions);
    `stats(side)` is looked at after every addition"""
    c, segments = sc.session("pairs", [9, 7, 9, 10], seed=5, fill=1.0, consumers=paired)
    if paired:   # the producers first, the same segments' consumers afterwards, as additions of their own
        def side_of(seg, numerator_column):
            data = seg[3].copy()
            data[sc.slot(segments, seg[0], numerator_column, 0):][:1 << seg[1]] = 0
            return (seg[0], seg[1], seg[2], data, seg[4])
        segments = [side_of(s, 5) for s in segments] + [side_of(s, 4) for s in segments]
    sides = make_sides(c.words)
    reports = []
    for i in range(len(segments)):
        for s in sides:
            s.add(segments[i])
        want = sr.check(c.words, segments[:i + 1])
        agree(sides, want)          # a report between additions ...
        reports.append(want)
        tuples = sum(int(np.count_nonzero(ref.dec(seg[3]).reshape(sc.N_DATA, -1)[4:6])) for seg in segments[:i + 1])
        for s in sides:
            assert s.sb.stats()[0] == tuples
            if stats:
                stats(s, tuples)
    assert [len(w) for w in reports[:4]] == [512, 640, 1152, 2176]
    assert reports[-1] == ([] if paired else sr.check(c.words, segments))   # ... changes nothing of what the end gives
    assert sides[0].sb.stats()[3] == 2176                                   # classes held
    for s in sides:
        s.close()


@pytest.mark.parametrize("paired", [False, True], ids=["own classes", "paired"])
def test_reports_between_additions(paired):
    case_growth(host_sides, paired)


# ---- 3. tuples from outside
def outside_of(blob, segments, source=7):
    """the segments' tuples as an outside list that cancels them: the same vectors, numerators negated"""
    vecs, nums = [], []
    for _, po2, code, data, glob in segments:
        v, num, _, _ = sr.segment_tuples(blob, po2, code, data, glob)
        vecs.append(v)
        nums.append((P - num) % P)
    return (source, np.concatenate(nums), np.concatenate(vecs))


def case_outside(make_sides):
    c, segments = sc.session("pairs", [8, 5], seed=2, consumers=False)            # producers alone: the consumers are given from outside
    source, nums, vecs = outside_of(c.words, segments)
    assert len(nums) == 216
    assert run(make_sides, c.words, segments, [(source, nums, vecs)]) == []
    # one producer taken away: its outside tuple stands alone, named by source, index and fraction 255
    v0, num0, rows0, _ = sr.segment_tuples(c.words, *segments[0][1:])
    gone = [(segments[0][0], 8, None, segments[0][3].copy(), segments[0][4]), segments[1]]
    gone[0][3][sc.slot(segments, 0, 4, int(rows0[3]))] = 0
    assert run(make_sides, c.words, gone, [(source, nums, vecs)]) == [(source, 3, 255, P - 1, 1, tuple(int(x) for x in vecs[3]))]
    # an outside tuple left out: the producer stands alone; one whose numerator is zero is no tuple, and the others keep their rows
    left = nums.copy()
    left[5] = 0
    want = run(make_sides, c.words, segments, [(source, left, vecs)])
    assert want == [(0, int(rows0[5]), 4, 1, 1, tuple(int(x) for x in vecs[5]))]
    # numerators a and p - a in one class
    a = np.asarray([1, 2, P - 1, (P - 1) // 2, 12345, P - 2] * 36, dtype=np.int64)
    weighted = [(s[0], s[1], s[2], s[3].copy(), s[4]) for s in segments]
    at = 0
    for k, seg in enumerate(weighted):
        rows = sr.segment_tuples(c.words, *segments[k][1:])[2]
        for r in rows:
            seg[3][sc.slot(segments, k, 4, int(r))] = ref.enc(a[at])
            at += 1
    assert run(make_sides, c.words, weighted, [(source, (P - a) % P, vecs)]) == []
    assert len(run(make_sides, c.words, weighted, [(source, (P - a + (np.arange(216) == 9)) % P, vecs)])) == 1
    # p - 1 on 5,000 members of ONE class against their count on one row: the sum passes 5,000 multiples of p
    many = [(segments[1][0], 5, None, segments[1][3].copy(), segments[1][4])]
    many[0][3][:] = 0
    for col, value in ((0, 9), (1, 4), (4, 5000)):
        many[0][3][sc.slot(many, 0, col, 17)] = ref.enc(value)
    vec = [1, P - 9, P - 4]
    assert run(make_sides, c.words, many, [(source, [P - 1] * 5000, [vec] * 5000)]) == []
    assert run(make_sides, c.words, many, [(source, [P - 1] * 4999, [vec] * 4999)]) == [(1, 17, 4, 1, 5000, tuple(vec))]
    # a part whose value is zero against a denominator without that part: one class
    z, zsegs = sc.session("zero part", [6, 9], seed=3)
    assert run(make_sides, z.words, zsegs) == []
    # ... and a coordinate scaled by an early public input's value
    e, esegs = sc.session("early", [5, 7], seed=4)
    assert run(make_sides, e.words, esegs) == []
    row = next(r for r in range(1 << 7) if ref.dec(esegs[1][3][sc.slot(esegs, 1, 4, r)]) == 1)
    assert len(run(make_sides, e.words, bump(esegs, 1, 1, row))) == 2


def test_tuples_from_outside():
    case_outside(host_sides)


# ---- 4. refusals
def case_refusals(make_sides):
    for kind, text in (("nine", "9 challenge identities"), ("late", "reads the value of late public input 5")):
        with pytest.raises(r0.R0HipError, match="r0h_session_balance_new: .*" + text):
            make_sides(sc.Circuit(kind).words)
    c, segments = sc.session("pairs", [4], seed=1)
    sides = make_sides(c.words)
    for s in sides:
        with pytest.raises(r0.R0HipError, match=r"r0h_session_balance_add_tuples: \d+ tuples in one call: more than 2\^24"):
            one, three = np.zeros(1, dtype=np.uint32), np.zeros(3, dtype=np.uint32)       # (the count is refused before a word is read)
            r0._check(r0.lib().r0h_session_balance_add_tuples(s.sb.handle, 0, one.ctypes.data_as(r0._vp), three.ctypes.data_as(r0._vp), (1 << 24) + 1))
        with pytest.raises(r0.R0HipError, match="numerator 0 is not canonical"):
            s.sb.add_tuples(0, [P], [[1, 2, 3]])
        with pytest.raises(r0.R0HipError, match="value 2 of tuple 1 is not canonical"):
            s.sb.add_tuples(0, [1, 1], [[1, 2, 3], [1, 2, 0xFFFFFFFF]])
        with pytest.raises(r0.R0HipError, match="not the trace circuit"):
            s.sb.add_verifier_side(b"\x7fELF", b"")
        for po2 in (3, 25):
            with pytest.raises(r0.R0HipError, match="po2 %d outside" % po2):
                s.add((0, po2) + segments[0][2:])
        bad_glob = segments[0][4].copy()
        bad_glob[2] = P
        with pytest.raises(r0.R0HipError, match=r"global\[2\] not canonical"):
            s.add(segments[0][:4] + (bad_glob,))
        late_garbage = segments[0][4].copy()
        late_garbage[4:] = 0xFFFFFFFF                      # late inputs do not exist yet: whatever stands there is not looked at
        s.add(segments[0][:4] + (late_garbage,))
    agree(sides, [])                                       # the handles go on working
    for s in sides:
        s.close()
    tiny = np.fromfile(circuit_path("tiny"), dtype=np.uint32)       # no public-total accumulators: nothing to check, 0 classes
    sides = make_sides(tiny)
    for s in sides:
        assert s.sb.identities == [] and s.sb.report() == [] and s.sb.stats()[0] == 0
        s.sb.add_tuples(0, [1], [])
        assert s.sb.report() == [] and s.sb.message() is None
        s.close()


def test_refusals():
    case_refusals(host_sides)
    c, segments = sc.session("pairs", [4], seed=1)
    sb = r0.SessionBalance(c.words)
    with pytest.raises(r0.R0HipError, match="r0h_session_balance_add: this handle was made without a context"):     # the wrong form for the handle's kind
        r0._check(r0.lib().r0h_session_balance_add(sb.handle, 0, sb.handle, 4, None, sb.handle, None))
    early = sc.session("early", [4], seed=1)
    sb2 = r0.SessionBalance(early[0].words)
    with pytest.raises(r0.R0HipError, match="a form reads a public input and none were given"):
        sb2.add(0, 4, None, early[1][0][3], None)


# ---- 5. / 6. the trace circuit: an honest run of at least three segments, and the forgeries
class TraceSession:
    """the guest of test_trace_circuit's session test, cut into at least three segments, each expanded at 2^16 rows"""

    def __init__(self):
        from bench_session import elf_of
        from test_rv32im import ADDI, _guest
        self.blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
        self.prog, self.base = _guest(160), 0x400
        self.elf = elf_of(self.prog, self.base)
        self.other_elf = elf_of(self.prog[:-4] + [ADDI(0, 0, 0)] + self.prog[-3:], self.base)      # one instruction the run never reached differs
        self.other_word = (self.base >> 2) + len(self.prog) - 4
        self.vm = self.machine()
        self.journal = bytes(self.vm.journal)
        self.code = ref.enc(np.asarray(tc.code_columns(1 << PO2), dtype=np.int64)).reshape(-1)
        self.segments = self.witnesses()
        assert len(self.segments) >= 3 and self.vm.segments()[-1].closing

    def machine(self):
        vm = r0.Vm()
        vm.load_elf(self.elf)
        vm.set_input([7, 0x01020304])
        assert vm.run(segment_po2=9, keep_trace=True, boundary_rows=True) == (0, 0)
        return vm

    def witnesses(self, edit=None):
        return [(k, size, self.code, data, glob) for k, (size, data, glob) in enumerate(sbh.witnesses(self.vm, edit=edit, po2=PO2))]

    def verifier_side(self, prog=None, journal=None):
        """what r0h_session_balance_add_verifier_side adds, as outside lists for the reference: numerator p - 1 per image / journal word"""
        def side(source, words, tag):
            return (source, [P - 1] * len(words), [[1, (-a) % P, (-(w & 0xFFFF)) % P, (-(w >> 16)) % P, (-tag) % P] for a, w in words])
        prog = self.prog if prog is None else prog
        journal = self.journal if journal is None else journal
        return [side(IMAGE, [((self.base >> 2) + i, w) for i, w in enumerate(prog)], tc.TAG_IMG),
                side(JOURNAL, [(r0.JOURNAL_BASE // 4 + i, w) for i, w in enumerate(struct.unpack("<%dI" % (len(journal) // 4), journal))], tc.TAG_JRN)]

    def boundary_alteration(self):
        """test_trace_circuit's case (iii): a word segment 1 only reads "is found" with another value than segment 0 left
        -> (edit for session_by_hand.witnesses, the word's address)"""
        b1 = self.vm.boundary(1)
        j = next(i for i, b in enumerate(b1) if b.prev_seg == 1 and b.addr < r0.REG_BASE and b.first_value == b.last_value)
        n1 = self.vm.segments()[1].user_cycles

        def alter(k, data, glob):
            if k != 1:
                return False
            n = 1 << PO2
            v = b1[j].first_value ^ 0x40
            for col, val in (("after_lo", v & 0xFFFF), ("zq", (v & 0xFFFF) >> 2), ("before_lo", v & 0xFFFF)):
                data[COL[col] * n + n1 + j] = ref.enc(val)
            for r, w in enumerate(self.vm.preflight(1)):
                if w.mem_kind and (w.mem_addr >> 2) == b1[j].addr:
                    for col in ("before_lo", "after_lo"):
                        data[COL[col] * n + r] = ref.enc(v & 0xFFFF)
            return True
        return alter, b1[j].addr


@pytest.fixture(scope="module")
def trace_session():
    return TraceSession()


def run_trace(make_sides, ts, segments, elf, journal, outside):
    """segments and the verifier's side through every handle (the library's own list of the ELF's and the journal's words) against the
    reference fed with the same words as outside lists"""
    sides = make_sides(ts.blob)
    for seg in segments:
        for s in sides:
            s.add(seg)
    for s in sides:
        s.sb.add_verifier_side(elf, journal)
    want = sr.check(ts.blob, segments, outside)
    agree(sides, want)
    for s in sides:
        s.close()
    return want


def case_trace_honest(make_sides, ts):
    assert sr.identities(ts.blob) == [(2, 20), (0, 0), (2, 24), (2, 28), (2, 32)]
    assert run_trace(make_sides, ts, ts.segments, ts.elf, ts.journal, ts.verifier_side()) == []
    # without the verifier's side every image word read and every journal word stands alone; with the image alone, the journal's
    sides = make_sides(ts.blob)
    for s in sides:
        for seg in ts.segments:
            s.add(seg)
        s.sb.add_verifier_side(ts.elf, None)
    want = sr.check(ts.blob, ts.segments, ts.verifier_side()[:1])
    assert len(want) == len(ts.journal) // 4 and all(w[2] == 39 and w[5][4] == P - tc.TAG_JRN for w in want)
    agree(sides, want)
    for s in sides:
        s.close()


def test_an_honest_trace_session_balances(trace_session):
    ts = trace_session
    case_trace_honest(host_sides, ts)
    # ... as trace_circuit.check_fractions sees it from segment 0, everything else given as session_extra: it finds nothing
    extra = []
    for _, po2, code, data, glob in ts.segments[1:]:
        v, num, _, _ = sr.segment_tuples(ts.blob, po2, code, data, glob)
        extra += [((-int(x[1])) % P, (-int(x[2])) % P, (-int(x[3])) % P, (-int(x[4])) % P, int(n)) for x, n in zip(v, num)]
    for _, nums, vecs in ts.verifier_side():
        extra += [((-x[1]) % P, (-x[2]) % P, (-x[3]) % P, (-x[4]) % P, n) for x, n in zip(vecs, nums)]
    _, po2, _, data, glob = ts.segments[0]
    m, g = canonical(data, po2).astype(np.int64), [int(x) * R_INV % P for x in glob]
    assert tc.check_fractions(m, g, session_extra=extra) == []
    assert tc.check_fractions(m, g, session_extra=extra[:-1]) != []      # (a journal word left out: it does look)


FORGERIES = ("boundary value", "another elf", "journal byte", "closing segment left out")


def case_trace_forgery(make_sides, ts, what):
    segments, elf, journal, outside, must = ts.segments, ts.elf, ts.journal, ts.verifier_side(), None
    if what == "boundary value":
        alter, addr = ts.boundary_alteration()
        segments = ts.witnesses(edit=alter)
        must = lambda w: w[5][1] == (-addr) % P                                         # noqa: E731  the altered address
    elif what == "another elf":
        elf, outside = ts.other_elf, ts.verifier_side(prog=ts.prog[:-4] + [0x13] + ts.prog[-3:])
        must = lambda w: w[5][1] == (-ts.other_word) % P and w[0] == IMAGE              # noqa: E731  the word that differs, from the image's side
    elif what == "journal byte":
        journal = bytes([ts.journal[0] ^ 1]) + ts.journal[1:]
        outside = ts.verifier_side(journal=journal)
        word = struct.unpack("<I", journal[:4])[0]
        must = lambda w: w[0] == JOURNAL and w[1] == 0 and w[5][2] == (-(word & 0xFFFF)) % P   # noqa: E731  the altered word
    elif what == "closing segment left out":
        segments = ts.segments[:-1]
        must = lambda w: w[2] == 37                                                     # noqa: E731  session:produce of what nobody took back
    want = run_trace(make_sides, ts, segments, elf, journal, outside)
    names = gen_circuit.fraction_names("trace", public_totals=True)
    print(what, len(want), [(s, r, names[f] if f < 255 else "outside", net, members, values) for s, r, f, net, members, values in want[:6]])
    assert want and any(must(w) for w in want)
    return want


@pytest.mark.parametrize("what", FORGERIES)
def test_a_forged_trace_session_is_named(trace_session, what):
    case_trace_forgery(host_sides, trace_session, what)


# ---- names, and 8. the command line's text
def test_fraction_names_go_on_through_the_public_total_fractions():
    assert gen_circuit.fraction_names("trace", public_totals=True)[36:] == ["session:consume", "session:produce", "session:image", "session:journal"]
    assert gen_circuit.fraction_names("trace", public_totals=True)[:36] == gen_circuit.fraction_names("trace")
    image = np.fromfile(circuit_path("image"), dtype=np.uint32)
    assert gen_circuit.fraction_names("image", public_totals=True) == ["fraction:%d" % f for f in range(4 * len(ref.parse(image)["accs"]))]
    assert gen_circuit.fraction_names("tiny", public_totals=True) == []
    with open(os.path.join(ROOT, "circuits", "trace.fractions.txt")) as f:      # what r0h_prove reads: the build writes all 40
        assert f.read().split("\n")[36:40] == ["session:consume", "session:produce", "session:image", "session:journal"]


def test_the_command_line_documents_the_switch():
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    out = subprocess.run([prove, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--check-session 1 [--fraction-names file.txt]" in out.stdout and "single-rank" in out.stdout
    out = subprocess.run([prove, circuit_path("tiny"), "--check-session"], capture_output=True, text=True)
    assert out.returncode == 1 and "--check-session needs a value" in out.stderr
    for name in ("r0h_session_balance_new", "r0h_session_balance_add", "r0h_session_balance_report", "r0h_ctx_set_check_session"):
        assert name in r0.EXPORTED_SYMBOLS
