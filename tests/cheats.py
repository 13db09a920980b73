"""A cheating prover for the verifiers' algebra (oracle/orc.h orc_prove_segment_cheat, through orc_binding's prove(cheat=)): seals whose
transcript and Merkle trees are valid and whose algebra tells ONE lie, so that no check but the one that binds the lied-about words
can refuse them.  This helper lists the cheats of a circuit and says which verdicts each kind may get; no run of a verifier went
into that.

A cheat is (kind, a, b, delta); the lie is delta added in the field to every word it covers.  The tests use word + 1 mod p (DELTA).

The verdicts follow from the order of the verifier's checks (csrc/verify.cpp, oracle/orc_prove.c: the transcript and the tree tops, 4 the
constraint identity at z, then per query 3 the group openings, 6 the DEEP value against the first round's member -- and every fold
against the next round's member --, 5 a round's opening, 7 the last fold against the final polynomial):
  committed  a column of CODE, DATA, ACCUM or CHECK lies in every row of the committed evaluations, nothing else does.  coeff_u is
             honest: the identity holds.  The paths are valid.  The column has a register, so the DEEP value of every query is off by
             delta times the register's weight over a non-zero denominator, and FRI's first matrix is honest: 6, at query 0.
  flowing    the same lie also feeds eval_check: CHECK's openings are those of (constraints over the lying columns) / vanishing, while
             coeff_u holds the honest columns at z -- the identity compares the two: 4.
  coeff_u    a word of CHECK's sixteen openings, or of a register's interpolant that moves a term of the constraint program, changes
             a side of the identity: 4.  A word that moves no term gets past it; the prover's quotient dropped a non-zero remainder,
             so the DEEP value is off by remainder / denominator: 6.  Coefficient k of an interpolant moves the tap at z w^-back by
             delta (z w^-back)^k: a word of the constant coefficient moves every tap of its register alike, which a term that reads
             the register through differences of its taps alone (a running sum: a(0) - a(1) - ...) does not see -- a column shifted by
             a constant is as good a witness, and only the DEEP comparison holds the opened interpolant to the committed column.
             `coeff_u_verdict` says 4 or 6 for every word, from the constraint program's text.
  fri        column 16 k + i of a round's matrix is component k of coset member i.  Query 0 opens that row: where its position picks
             member i the goal comparison of that round fails, 6; otherwise the fold of the sixteen members is off and the next
             comparison fails -- the next round's member, 6, or after the last round the final polynomial, 7.
  final      the final polynomial is off by delta X^i, which no power of the final domain's generator annuls: 7, at query 0.
Never 0.  Never 1, 2, 3, 5, 8 or 9: the transcript or a Merkle path would have caught the lie, and the cheat was not the one intended.
With the control root given, a lie about a CODE column is a CODE commitment that is not the program's: 10, before any algebra."""
import numpy as np

import check_ref
import tap_circuits as tc
from conftest import circuit_path
from verify_mutations import regions

DELTA = 1  # word + 1 mod p
GROUP_NAMES = ("accum", "code", "data", "check")  # a = 0 .. 3 of the column kinds (orc.h ORC_GROUP_*)
CHECK, CHECK_SIZE, FRI_COLUMNS = 3, 16, 64
KINDS = ("committed", "flowing", "coeff_u", "fri", "final")
ALLOWED = {"committed": {6}, "flowing": {4}, "coeff_u": {4, 6}, "fri": {6, 7}, "final": {7}}
REASON = {4: "constraint check mismatch at z", 6: "fri fold goal mismatch", 7: "fri final polynomial mismatch",
          10: "code root is not the expected control root"}
CODE_ROOT = 10


def group_sizes(blob):
    return list(check_ref.Program(blob).group_size) + [CHECK_SIZE]


def unregistered(blob):
    """[(group, column)] of the columns no register covers: nothing of the DEEP comparison binds such a column"""
    have = {(g, col) for g, col, _ in check_ref.Program(blob).taps}
    return [(g, col) for g, size in enumerate(group_sizes(blob)[:3]) for col in range(size) if (g, col) not in have]


def _read_taps(pr):
    """the taps that the terms of the constraint program reach"""
    seen, stack = set(), [v for value, gates in pr.terms for v in [value] + gates]
    while stack:
        v = stack.pop()
        if v in seen:
            continue
        seen.add(v)
        op, a, b, _ = pr.fp[v]
        if op in (check_ref.OP_ADD, check_ref.OP_SUB, check_ref.OP_MUL):
            stack += [a, b]
    return {pr.fp[v][1] for v in seen if pr.fp[v][0] == check_ref.OP_GET}


def _moved_by_a_shift(pr):
    """the (group, column)s whose register, all its taps shifted by one constant, moves a term.  Per variable of the program, the
    derivative along that shift for every register it depends on: a field constant where the text shows one (taps 1, sums and
    differences, products with a constant), None where it does not (a product of two things that move, or of one with something
    else: taken as moving).  A difference of two taps of one register has derivative 0, and so has its product with anything."""
    p, d = check_ref.P, []
    for op, a, b, _ in pr.fp:
        if op == check_ref.OP_GET:
            d.append({pr.taps[a][:2]: 1})
        elif op in (check_ref.OP_ADD, check_ref.OP_SUB):
            sign, out = 1 if op == check_ref.OP_ADD else -1, {}
            for reg in set(d[a]) | set(d[b]):
                x, y = d[a].get(reg, 0), d[b].get(reg, 0)
                out[reg] = None if x is None or y is None else (x + sign * y) % p
            d.append({reg: v for reg, v in out.items() if v != 0})
        elif op == check_ref.OP_MUL:
            const = [pr.fp[v][1] % p for v in (a, b) if pr.fp[v][0] == check_ref.OP_CONST]
            other = d[b] if pr.fp[a][0] == check_ref.OP_CONST else d[a]
            if const:
                d.append({reg: None if v is None else v * const[0] % p for reg, v in other.items() if const[0]})
            else:
                d.append({reg: None for reg in set(d[a]) | set(d[b])})
        else:
            d.append({})
    return {reg for value, gates in pr.terms for v in [value] + gates for reg in d[v]}


def coeff_u_verdict(blob):
    """word of coeff_u -> 4 or 6.  coeff_u holds, register by register in tap order, the coefficients of the interpolant through the
    register's taps at z (four words each), then CHECK's sixteen values."""
    pr = check_ref.Program(blob)
    read, moved, verdict = _read_taps(pr), _moved_by_a_shift(pr), []
    for g, col, first, words in register_words(blob):
        is_read = any(t in read for t in range(first // 4, (first + words) // 4))
        verdict += [4 if is_read and (g, col) in moved else 6] * 4 + [4 if is_read else 6] * (words - 4)
    return verdict + [4] * (4 * CHECK_SIZE)


def register_words(blob):
    """[(group, column, first word of coeff_u, words)] per register, in tap order"""
    taps, out, t = check_ref.Program(blob).taps, [], 0
    while t < len(taps):
        size = 1
        while t + size < len(taps) and taps[t + size][:2] == taps[t][:2]:
            size += 1
        out.append((taps[t][0], taps[t][1], 4 * t, 4 * size))
        t += size
    return out


def late_accum_word(blob):
    """the first coeff_u word of an ACCUM register that some term reads together with a late public input (one that enters the
    transcript after the DATA commitment)"""
    from sha_suite_ref import parse_blob
    pr, c = check_ref.Program(blob), parse_blob(blob)
    first_late = c["n_global"] - c["n_late"]
    assert c["n_late"], "the circuit has no late public inputs"
    first_word = {(g, col): w for g, col, w, _ in register_words(blob)}
    for value, gates in pr.terms:
        seen, stack, accum, late = set(), [value] + gates, [], False
        while stack:
            v = stack.pop()
            if v in seen:
                continue
            seen.add(v)
            op, a, b, _ = pr.fp[v]
            if op in (check_ref.OP_ADD, check_ref.OP_SUB, check_ref.OP_MUL):
                stack += [a, b]
            elif op == check_ref.OP_GET and pr.taps[a][0] == check_ref.G_ACCUM:
                accum.append(pr.taps[a][:2])
            elif op == check_ref.OP_GET_GLOBAL and a == 0 and b >= first_late:
                late = True
        if late and accum:
            return first_word[min(accum)]
    raise AssertionError("no term reads an ACCUM tap together with a late public input")


def cheats(blob, po2, kind):
    """[(label, (kind, a, b, DELTA))]: the whole sweep of one kind over a proof of 2^po2 rows"""
    sizes = group_sizes(blob)
    if kind == "committed":
        return [("%s column %d, committed" % (GROUP_NAMES[g], col), (kind, g, col, DELTA)) for g in (1, 2, 0, 3) for col in range(sizes[g])]
    if kind == "flowing":
        return [("%s column %d, flowing" % (GROUP_NAMES[g], col), (kind, g, col, DELTA)) for g in (1, 2, 0) for col in range(sizes[g])]
    if kind == "coeff_u":
        return [("coeff_u word %d" % w, (kind, w, 0, DELTA)) for w in range(4 * (len(check_ref.Program(blob).taps) + CHECK_SIZE))]
    r = _layout(blob, po2)
    if kind == "fri":
        return [("fri round %d column %d" % (rd, col), (kind, rd, col, DELTA)) for rd in range(len(r["fri"])) for col in range(FRI_COLUMNS)]
    assert kind == "final"
    return [("final word %d" % w, (kind, w, 0, DELTA)) for w in range(r["final"][1] - r["final"][0])]


def sample_two_rounds(blob, po2=13):
    """what is swept where a proof costs a quarter of a second: in each FRI round one column per coset member, the component rotating
    (16 columns), and four committed columns -- the first of each group"""
    assert len(_layout(blob, po2)["fri"]) == 2
    out = [("fri round %d column %d" % (rd, 16 * (i % 4) + i), ("fri", rd, 16 * (i % 4) + i, DELTA)) for rd in (0, 1) for i in range(16)]
    return out + [("%s column 0, committed" % GROUP_NAMES[g], ("committed", g, 0, DELTA)) for g in (1, 2, 0, 3)]


def trace_handful(blob):
    """[(label, cheat, verdict)] for a circuit whose proofs take seconds each: the last column of every group, committed, and four
    words of coeff_u -- of an ACCUM register read together with a late public input, its constant coefficient (a running sum: the
    identity does not see the shift) and its linear one (it does), of a register no term reads (if there is one) and the last word
    of CHECK's openings"""
    sizes, verdict, late = group_sizes(blob), coeff_u_verdict(blob), late_accum_word(blob)
    read = _read_taps(check_ref.Program(blob))
    out = [("%s column %d, committed" % (GROUP_NAMES[g], sizes[g] - 1), ("committed", g, sizes[g] - 1, DELTA), 6) for g in (1, 2, 0, 3)]
    unread = [first + 3 for _, _, first, words in register_words(blob) if not any(t in read for t in range(first // 4, (first + words) // 4))]
    words = [late, late + 4] + unread[-1:] + [len(verdict) - 1]
    return out + [("coeff_u word %d" % w, ("coeff_u", w, 0, DELTA), verdict[w]) for w in words]


def _layout(blob, po2):
    import verify_mutations
    from sha_suite_ref import parse_blob
    return verify_mutations._regions(parse_blob(blob), po2)


class Subject:
    """a circuit with one honest witness at one size: `prove(cheat)` is the oracle's seal of it, honest (None, kept) or cheating"""

    def __init__(self, orc, name, po2):
        self.name, self.po2 = name, po2
        if name == "trace":  # a corner program's run, its late public inputs filled as a session would (any challenge will do)
            import hyperfridge_r0_amd as r0
            import session_by_hand
            import trace_forgeries
            self.blob = np.fromfile(circuit_path(name), dtype=np.uint32)
            self.oc = orc.circuit(self.blob)
            pv, run = session_by_hand.OracleProver(self.oc), trace_forgeries.honest("alu")
            self.code, self.data, glob = pv.fixed(po2)[0], run.data, run.glob.copy()
            glob[r0.TRACE_GAMMA:r0.TRACE_GAMMA + 16] = [orc.enc(int(v)) for v in np.random.default_rng(3).integers(0, tc.P, 16)]
            self.glob, self.accum = pv.totals(po2, self.data, glob), None
        elif name in tc.FAMILIES:
            fam = tc.FAMILIES[name]
            self.blob = fam.blob()
            self.oc = orc.circuit(self.blob)
            self.code, self.data = fam.witness(1 << po2, np.random.default_rng([91, po2]))
            self.glob, self.accum = fam.glob, lambda mix: fam.accum(self.data, mix)
        else:
            self.blob = np.fromfile(circuit_path(name), dtype=np.uint32)
            self.oc = orc.circuit(self.blob)
            self.code, self.data, self.glob = self.oc.witgen(po2, 5)
            self.accum = None
        self.honest = self.prove(None)
        self.honest.setflags(write=False)
        assert self.oc.verify(self.honest) == (0, "ok") and regions(self.blob, self.honest)["po2"] == po2

    def prove(self, cheat):
        return self.oc.prove(self.po2, self.code, self.data, self.glob, accum=self.accum, cheat=cheat)

    def code_root(self):
        return self.oc.code_root(self.code, self.po2)


_subjects, _seals, _verdicts = {}, {}, {}
KEPT = ("tiny", "small")


COEFF_U_PARTS = 3  # every third word of coeff_u to a test: small's 528 words are 11 s in one
SWEEPS = [(kind, None) for kind in KINDS if kind != "coeff_u"] + [("coeff_u", (k, None, COEFF_U_PARTS)) for k in range(COEFF_U_PARTS)]


SAMPLE = [("sample", (0, 16, None)), ("sample", (16, 32, None)), ("sample", (32, 36, None))]  # round 0, round 1, committed columns


def every_cheating_seal(orc, name, po2, sweeps=SWEEPS):
    """all five sweeps of a circuit (or, sweeps=SAMPLE, the whole two-round sample), in the parts the tests prove them in"""
    return [c for which, part in sweeps for c in cheating_seals(orc, name, po2, which, part)]


def product_verdict(blob, seal):
    """r0.verify_seal(blob, seal), asked once per seal: the reference of the collecting forms, on the host and on the device"""
    import hashlib

    import hyperfridge_r0_amd as r0
    key = (blob.size, hashlib.blake2b(seal.tobytes()).digest())
    if key not in _verdicts:
        _verdicts[key] = r0.verify_seal(blob, seal)
    return _verdicts[key]


def subject(orc, name, po2):
    if (name, po2) not in _subjects:
        _subjects[name, po2] = Subject(orc, name, po2)
    return _subjects[name, po2]


def cheating_seals(orc, name, po2, which, part=None):
    """[(label, cheat, seal)] of a sweep (`which` a kind, or "sample" for sample_two_rounds; part = (start, stop, step) for that slice
    of it), left unchanged; the sweeps of the circuits in KEPT, which more than one test module goes through, are proved once
    (about 70 kB a seal)"""
    if (name, po2, which, part) in _seals:
        return _seals[name, po2, which, part]
    s = subject(orc, name, po2)
    todo = sample_two_rounds(s.blob, po2) if which == "sample" else cheats(s.blob, po2, which)
    out = []
    for label, cheat in todo if part is None else todo[slice(*part)]:
        seal = s.prove(cheat)
        seal.setflags(write=False)
        out.append((label, cheat, seal))
    if name in KEPT:
        _seals[name, po2, which, part] = out
    return out
