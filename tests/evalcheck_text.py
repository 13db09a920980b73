"""An interpreter of the straight-line text r0h_circuit_emit_hip writes (csrc/evalcheck_emit.cpp), on exact-width integers: every
u32 and u64 value is a Python int, and a u32 sum (`a + b`, inside fadd or bare) or a u64 sum (the running sums T0..T3, the
Montgomery step of fmul) that would wrap raises Wrap instead of wrapping.  A bound of the generator that is too loose for the
operands at hand shows up here without a device; whether the device computes what the text says is the GPU tests' matter.

fred, fadd, fsub, fmul, fred64, dfix and dfinish are modelled as the prelude defines them (the inline assembly by what the
instructions do); the TAP macro's row stride is read from the text.  Statements are matched line by line and a line this module
does not know raises Unknown: when the generator's text changes shape, the interpreter says so instead of guessing.  Variables
live per kernel (a kernel that reads a value only an earlier kernel defined fails), the check buffer is carried from kernel to
kernel, and kernel k runs with accumulate = (k != 0), as r0h_eval_check launches it.

Below: a model of the running sums' cadence and the seeded search for a poly_mix at which a looser one wraps, and the same
interpretation of the witness checker's text (r0h_circuit_emit_hip_check), tallied per term and row."""
import re

import numpy as np

P = 2013265921
U32, U64 = 1 << 32, 1 << 64
R = U32 % P


class Wrap(Exception):
    """an unsigned sum of the text exceeded its type's width"""


class Unknown(Exception):
    """a line of the text this interpreter has no rule for"""


def add32(a, b, what):
    s = a + b
    if s >= U32:
        raise Wrap("u32 sum wraps in %s: %d + %d" % (what, a, b))
    return s


def add64(a, b, what):
    s = a + b
    if s >= U64:
        raise Wrap("u64 sum wraps in %s: %d + %d" % (what, a, b))
    return s


def fred(x):  # v_subrev_co_u32 r = x - p, vcc = borrow; v_cndmask r = vcc ? x : r
    return x if x < P else x - P


def fadd(a, b):
    return fred(add32(a, b, "fadd"))


def fsub(a, b):  # v_sub_co_u32 d = a - b, vcc = borrow; e = d + p; d = vcc ? e : d
    d = (a - b) % U32
    return (d + P) % U32 if a < b else d


def fmul(a, b):
    t = a * b
    m = (t % U32) * 0x77ffffff % U32
    return fred(add64(t, m * P, "fmul") >> 32)


def fred64(t):
    m = (t % U32) * 0x88000001 % U32
    return fred(fsub(t >> 32, (m * P) >> 32))


def dfix(t):
    return (fred(t >> 32) << 32) | (t % U32)


def dfinish(t):
    return fred64(dfix(t))


FUNCS = {"fadd": fadd, "fsub": fsub, "fmul": fmul}
_TAP_DEF = re.compile(r"#define TAP\(g, col, back\) g\[\(size_t\)\(col\) \* domain \+ \(\(i - (?:(\d+)u \* )?\(back\)\) & mask\)\]")
_VAR = re.compile(r"  const u32 v(\d+) = (.*);$")
_TERM = re.compile(r"  const u32 w(\d+) = (.*);$")
_ACC = re.compile(r"  T(\d) (\+?=) \(u64\)mixpow\[(\d+)\] \* w(\d+);$")
_DFIX = "  T0 = dfix(T0); T1 = dfix(T1); T2 = dfix(T2); T3 = dfix(T3);"
_HEAD = ('(u32* __restrict__ check, const u32* __restrict__ g0, const u32* __restrict__ g1, const u32* __restrict__ g2,\n'
         '    const u32* __restrict__ glob, const u32* __restrict__ mix, const u32* __restrict__ mixpow,\n'
         '    const u32* __restrict__ inv_van, u32 po2, u32 accumulate) {\n'
         '  const u32 domain = 4u << po2, mask = domain - 1u;\n'
         '  const u32 i = blockIdx.x * 256u + threadIdx.x;\n'
         '  u64 T0 = 0, T1 = 0, T2 = 0, T3 = 0;\n'
         '  {\n')
_TAIL = ('  }\n'
         '  u32 t0 = dfinish(T0), t1 = dfinish(T1), t2 = dfinish(T2), t3 = dfinish(T3);\n'
         '  const u32 iv = inv_van[i & 3u];\n'
         '  t0 = fmul(t0, iv); t1 = fmul(t1, iv); t2 = fmul(t2, iv); t3 = fmul(t3, iv);\n'
         '  if (accumulate) {\n'
         '    t0 = fadd(t0, check[i]); t1 = fadd(t1, check[(size_t)domain + i]);\n'
         '    t2 = fadd(t2, check[2 * (size_t)domain + i]); t3 = fadd(t3, check[3 * (size_t)domain + i]);\n'
         '  }\n'
         '  check[i] = t0; check[(size_t)domain + i] = t1; check[2 * (size_t)domain + i] = t2; check[3 * (size_t)domain + i] = t3;\n'
         '}\n\n')
_EXPR = [
    (re.compile(r"(\d+)u$"), lambda m: ("const", int(m.group(1)))),
    (re.compile(r"TAP\(g(\d), (\d+)u, (\d+)u\)$"), lambda m: ("tap", int(m.group(1)), int(m.group(2)), int(m.group(3)))),
    (re.compile(r"(glob|mix)\[(\d+)\]$"), lambda m: (m.group(1), int(m.group(2)))),
    (re.compile(r"v(\d+) \+ v(\d+)$"), lambda m: ("lazy", int(m.group(1)), int(m.group(2)))),
    (re.compile(r"(fadd|fsub|fmul)\(v(\d+), v(\d+)\)$"), lambda m: (m.group(1), int(m.group(2)), int(m.group(3)))),
]
_GATED = re.compile(r"fmul\(v(\d+), (.*)\)$")


class Text:
    """the parsed text: .stride (rows per unit of back), .kernels = [[statement]], a statement being ("var", v, expr),
    ("term", t, [gate vars, outermost first], value var), ("acc", q, fresh, mixpow index, t) or ("dfix",)"""

    def __init__(self, src):
        m = _TAP_DEF.search(src)
        if not m:
            raise Unknown("no TAP macro of the known shape")
        self.stride = int(m.group(1) or 1)
        parts = src.split('extern "C" __global__ __launch_bounds__(256) void eval_check_')
        self.n_kernels = int(parts[0].split("kernels: ")[1].split("\n")[0])
        self.kernels = []
        for k, part in enumerate(parts[1:]):
            if not (part.startswith(str(k) + _HEAD) and part.endswith(_TAIL)):
                raise Unknown("kernel %d: frame of an unknown shape" % k)
            body = part[len(str(k) + _HEAD):-len(_TAIL)]
            self.kernels.append([self._statement(line) for line in body.split("\n") if line])
        if len(self.kernels) != self.n_kernels:
            raise Unknown("the text announces %d kernels and holds %d" % (self.n_kernels, len(self.kernels)))

    @staticmethod
    def _statement(line):
        m = _VAR.match(line)
        if m:
            for pattern, make in _EXPR:
                e = pattern.match(m.group(2))
                if e:
                    return ("var", int(m.group(1)), make(e))
            raise Unknown(line)
        m = _TERM.match(line)
        if m:
            gates, val = [], m.group(2)
            while True:
                g = _GATED.match(val)
                if not g:
                    break
                gates.append(int(g.group(1)))
                val = g.group(2)
            if not re.match(r"v\d+$", val):
                raise Unknown(line)
            return ("term", int(m.group(1)), gates, int(val[1:]))
        m = _ACC.match(line)
        if m:
            return ("acc", int(m.group(1)), m.group(2) == "=", int(m.group(3)), int(m.group(4)))
        if line == _DFIX:
            return ("dfix",)
        raise Unknown(line)

    def powers_used(self):
        """{term: power of poly_mix it is folded with}, from the mixpow indices (4 power + component)"""
        out = {}
        for kernel in self.kernels:
            for st in kernel:
                if st[0] == "acc":
                    assert st[3] % 4 == st[1] and out.setdefault(st[4], st[3] // 4) == st[3] // 4
        return out


def mix_powers(poly_mix, n_pow):
    """Montgomery words of poly_mix^0 .. poly_mix^(n_pow - 1) in F_p[x] / (x^4 - 11), 4 words each: r0h_eval_check's mixpow block"""
    r_inv = pow(U32, P - 2, P)
    pm = [int(x) * r_inv % P for x in poly_mix]
    cur, out = [1, 0, 0, 0], []
    for _ in range(n_pow):
        out += [c * R % P for c in cur]
        c = [0] * 7
        for i in range(4):
            for j in range(4):
                c[i + j] += cur[i] * pm[j]
        cur = [(c[0] + 11 * c[4]) % P, (c[1] + 11 * c[5]) % P, (c[2] + 11 * c[6]) % P, c[3] % P]
    return out


def inverse_vanishing(po2):
    """Montgomery words of 1 / ((3 w^i)^N - 1) for i mod 4 = 0..3: (3 w^i)^N = 3^N (w^N)^i with w^N = 137^(2^25), of order 4"""
    w4, three_n = pow(137, 1 << 25, P), pow(3, 1 << po2, P)
    return [pow((three_n * pow(w4, k, P) - 1) % P, P - 2, P) * R % P for k in range(4)]


def run(text, po2, lanes, ea, ec, ed, glob, mix, poly_mix, check_fill=0xA5A5A5A5):
    """{lane: [4 words of check]} after all kernels of `text` (a Text) ran on those lanes, the check buffer starting as `check_fill`"""
    domain = 4 << po2
    groups = [np.asarray(g, dtype=np.uint32).reshape(-1) for g in (ea, ec, ed)]
    scal = {"glob": [int(x) for x in glob], "mix": [int(x) for x in mix]}
    n_pow = 1 + max(st[3] // 4 for kernel in text.kernels for st in kernel if st[0] == "acc")
    mixpow, inv_van = mix_powers(poly_mix, n_pow), inverse_vanishing(po2)
    out = {}
    for i in lanes:
        check = [check_fill] * 4
        for k, kernel in enumerate(text.kernels):
            v, w, T = {}, {}, [0, 0, 0, 0]
            for st in kernel:
                if st[0] == "var":
                    e = st[2]
                    if e[0] == "const":
                        r = e[1]
                    elif e[0] == "tap":
                        r = int(groups[e[1]][e[2] * domain + ((i - text.stride * e[3]) % U32 & (domain - 1))])
                    elif e[0] in scal:
                        r = scal[e[0]][e[1]]
                    elif e[0] == "lazy":
                        r = add32(v[e[1]], v[e[2]], "v%d" % st[1])
                    else:
                        r = FUNCS[e[0]](v[e[1]], v[e[2]])
                    if st[1] in v:
                        raise Unknown("v%d defined twice in kernel %d" % (st[1], k))
                    v[st[1]] = r
                elif st[0] == "term":
                    r = v[st[3]]
                    for g in reversed(st[2]):
                        r = fmul(v[g], r)
                    w[st[1]] = r
                elif st[0] == "acc":
                    _, q, fresh, at, t = st
                    T[q] = add64(0 if fresh else T[q], mixpow[at] * w[t], "T%d at term %d, kernel %d, lane %d" % (q, t, k, i))
                else:
                    T = [dfix(x) for x in T]
            t = [fmul(dfinish(x), inv_van[i & 3]) for x in T]
            if k:
                t = [fadd(x, c) for x, c in zip(t, check)]
            check = t
        out[i] = check
    return out


# ---- the cadence of the running sums, as a model: for finding operands at which a looser cadence would wrap -------------------
def cadence_wraps(mixpow_words, first, every, n_terms, w=P - 1):
    """Does some component's running sum wrap over n_terms products mixpow[t] * w when the high word is corrected before product
    `first` and before every `every`-th product after it (the generator: first 4, every 2)?  mixpow_words: uint64 [candidates]
    [n_terms][4] -> bool [candidates].  uint64 numpy arithmetic; a wrapped sum is smaller than what it was."""
    m = np.asarray(mixpow_words, dtype=np.uint64)
    T = np.zeros((m.shape[0], 4), dtype=np.uint64)
    wrapped = np.zeros(m.shape[0], dtype=bool)
    p64, lo = np.uint64(P), np.uint64(U32 - 1)
    for t in range(n_terms):
        if t >= first and (t - first) % every == 0:
            hi = T >> np.uint64(32)
            hi = np.where(hi >= p64, hi - p64, hi)
            T = (hi << np.uint64(32)) | (T & lo)
        nxt = T + m[:, t, :] * np.uint64(w)
        wrapped |= (nxt < T).any(axis=1)
        T = nxt
    return wrapped


def find_sharp_poly_mix(seed, first, every, n_terms, budget=1 << 20, chunk=1 << 15):
    """The first poly_mix (4 Montgomery words), among at most `budget` seeded random ones, whose powers make a running sum of
    n_terms bare terms at p - 1 wrap under the cadence (first, every) and not under the generator's (4, 2); None if there is none."""
    rng = np.random.default_rng(seed)
    p64 = np.uint64(P)
    for _ in range(budget // chunk):
        pm = rng.integers(0, P, size=(chunk, 4), dtype=np.uint64)  # canonical
        cur = np.zeros((chunk, 4), dtype=np.uint64)
        cur[:, 0] = 1
        powers = []
        for _t in range(n_terms):
            powers.append((cur * np.uint64(R)) % p64)
            c = [np.zeros(chunk, dtype=np.uint64) for _ in range(7)]
            for i in range(4):
                for j in range(4):
                    c[i + j] = (c[i + j] + (cur[:, i] * pm[:, j]) % p64) % p64
            cur = np.stack([(c[0] + np.uint64(11) * c[4]) % p64, (c[1] + np.uint64(11) * c[5]) % p64, (c[2] + np.uint64(11) * c[6]) % p64, c[3]], axis=1)
        m = np.stack(powers, axis=1)
        hit = cadence_wraps(m, first, every, n_terms) & ~cadence_wraps(m, 4, 2, n_terms)
        if hit.any():
            return [int(x) * R % P for x in pm[int(np.argmax(hit))]]
    return None


# ---- the witness checker's text (r0h_circuit_emit_hip_check): the same statements, tallied per term instead of folded ---------
_CHECK_HEAD = ('(u32* __restrict__ table, const u32* __restrict__ g0, const u32* __restrict__ g1, const u32* __restrict__ g2,\n'
               '    const u32* __restrict__ glob, const u32* __restrict__ mix, u32 po2, u32 with_accum) {\n'
               '  const u32 domain = 1u << po2, mask = domain - 1u;\n'
               '  const u32 i = blockIdx.x * blockDim.x + threadIdx.x;\n')
_TALLY = re.compile(r"  tally\(table, (\d+)u, (.*), i\);$")


class CheckText:
    """the parsed checker: .stride, .kernels = [[(statement, under the with_accum switch?)]], statements as in Text with
    ("tally", t, gates, value var) for a term"""

    def __init__(self, src):
        defs = _TAP_DEF.findall(src)
        if len(defs) != 2 or "#undef TAP\n#define TAP" not in src:
            raise Unknown("the checker redefines TAP once")
        self.stride = int(defs[1] or 1)
        parts = src.split('extern "C" __global__ __launch_bounds__(256) void check_witness_')
        self.kernels = []
        for k, part in enumerate(parts[1:]):
            if not (part.startswith(str(k) + _CHECK_HEAD) and part.endswith("}\n\n")):
                raise Unknown("checker kernel %d: frame of an unknown shape" % k)
            body, late, out = part[len(str(k) + _CHECK_HEAD):-3].split("\n"), False, []
            for line in body:
                if not line:
                    continue
                if line == "  if (with_accum) {" and not late:
                    late = True
                elif line == "  }" and late:
                    late = None  # closed: nothing may follow
                elif late is None:
                    raise Unknown("a statement after the with_accum block: " + line)
                else:
                    m = _TALLY.match(line)
                    if m:
                        st = Text._statement("  const u32 w%s = %s;" % m.groups())
                        out.append((("tally",) + st[1:], late))
                    else:
                        out.append((Text._statement(line), late))
            self.kernels.append(out)


def run_check(text, po2, code, data, glob, accum=None, mix=None):
    """{term: (rows on which it does not vanish, the first of them)} as the checker's kernels tally it over all 2^po2 rows; without
    `accum` the statements under the switch do not run, and one outside it that reads group 0 or a mix word raises (the device
    is handed no such buffer)"""
    n = 1 << po2
    groups = [None if g is None else np.asarray(g, dtype=np.uint32).reshape(-1) for g in (accum, code, data)]
    scal = {"glob": [int(x) for x in glob], "mix": None if accum is None or mix is None else [int(x) for x in mix]}
    rows = {}
    for i in range(n):
        for kernel in text.kernels:
            v = {}
            for st, late in kernel:
                if late and accum is None:
                    continue
                if st[0] == "var":
                    e = st[2]
                    if e[0] == "const":
                        r = e[1]
                    elif e[0] == "tap":
                        if groups[e[1]] is None:
                            raise Unknown("v%d reads group %d outside the with_accum switch" % (st[1], e[1]))
                        r = int(groups[e[1]][e[2] * n + ((i - text.stride * e[3]) % U32 & (n - 1))])
                    elif e[0] in scal:
                        if scal[e[0]] is None:
                            raise Unknown("v%d reads a mix word outside the with_accum switch" % st[1])
                        r = scal[e[0]][e[1]]
                    elif e[0] == "lazy":
                        r = add32(v[e[1]], v[e[2]], "v%d" % st[1])
                    else:
                        r = FUNCS[e[0]](v[e[1]], v[e[2]])
                    v[st[1]] = r
                else:
                    r = v[st[3]]
                    for g in reversed(st[2]):
                        r = fmul(v[g], r)
                    if r:
                        rows.setdefault(st[1], []).append(i)
    return {t: (len(r), r[0]) for t, r in rows.items()}
