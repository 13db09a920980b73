"""Where things lie in a seal, and one mutation of every kind the collecting verifier has to agree with the immediate one on
(tests/test_verify_collecting.py without a GPU, tests/test_gpu_verify_on_device.py with the device hashing the openings).

The layout is csrc/seal_layout.hpp's, stated from sizes alone (nothing is hashed here): globals and po2; the top layers of CODE, DATA,
ACCUM, CHECK; coeff_u; the FRI rounds' top layers; the final polynomial; then per query the openings of ACCUM, CODE, DATA, CHECK and
of every FRI round, each `cols` values followed by its path digests."""
import numpy as np

from sha_suite_ref import CHECK_SIZE, FRI_FOLD, FRI_MIN_DEGREE, INV_RATE, QUERIES, P, parse_blob


def _shape(rows, cols):
    layers, top_layer = rows.bit_length() - 1, 0
    for i in range(1, layers):
        if (1 << i) > QUERIES:
            break
        top_layer = i
    return {"rows": rows, "cols": cols, "top_words": 8 << top_layer, "path": layers - top_layer}


def regions(blob, seal):
    """name -> (start, end) for the tops ("code_top", .., "fri0_top", ..), "coeff_u", "final"; "opening" -> {(tree, query): (values
    start, path start, end)}; "groups" / "fri": the tree names in opening order; "words": the seal's length by its layout"""
    c = parse_blob(blob)
    for po2 in range(9, 25):  # (the seal's po2 word is in Montgomery form: the size is taken from the length, which only one fits)
        r = _regions(c, po2)
        if r["words"] == len(seal):
            return r
    raise AssertionError("no trace size gives a seal of %d words" % len(seal))


def _regions(c, po2):
    n, domain = 1 << po2, INV_RATE << po2
    out, pos = {}, c["n_global"] + 1
    trees = {"accum": _shape(domain, c["group_size"][0]), "code": _shape(domain, c["group_size"][1]), "data": _shape(domain, c["group_size"][2]),
             "check": _shape(domain, CHECK_SIZE)}
    for name in ("code", "data", "accum", "check"):
        out[name + "_top"] = (pos, pos + trees[name]["top_words"])
        pos += trees[name]["top_words"]
    n_u = c["n_taps"] + CHECK_SIZE
    out["coeff_u"] = (pos, pos + 4 * n_u)
    pos += 4 * n_u
    fri, deg = [], n
    while deg > FRI_MIN_DEGREE:
        name = "fri%d" % len(fri)
        trees[name] = _shape(deg * INV_RATE // FRI_FOLD, FRI_FOLD * 4)
        out[name + "_top"] = (pos, pos + trees[name]["top_words"])
        pos += trees[name]["top_words"]
        fri.append(name)
        deg //= FRI_FOLD
    out["final"] = (pos, pos + 4 * deg)
    pos += 4 * deg
    out["groups"], out["fri"], out["opening"] = ["accum", "code", "data", "check"], fri, {}
    for q in range(QUERIES):
        for name in out["groups"] + fri:
            t = trees[name]
            out["opening"][(name, q)] = (pos, pos + t["cols"], pos + t["cols"] + 8 * t["path"])
            pos += t["cols"] + 8 * t["path"]
    out["words"], out["po2"] = pos, po2
    return out


def _bump(seal, pos):
    bad = seal.copy()
    bad[pos] = (int(bad[pos]) + 1) % P
    assert bad[pos] != seal[pos]
    return bad


def _raise(seal, lo, hi):
    """the first word of [lo, hi) that + p still fits 32 bits, raised by p: another word sequence for the same field element"""
    for pos in range(lo, hi):
        if int(seal[pos]) + P < 1 << 32:
            bad = seal.copy()
            bad[pos] = int(bad[pos]) + P
            return bad
    raise AssertionError("no word of the range can be raised by p")


def mutations(blob, seal):
    """[(label, mutated seal)]: one of every kind.  `expect` in the label's place would tie this to one suite; the tests compare with
    the immediate verifier instead and pin the codes that do not depend on the suite themselves."""
    seal = np.ascontiguousarray(seal, dtype=np.uint32)
    r = regions(blob, seal)
    op, last_fri = r["opening"], r["fri"][-1]
    out = [("untouched", seal.copy())]
    out.append(("top-layer word, group tree", _bump(seal, r["data_top"][0] + 3)))
    out.append(("top-layer word, FRI tree", _bump(seal, r[last_fri + "_top"][0] + 9)))
    out.append(("leaf value, group tree", _bump(seal, op[("data", 7)][0] + 1)))
    out.append(("leaf value, FRI tree", _bump(seal, op[(last_fri, 7)][0] + 5)))
    out.append(("path digest, group tree", _bump(seal, op[("accum", 2)][1] + 8 + 3)))
    out.append(("path digest, FRI tree", _bump(seal, op[("fri0", 2)][1] + 1)))
    out.append(("non-canonical sibling", _raise(seal, op[("code", 4)][1], op[("code", 4)][2])))
    out.append(("non-canonical leaf value", _raise(seal, op[("check", 4)][0], op[("check", 4)][1])))
    out.append(("coeff_u word", _bump(seal, r["coeff_u"][0] + 6)))
    out.append(("final-coefficient word", _bump(seal, r["final"][0] + 2)))
    out.append(("truncation inside an opening", seal[:op[("data", 10)][1] + 5].copy()))
    out.append(("one extra word", np.concatenate([seal, np.zeros(1, np.uint32)])))
    two = _bump(seal, op[("accum", 3)][1] + 2)  # a path digest in query 3 ...
    two = _bump(two, op[("fri0", 1)][0] + 4)    # ... and a FRI value in query 1: query 1 comes first in the seal
    out.append(("two faults: path digest in query 3, FRI value in query 1", two))
    return out
