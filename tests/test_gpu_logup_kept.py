"""A session evaluates and scans its segment's public accumulator once: the totals step keeps the scanned terms and the accumulation
unpacks them (csrc/session.cpp finish_segment; LogupKept, logup_totals_keep, logup_accum_kept in csrc/circuit.hpp).  On the smallest
trace size, for every segment of a small session: the ACCUM columns and the public inputs through that internal path are those of
r0h_logup_totals + r0h_accum_public, and the session's seal is the seal r0h_prove_segment gives from the host reference's witness
(which accumulates without kept terms).  The internal functions are C++ (no C ABI of their own): they are reached by their mangled names."""
import ctypes
import os
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import hyperfridge_r0_amd as r0
from conftest import circuit_path
from test_rv32im import _guest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
from bench_session import elf_of  # noqa: E402

pytestmark = pytest.mark.gpu
TOTALS_KEEP = "_ZN3r0h17logup_totals_keepEP7r0h_ctxPK11r0h_circuitjPK7r0h_bufS7_PjPNS_9LogupKeptE"
ACCUM_KEPT = "_ZN3r0h16logup_accum_keptEP7r0h_ctxPK11r0h_circuitjPK7r0h_bufS7_PKjS9_PS5_PKNS_9LogupKeptE"


def internal(name, n_args):
    fn = getattr(r0.lib(), name)
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * (n_args - 3)
    fn.restype = ctypes.c_void_p
    return fn


def test_kept_terms_give_the_accum_columns_and_the_seal_of_the_public_calls(hal, orc):
    blob = np.fromfile(circuit_path("trace"), dtype=np.uint32)
    gc = hal.load_circuit(blob, entry.code_object_path("trace"))
    elf, words = elf_of(_guest(300), 0x400), [7, 0x01020304]
    receipt, _, _ = hal.prove_elf(gc, elf, words, segment_po2=16)   # finish_segment: the internal path
    seals = receipt.seals()
    vm = r0.Vm()
    vm.load_elf(elf)
    vm.set_input(words)
    assert vm.run(segment_po2=16, keep_trace=True, boundary_rows=True) == (0, 0)
    claims = vm.claims()
    assert len(seals) == len(claims) >= 1
    size, n = r0.TRACE_MIN_PO2, 1 << r0.TRACE_MIN_PO2
    code = hal.copy_from(orc.circuit(blob).witgen(size, 0)[0])
    totals_keep, accum_kept = internal(TOTALS_KEEP, 7), internal(ACCUM_KEPT, 9)
    mix = np.random.default_rng(size).integers(0, r0.P, size=gc.n_mix).astype(np.uint32)
    for k, (_, seal) in enumerate(seals):
        data, _ = vm.trace_witness(k, size, claim_globals=claims[k].globals())
        glob = seal[:r0.TRACE_GLOBALS].copy()           # the seal's own public inputs (the challenge among them), the segment's sum yet to come
        glob[r0.TRACE_SUM:r0.TRACE_SUM + 4] = 0
        db = hal.copy_from(data)
        # the public calls: every step evaluates for itself
        want_glob = hal.logup_totals(gc, size, code, db, glob)
        assert np.array_equal(want_glob, seal[:r0.TRACE_GLOBALS])
        want = hal.accum_public(gc, size, code, db, want_glob, mix)
        # the internal path: the totals step keeps its scanned terms, the accumulation unpacks them
        kept = (ctypes.c_uint64 * 8)()   # an empty LogupKept: no buffer, zero sizes
        got_glob = glob.copy()
        r0._check(totals_keep(hal.ctx, gc.handle, size, code.handle, db.handle, got_glob.ctypes.data_as(r0._vp), kept))
        assert kept[0] and kept[1] & 0xFFFFFFFF == size and kept[1] >> 32 >= 1, "the totals step kept nothing"
        got = hal.alloc(gc.group_size[r0.GROUP_ACCUM] * n)
        r0._check(accum_kept(hal.ctx, gc.handle, size, code.handle, db.handle, got_glob.ctypes.data_as(r0._vp), mix.ctypes.data_as(r0._vp), got.handle, kept))
        r0.lib().r0h_buf_free(ctypes.c_void_p(kept[0]))
        assert np.array_equal(got_glob, want_glob)
        assert np.array_equal(got.to_host(), want.to_host())
        # and with no kept terms the same function is r0h_accum_public
        r0._check(accum_kept(hal.ctx, gc.handle, size, code.handle, db.handle, got_glob.ctypes.data_as(r0._vp), mix.ctypes.data_as(r0._vp), got.handle, None))
        assert np.array_equal(got.to_host(), want.to_host())
        # the session's seal (kept terms) is the seal of the segment proved by the public call (none kept)
        assert np.array_equal(hal.prove_segment(gc, size, code, db, want_glob), seal)
        for b in (db, want, got):
            b.free()
    code.free()
    gc.free()
