"""Tree tops (r0h_merkle_top / _open_top, r0h_proof_data_top / _begin_committed_top, r0h_ctx_set_session_tree_tops) as far as they can
be seen without a GPU: the entries exist at every layer, the command line names its option, NULL arguments are errors, and the
reference's path arithmetic is the seal layout's.  What they do is tests/test_gpu_merkle_top.py's, test_gpu_proof_tree_top.py's and
test_gpu_session_tree_tops.py's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hyperfridge_r0_amd as r0
import merkle_top_ref as ref
from conftest import ROOT

NEW = ("r0h_merkle_top", "r0h_merkle_open_top", "r0h_proof_data_top", "r0h_proof_begin_committed_top", "r0h_ctx_set_session_tree_tops", "r0h_last_session_tree_tops")


def test_the_new_entries_are_exported_declared_and_bound():
    lib = r0.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r0hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in r0.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
    assert re.search(r"#define R0H_MERKLE_TOP_MAX_LEVELS %d\b" % ref.MAX_TOP_LEVELS, header)
    for method in ("merkle_top", "merkle_open_top", "proof_data_top", "set_session_tree_tops", "last_session_tree_tops"):
        assert callable(getattr(r0.Hal, method)), method


def test_the_command_line_names_its_option():
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    out = subprocess.run([prove, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--session-keep-tree-tops L" in out.stdout
    tiny = os.path.join(ROOT, "circuits", "tiny.r0c")
    out = subprocess.run([prove, tiny, "--session-keep-tree-tops"], capture_output=True, text=True)
    assert out.returncode == 1 and "--session-keep-tree-tops needs a value" in out.stderr
    for value in ("6", "9"):
        out = subprocess.run([prove, tiny, "--session-keep-tree-tops", value], capture_output=True, text=True)
        assert out.returncode == 1 and "--session-keep-tree-tops takes 0 .. 8 levels and goes with --elf" in out.stderr
    bench = open(os.path.join(ROOT, "tools", "bench_session.py")).read()
    assert "--keep-tree-tops" in bench and "segments_replayed_from_their_tree_top" in bench


def test_null_arguments_are_errors_not_crashes():
    lib = r0.lib()
    first, handle = ctypes.c_uint32(7), ctypes.c_void_p()
    with pytest.raises(r0.R0HipError, match="r0h_merkle_top: NULL argument"):
        r0._check(lib.r0h_merkle_top(None, None, 64, 1, None))
    with pytest.raises(r0.R0HipError, match="r0h_merkle_open_top: NULL argument"):
        r0._check(lib.r0h_merkle_open_top(None, None, None, None, 1, None, 1, 64, 1, ctypes.byref(first)))
    with pytest.raises(r0.R0HipError, match="r0h_proof_data_top: NULL argument"):
        r0._check(lib.r0h_proof_data_top(None, 6, None))
    with pytest.raises(r0.R0HipError, match="r0h_proof_begin_committed_top: NULL argument"):
        r0._check(lib.r0h_proof_begin_committed_top(None, None, 9, None, None, None, None, 6, None, ctypes.byref(handle)))
    assert first.value == 7 and not handle.value
    with pytest.raises(r0.R0HipError, match="r0h_ctx_set_session_tree_tops: ctx is NULL"):
        r0._check(lib.r0h_ctx_set_session_tree_tops(None, 6))
    out = (ctypes.c_uint64 * 3)()
    with pytest.raises(r0.R0HipError, match="r0h_last_session_tree_tops: NULL argument"):
        r0._check(lib.r0h_last_session_tree_tops(None, out))


def test_the_reference_counts_path_digests_as_the_seal_layout_does():
    """layers - top_layer, the top layer being the deepest one of at most 50 nodes: the shapes the GPU tests rest on, and the session's"""
    assert [ref.path_digests(1 << k) for k in (1, 5, 6, 7, 11, 13, 18, 22)] == [1, 1, 1, 2, 6, 8, 13, 17]
    assert ref.opening_words(1 << 11, 17) == 17 + 8 * 6
    assert ref.top_digests(1 << 18, 6) * 32 == 262144 and ref.top_digests(1 << 22, 6) * 32 == 4 << 20
    # an opening of a four-leaf tree of labelled digests: the seal carries layer 1, so the leaf's sibling is the whole path
    nodes = np.arange(8 * 8, dtype=np.uint32).reshape(8, 8)
    got = ref.openings(np.array([[10, 11, 12, 13]], dtype=np.uint32), nodes, [2])
    assert np.array_equal(got, [np.concatenate([[12], nodes[7]])])
