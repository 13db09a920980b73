"""The device limit of a session (r0h_ctx_set_session_device_limit) and the rows handles it rests on (r0h_trace_rows_*), as far as
they can be seen without a GPU: the entries exist at every layer, the command line names its option, and NULL arguments are
errors.  What they do is tests/test_gpu_session_eviction.py's."""
import ctypes
import os
import re
import subprocess

import pytest

import hyperfridge_r0_amd as r0
from conftest import ROOT

NEW = ("r0h_trace_rows_upload", "r0h_trace_rows_expand", "r0h_trace_rows_bytes", "r0h_trace_rows_free", "r0h_ctx_set_session_device_limit",
       "r0h_last_session_device", "r0h_ctx_session_held_bytes")


def test_the_new_entries_are_exported_declared_and_bound():
    lib = r0.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "r0hip.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "r0hip_sys.rs")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in r0.EXPORTED_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert "pub fn %s(" % name in rust, name
    assert "pub struct r0h_trace_rows" in rust
    # r0h_session_stats keeps its layout: callers pass a struct of that size
    assert ctypes.sizeof(r0.SessionStats) == 48
    for method in ("set_session_device_limit", "last_session_device", "session_held_bytes", "trace_rows_upload", "trace_rows_expand", "trace_rows_bytes", "trace_rows_free"):
        assert callable(getattr(r0.Hal, method)), method


def test_the_command_line_names_its_option():
    prove = os.path.join(ROOT, "hyperfridge-r0_amd", "r0h_prove")
    out = subprocess.run([prove, "--help"], capture_output=True, text=True)
    assert out.returncode == 0 and "--session-device-limit-gb G" in out.stdout and "evicted" in out.stdout
    out = subprocess.run([prove, os.path.join(ROOT, "circuits", "tiny.r0c"), "--session-device-limit-gb"], capture_output=True, text=True)
    assert out.returncode == 1 and "--session-device-limit-gb needs a value" in out.stderr
    out = subprocess.run([prove, os.path.join(ROOT, "circuits", "tiny.r0c"), "--session-device-limit-gb", "1"], capture_output=True, text=True)
    assert out.returncode == 1 and "goes with --elf" in out.stderr
    bench = open(os.path.join(ROOT, "tools", "bench_session.py")).read()
    assert "--device-limit-gb" in bench and "evicted_segments_of_the_reported_session" in bench


def test_null_arguments_are_errors_not_crashes():
    lib = r0.lib()
    glob = (ctypes.c_uint32 * r0.TRACE_GLOBALS)()
    seg = r0.TraceSegment(1, 1, 0, 0)
    handle = ctypes.c_void_p()
    with pytest.raises(r0.R0HipError, match="r0h_trace_rows_upload: NULL argument"):
        r0._check(lib.r0h_trace_rows_upload(None, None, 0, None, 0, 16, ctypes.byref(seg), ctypes.byref(handle), glob))
    assert not handle.value
    with pytest.raises(r0.R0HipError, match="r0h_trace_rows_expand: NULL argument"):
        r0._check(lib.r0h_trace_rows_expand(None, None))
    assert lib.r0h_trace_rows_bytes(None) == 0
    r0._check(lib.r0h_trace_rows_free(None))
    with pytest.raises(r0.R0HipError, match="r0h_ctx_set_session_device_limit: ctx is NULL"):
        r0._check(lib.r0h_ctx_set_session_device_limit(None, 1))
    out = (ctypes.c_uint64 * 4)()
    with pytest.raises(r0.R0HipError, match="r0h_last_session_device: NULL argument"):
        r0._check(lib.r0h_last_session_device(None, out))
    assert lib.r0h_ctx_session_held_bytes(None) == 0
