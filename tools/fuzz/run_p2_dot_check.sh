#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the dot products of the Poseidon2 partial rounds as the kernels compile them
# (tools/fuzz/p2_dot_check.cpp): both correction schedules at the exact worst case and on random states, every bound asserted in
# 128-bit arithmetic.  CPU only: the device header's host forms, the host-only table unit and a stand-alone main; no device code is
# built or run, nothing is loaded into Python.
#   tools/fuzz/run_p2_dot_check.sh [work dir, default /tmp/r0h_p2_dot_check]
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
WORK=${1:-/tmp/r0h_p2_dot_check}
mkdir -p "$WORK"
FLAGS="-O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
g++ $FLAGS -I "$ROOT/hyperfridge-r0_amd/csrc" -o "$WORK/p2_dot_check" "$ROOT/tools/fuzz/p2_dot_check.cpp" "$ROOT/hyperfridge-r0_amd/csrc/poseidon2_host.cpp"
"$WORK/p2_dot_check"
