#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the plan of r0h_hash_fold_top (tools/fuzz/merkle_fused_check.cpp): for every tree
# of 2^0 .. 2^26 rows under both hash suites, the launches of csrc/merkle_fused_plan.hpp are carried out on a host array with the host
# suite's hash_pair -- every node produced once, no read of what another workgroup of the same launch writes, the same nodes as the
# level-by-level fold.  CPU only: the plan header, the host-only suite units and a stand-alone main; no device code is built or
# run, nothing is loaded into Python.
# (hash_suite.cpp is linked for the two suites and claim.cpp for its SHA-256 compression alone: with a section per function the linker
# drops the context, receipt and verifier entry points beside them, and with those their references to units that are not built here.)
#   tools/fuzz/run_merkle_fused_check.sh [work dir, default /tmp/r0h_merkle_fused_check]
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
WORK=${1:-/tmp/r0h_merkle_fused_check}
mkdir -p "$WORK"
FLAGS="-O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -Wno-unknown-pragmas -ffunction-sections -Wl,--gc-sections -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
CSRC="$ROOT/hyperfridge-r0_amd/csrc"
g++ $FLAGS -I "$CSRC" -o "$WORK/merkle_fused_check" "$ROOT/tools/fuzz/merkle_fused_check.cpp" "$CSRC/hash_suite.cpp" "$CSRC/poseidon2_host.cpp" "$CSRC/claim.cpp"
"$WORK/merkle_fused_check"
