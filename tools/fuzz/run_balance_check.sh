#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host side of the balance check (tools/fuzz/balance_host_check.cpp):
# r0h_logup_check_balance_host against an exact restatement, on tuple circuits and the trace circuit, witnesses as generated and edited;
# a host session handle against the same restatement on a two-segment session of the tests' `pairs` circuit.
# CPU only: host-only translation units and a stand-alone main; no device code is built or run, nothing is loaded into Python.
#   tools/fuzz/run_balance_check.sh [work dir, default /tmp/r0h_balance_check]
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
WORK=${1:-/tmp/r0h_balance_check}
mkdir -p "$WORK"
FLAGS="-O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
g++ $FLAGS -o "$WORK/balance_host_check" "$ROOT/tools/fuzz/balance_host_check.cpp" "$ROOT/hyperfridge-r0_amd/csrc/balance_host.cpp" "$ROOT/hyperfridge-r0_amd/csrc/logup_host.cpp" \
  "$ROOT/hyperfridge-r0_amd/csrc/blob.cpp"
python3 - "$ROOT" "$WORK" <<'PY'
import sys
sys.path.insert(0, sys.argv[1] + "/tests")
sys.path.insert(0, sys.argv[1] + "/tools")
import numpy as np
import balance_circuits as bc
import logup_ref as ref
work = sys.argv[2]
cases = []
for name in bc.SCENARIOS:
    for po2 in (4, 9):
        c, data, glob = bc.scenario(name, po2, seed=po2)
        cases.append((c.words, po2, data, glob, None, 30))
# the trace circuit's CODE tables and an idle witness (every row dead: its lookups ask for zero, the multiplicities say so)
import trace_circuit as tc
blob = np.fromfile(sys.argv[1] + "/circuits/trace.r0c", dtype=np.uint32)
n = 1 << 16
m = np.zeros((len(tc.TRACE_COLUMNS), n), dtype=np.int64)
tc.multiplicities(m, [0] * tc.TRACE_GLOBALS)
cases.append((blob, 16, ref.enc(m).reshape(-1), np.zeros(tc.TRACE_GLOBALS, dtype=np.uint32), ref.enc(np.array(tc.code_columns(n), dtype=np.int64)).reshape(-1), 3))
with open(work + "/cases.txt", "w") as f:
    for i, (words, po2, data, glob, code, edits) in enumerate(cases):
        for name, a in (("blob", words), ("data", data), ("glob", glob)) + ((("code", code),) if code is not None else ()):
            np.asarray(a, dtype=np.uint32).tofile("%s/%s_%d.bin" % (work, name, i))
        f.write("%d %d %s %d\n" % (i, po2, "%s/code_%d.bin" % (work, i) if code is not None else "-", edits))
# a session whose tuples are produced in one segment and consumed in another (tests/session_balance_circuits.py)
import session_balance_circuits as sc
c, segments = sc.session("pairs", [5, 7], seed=3)
np.asarray(c.words, dtype=np.uint32).tofile(work + "/session_blob.bin")
with open(work + "/session.txt", "w") as f:
    for source, po2, _, data, glob in segments:
        data.tofile("%s/session_data_%d.bin" % (work, source))
        glob.tofile("%s/session_glob_%d.bin" % (work, source))
        f.write("%d %s/session_data_%d.bin %s/session_glob_%d.bin " % (po2, work, source, work, source))
PY
while read -r i po2 code edits; do
  "$WORK/balance_host_check" "$WORK/blob_$i.bin" "$WORK/data_$i.bin" "$WORK/glob_$i.bin" "$po2" "$code" "$edits"
done < "$WORK/cases.txt"
# shellcheck disable=SC2046
"$WORK/balance_host_check" session "$WORK/session_blob.bin" 40 $(cat "$WORK/session.txt")
echo "balance host check: no report"
