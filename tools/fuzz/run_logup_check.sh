#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the host side of the log-derivative kernels (tools/fuzz/logup_host_check.cpp): the
# lookup-list builder against the host count, fp4_batch_div against separate inversions.  CPU only: host-only translation units and a
# stand-alone main; no device code is built or run, nothing is loaded into Python.
#   tools/fuzz/run_logup_check.sh [work dir, default /tmp/r0h_logup_check]
set -e
ROOT=$(cd "$(dirname "$0")/../.." && pwd)
WORK=${1:-/tmp/r0h_logup_check}
mkdir -p "$WORK"
FLAGS="-O1 -g -std=c++17 -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include"
g++ $FLAGS -o "$WORK/logup_host_check" "$ROOT/tools/fuzz/logup_host_check.cpp" "$ROOT/hyperfridge-r0_amd/csrc/logup_host.cpp" "$ROOT/hyperfridge-r0_amd/csrc/blob.cpp"
# generated circuits with both tables and their witnesses (tests/logup_circuits.py), honest and breaking the contract
python3 - "$ROOT" "$WORK" <<'PY'
import sys
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import logup_circuits as lc
import logup_ref as ref
work = sys.argv[2]
cases = []
for seed in (5, 7, 9, 17):
    c = lc.generate(seed, tables=[1, 2], n_chain=4)
    for po2 in (16, 17):
        data, glob, _ = c.witness(po2, seed=po2)
        cases.append((c, po2, data, glob))
c = lc.generate(17, tables=[1, 2], n_chain=4)
data, glob, _ = c.witness(16, seed=1)
bad = data.reshape(-1, 1 << 16).copy()
for s in c.sel:
    bad[s, 5] = ref.enc(2)
cases.append((c, 16, bad.reshape(-1), glob))
with open(work + "/cases.txt", "w") as f:
    for i, (c, po2, data, glob) in enumerate(cases):
        for name, a in (("blob", c.words), ("data", data), ("glob", glob)):
            np.asarray(a, dtype=np.uint32).tofile("%s/%s_%d.bin" % (work, name, i))
        f.write("%d %d\n" % (i, po2))
PY
while read -r i po2; do
  "$WORK/logup_host_check" "$WORK/blob_$i.bin" "$WORK/data_$i.bin" "$WORK/glob_$i.bin" "$po2" 1000
done < "$WORK/cases.txt"
echo "logup host check: no report"
