#!/usr/bin/env python3
"""Tile-step launches of bench.py's timed calls, grouped by their position k in the call (the kinds of launch of a
single-filter recurrence call: step 1, step 2, flush-free steps, read-modify-write flushes, the last step), from a
rocprofv3 --kernel-trace CSV of one plain bench.py run and that run's JSON line: duration, the bytes the kind must
move (bench.py's model: CSR + n U) and the resulting rate.
    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python bench.py > DIR/bench.json
    python tools/step_kinds.py DIR/**/t_kernel_trace.csv DIR/bench.json [label]   -> one markdown table"""
import csv
import json
import sys

import numpy as np

trace, bench = sys.argv[1], sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
b = json.loads(open(bench).read().strip().splitlines()[-1])
cfg = b["config"]
N, nsig, K = cfg["N"], cfg["Nsig"], cfg["order"]
elt = 4 if b.get("dtype") == "f32" else 8
U = N * nsig * elt
csr = cfg["nnz_L"] * (elt + 4) + 4 * (N + 1)
timed = int(b["roofline"]["launches_timed"])
rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"]), r["Kernel_Name"])
              for r in csv.DictReader(open(trace)) if "k_step_tile" in r.get("Kernel_Name", ""))
assert len(rows) >= timed > 0 and timed % K == 0, (len(rows), timed, K)
rows = rows[-timed:]
# the fused plan of one filter (make_plan_fused): flushes at k = 2, 5, 8, ... and at K
flush = [k for k in range(1, K + 1) if k == K or (k >= 2 and (k - 2) % 3 == 0)]
kinds = [("step 1 (gamma = 0, no flush)", [1], 2),
         ("step 2 (first flush: write)", [2], 4),
         ("flush-free steps", [k for k in range(3, K) if k not in flush], 3),
         ("read-modify-write flushes", [k for k in flush if 2 < k < K], 5),
         ("last step (flush into y)", [K], 5)]
print("| {} kind | k | launches | median us | min..max us | bytes (model) | TB/s at the median |".format(label).replace("|  ", "| "))
print("|---|---|---|---|---|---|---|")
for name, ks, nu in kinds:
    d = np.array([rows[i][1] for i in range(timed) if (i % K) + 1 in ks], dtype=np.float64) / 1e3
    names = sorted({rows[i][2].split("(")[0][:60] for i in range(timed) if (i % K) + 1 in ks})
    by = csr + nu * U
    print("| {} | {} | {} | {:.1f} | {:.1f}..{:.1f} | CSR + {}U = {:.3f} GB | {:.2f} |".format(
        name, ",".join(map(str, ks)) if len(ks) <= 3 else "{}..{} ({})".format(ks[0], ks[-1], len(ks)), len(d),
        np.median(d), d.min(), d.max(), nu, by / 1e9, by / (np.median(d) * 1e-6) / 1e12))
    print("<!-- kernels: {} -->".format("; ".join(names)))
tot = sum(r[1] for r in rows) / 1e6 / (timed // K)
print("\nsum of the {} launches of a call: {:.3f} ms (trace); bench.py: device_ms_recurrence_per_step {:.3f} ms, "
      "avg_launch_ms {:.5f}, value {:.4g}".format(K, tot, b["device_ms_recurrence_per_step"],
                                                 b["roofline"]["avg_launch_ms"], b["value"]))
