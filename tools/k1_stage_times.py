#!/usr/bin/env python
"""Per-stage times of the headline K1 in a rocprofv3 kernel trace of
`bench.py --gpus 1 --steps K --warmup W`: the last 4 K dispatches of the fused-stage
kernel (of its column-striped form, and of its frozen-tail form, the solve's last launch) are the
timed solve's, four
per rk4 step in stage order.
python tools/k1_stage_times.py <run_kernel_trace.csv> [K]"""
import csv
import statistics
import sys

NAME = "void gnpde::agg_kernel<4, 32, 1, 4, 2, 1, gnpde::PlainWeights, float>"
# a step's last launch on a graph with frozen rows (kStgFrozen)
NAME_FROZEN = "void gnpde::agg_kernel<4, 32, 1, 4, 2, 6, gnpde::PlainWeights, float>"
# the same stage launch in S column stripes (large graphs)
NAMES_STRIPED = ("void gnpde::agg_stripe_kernel<4, 1>", "void gnpde::agg_stripe_kernel<2, 1>")

rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 50
ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows
            if r["Kernel_Name"].startswith((NAME, NAME_FROZEN) + NAMES_STRIPED))
striped = sum(r["Kernel_Name"].startswith(NAMES_STRIPED) for r in rows)
print("K1 fused-stage dispatches: %d (%d striped) | names: %s*, %s*" % (len(ev), striped, NAME, NAMES_STRIPED[0][:-5]))
ev = ev[-4 * steps:]
for s in range(4):
    d = [(e - b) / 1e3 for b, e in ev[s::4]]
    print("stage %d: mean %.1f us  median %.1f  min %.1f  max %.1f  (n=%d)" % (
        s + 1, statistics.mean(d), statistics.median(d), min(d), max(d), len(d)))
span = (ev[-1][1] - ev[0][0]) / 1e3
busy = sum(e - b for b, e in ev) / 1e3
print("span of the last %d launches %.1f us, busy %.1f us (%.1f %%)" % (len(ev), span, busy, 100.0 * busy / span))
