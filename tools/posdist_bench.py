#!/usr/bin/env python
"""The positional-encoding distance kernels (csrc/posdist.hip through ops.pos_knn,
ops.pair_quantile, ops.pair_threshold_edges) at the sizes a pos_enc_knn rewire runs at:

  Cora (2,708 x 16), PubMed (19,717 x 16), ogbn-arxiv at HYPS16's and DW64's widths
  (169,343 x 16, 169,343 x 64); both metrics; k = 64, quant = 1/1000; points drawn inside the
  unit ball from a seed.

Every (shape, metric) case runs in a fresh child process under a time limit of its own; the
driver stops at the first child that fails or runs out of time (nothing more is started on the
device after a fault).  Per case: each op between HIP events after warm-up (median / min / max
of --reps calls; pair_threshold_edges includes its one host read and the allocation of the edge
list), the torch restatements on the same device where their dense fp32 matrix fits
(--baseline-max-bytes), and the implied rates: pairs / s and pair-columns / s (N^2 C per sweep
of the full matrix; the select's three sweeps cover the upper triangle, 1.5 N^2 per select).

Prints one JSON document (--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))

SHAPES = {"Cora": (2708, 16), "PubMed": (19717, 16), "arxiv-HYPS16": (169343, 16), "arxiv-DW64": (169343, 64)}
METRICS = ("poincare", "euclid")
K, QUANT = 64, 1 / 1000


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "reps": reps}


def run_case(name, metric, args):
    import torch

    import gnpde
    from gnpde import ops
    if not torch.cuda.is_available():
        sys.exit("posdist_bench: no GPU, nothing to measure")
    N, C = SHAPES[name]
    g = torch.Generator(device="cpu").manual_seed(1)
    v = torch.randn(N, C, generator=g)
    x = (v / v.norm(dim=1, keepdim=True) * (0.05 + 0.9 * torch.rand(N, 1, generator=g))).to("cuda:0")
    lo, hi, frac = ops.pair_rank(N, QUANT)
    selects = 2 if (hi > lo and frac != 0.0) else 1
    doc = {"rows": N, "width": C, "metric": metric, "k": K, "quant": QUANT, "selects_per_quantile": selects,
           "device": torch.cuda.get_device_name(0), "build_id": gnpde.build_info()["build_id"]}
    ops_ = {"pos_knn": lambda: ops.pos_knn(x, K, metric, return_dist=True),
            "pair_quantile": lambda: ops.pair_quantile(x, QUANT, metric),
            "pair_threshold_edges": lambda: ops.pair_threshold_edges(x, QUANT, metric)}
    base = {"pos_knn": lambda: ops.pos_knn_torch(x, K, metric, return_dist=True, chunk_bytes=1 << 32),
            "pair_quantile": lambda: ops.pair_quantile_torch(x, QUANT, metric),
            "pair_threshold_edges": lambda: ops.pair_threshold_edges_torch(x, QUANT, metric)}
    # full-matrix sweeps of N^2 pairs each op makes
    sweeps = {"pos_knn": 1.0, "pair_quantile": 1.5 * selects, "pair_threshold_edges": 1.5 + 2.0}
    for op, fn in ops_.items():
        t = timed(torch, fn, args.warmup, args.reps)
        pairs = sweeps[op] * N * N
        doc[op] = {"kernel_ms": t, "sweeps": sweeps[op], "pairs_per_s": pairs / (t["median"] * 1e-3),
                   "pair_columns_per_s": pairs * C / (t["median"] * 1e-3)}
        print("%s %s %s: %.3f ms" % (name, metric, op, t["median"]), file=sys.stderr, flush=True)
        if 4 * N * N <= args.baseline_max_bytes:
            b = timed(torch, base[op], 1, args.baseline_reps)
            doc[op]["torch_baseline_ms"] = b
            doc[op]["baseline_over_kernel"] = b["median"] / t["median"]
    thr, u_lo, cnt = ops.pair_quantile(x, QUANT, metric)
    doc["u_lo"], doc["thr"], doc["edges"] = float(u_lo), float(thr), int(cnt)
    print(json.dumps(doc))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--metrics", default=",".join(METRICS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--baseline-max-bytes", type=int, default=2 << 30)
    ap.add_argument("--case-timeout", type=int, default=150, help="seconds per (shape, metric) child")
    ap.add_argument("--case", help="(internal) run one case in this process: NAME:METRIC")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.reps < 10:
        sys.exit("posdist_bench: --reps must be at least 10")
    if args.case:
        name, metric = args.case.split(":")
        return run_case(name, metric, args)
    doc = {"k": K, "quant": QUANT, "cases": {}}
    for name in args.shapes.split(","):
        for metric in args.metrics.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", "%s:%s" % (name, metric), "--reps",
                   str(args.reps), "--warmup", str(args.warmup), "--baseline-reps", str(args.baseline_reps),
                   "--baseline-max-bytes", str(args.baseline_max_bytes)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.case_timeout)
            except subprocess.TimeoutExpired:
                sys.exit("posdist_bench: %s %s ran past %d s: stopping" % (name, metric, args.case_timeout))
            if r.returncode != 0:
                sys.exit("posdist_bench: %s %s ended with status %d: stopping" % (name, metric, r.returncode))
            doc["cases"]["%s/%s" % (name, metric)] = json.loads(r.stdout.decode().strip().splitlines()[-1])
            if args.out:   # (kept current case by case)
                with open(args.out, "w") as fh:
                    fh.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
