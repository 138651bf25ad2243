#!/usr/bin/env python
"""The exact top-k kernel of the kNN rewiring (gnpde_knn_f32 through ops.knn) at the sizes a
rewire runs at, in ONE process:

  ogbn-arxiv rows at G-arxiv's width (169,343 x 128), at BLEND's width (169,343 x 162), and a
  Cora-sized graph (2,708 x 80); k = 64 (every best_params entry), standard normal inputs
  from a seed.

Per shape: ops.knn between HIP events after warm-up (median / min / max of --reps calls, mask
pre-pass included); the torch restatement ops.knn_torch on the same device and input, timed
the same way (what a user without the kernel would write: chunked difference form, integer
(d, j) keys, topk — it is not the code under test, and at the full sizes it takes seconds,
so it gets --baseline-reps calls); the two results compared at the size timed (index
agreement; a difference is a pair of candidates the two fp32 summation orders rank
differently); and the derived lower bound: N^2 C terms of one subtract and one fused
multiply-add, 4 N^2 C FLOP, at the packed-fp32 vector peak of 157.3 TFLOP/s.

Prints one JSON document (--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

import gnpde  # noqa: E402
from gnpde import ops  # noqa: E402

PEAK_FLOPS = 157.3e12  # packed fp32 VALU, MI355X
SHAPES = {"G-arxiv": (169343, 128, 64), "BLEND": (169343, 162, 64), "Cora-sized": (2708, 80, 64)}
FULL_SIZE = 50000  # rows above which the baseline gets --baseline-reps calls


def timed(fn, warmup, reps):
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
        print("  %.3f ms" % ms[-1], file=sys.stderr, flush=True)
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=1)
    ap.add_argument("--baseline-chunk-bytes", type=int, default=1 << 32)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("knn_bench: no GPU, nothing to measure")
    if args.reps < 10:
        sys.exit("knn_bench: --reps must be at least 10")
    dev = "cuda:0"
    doc = {"device": torch.cuda.get_device_name(0), "build_id": gnpde.build_info()["build_id"],
           "peak_flops": PEAK_FLOPS, "cases": {}}
    for name in args.shapes.split(","):
        N, C, k = SHAPES[name]
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.randn(N, C, generator=g).to(dev)
        print("%s: kernel" % name, file=sys.stderr, flush=True)
        kern = timed(lambda: ops.knn(x, k, return_dist=True), args.warmup, args.reps)
        full = N > FULL_SIZE
        print("%s: torch baseline" % name, file=sys.stderr, flush=True)
        base = timed(lambda: ops.knn_torch(x, k, return_dist=True, chunk_bytes=args.baseline_chunk_bytes),
                     0 if full else args.warmup, args.baseline_reps if full else args.reps)
        idx, _, n_valid = ops.knn(x, k, return_dist=True)
        want = ops.knn_torch(x, k, chunk_bytes=args.baseline_chunk_bytes)[0]
        bound_ms = 4.0 * N * N * C / PEAK_FLOPS * 1e3
        doc["cases"][name] = {
            "rows": N, "width": C, "k": k, "n_valid": n_valid.tolist(),
            "kernel_ms": kern, "torch_baseline_ms": base, "baseline_chunk_bytes": args.baseline_chunk_bytes,
            "baseline_over_kernel": base["median"] / kern["median"],
            "bound_ms": bound_ms, "fraction_of_bound": bound_ms / kern["median"],
            "achieved_tflops": 4.0 * N * N * C / (kern["median"] * 1e-3) / 1e12,
            "entries_equal_to_baseline": float((idx == want).float().mean()),
            "rows_equal_to_baseline": float((idx == want).all(dim=-1).float().mean()),
        }
        del x, idx, want
        torch.cuda.empty_cache()
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
