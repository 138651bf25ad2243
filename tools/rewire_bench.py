#!/usr/bin/env python
"""The two-hop product of the rewire_attention block (csrc/two_hop.hip through ops.two_hop) at
the sizes a rewire runs at, in ONE process:

  a Cora-sized graph (2,708 nodes, 13,264 edges) and the largest G-arxiv-like RMAT graph
  (169,343 nodes, 1.2 M edges, halved until it fits) whose product stays under 2^31
  positions; self loops, rw-normalised weights (gnpde.synthetic.rw_graph).

Per graph: ops.two_hop between HIP events after warm-up (median / min / max of --reps calls:
the coalescing prep pass, the bound, symbolic and numeric passes, the scan and the one host
read); the torch restatement ops.two_hop_torch on the same device and input by its sparse
route (torch.sparse.mm + coalesce: what a user without the kernel would write), timed the
same way with --baseline-reps calls above --full-nnz positions; at the Cora size also the
reference's dense route (to_dense, [N, N] matmul: src/block_transformer_rewiring.py:68-77);
the results compared (positions exactly, values relatively); the product's length and the
bytes the passes move: `bytes_compulsory` (W read once, the product written once) and
`bytes_gathered` (every neighbour row read once per owner row, columns in the symbolic pass,
columns and values in the numeric one, plus the product).

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
from gnpde import ops, synthetic  # noqa: E402


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


def case(name, N, E, args, dense):
    dev = "cuda:0"
    ei, w = synthetic.rw_graph(N, E, seed=0, device=dev)
    g = ops.GraphCSR(ei, N)
    print("%s: N %d, E %d: kernel" % (name, N, ei.shape[2]), file=sys.stderr, flush=True)
    e, v, rowptr = ops.two_hop(g, w)            # raises ValueError at 2^31 positions or more
    nnz = int(e.shape[2])
    kern = timed(lambda: ops.two_hop(g, w), args.warmup, args.reps)
    full = nnz > args.full_nnz
    print("%s: torch sparse baseline (%d positions)" % (name, nnz), file=sys.stderr, flush=True)
    base = timed(lambda: ops.two_hop_torch(g, w, dense_n=0), 0 if full else args.warmup,
                 args.baseline_reps if full else args.reps)
    e2, v2, rowptr2 = ops.two_hop_torch(g, w, dense_n=0)
    rp, col, val = ops.coalesced_csr(g, w.contiguous())
    nnz_w = int(rp[-1])
    lens = (rp[1:] - rp[:-1]).long()
    ub_sum = int(lens[col[:nnz_w].long()].sum())
    out_bytes = nnz * (4 + 4 + 16) + 4 * (N + 1)
    doc = {
        "nodes": N, "edges": int(ei.shape[2]), "coalesced_edges": nnz_w, "nnz": nnz, "sum_ub": ub_sum,
        "rows_lds": int(((ops_ub(rp, col, nnz_w) <= ops.TWO_HOP_LDS_MAX)).sum()),
        "kernel_ms": kern, "torch_sparse_ms": base, "torch_sparse_over_kernel": base["median"] / kern["median"],
        "bytes_compulsory": nnz_w * 8 + 4 * (N + 1) + out_bytes,
        "bytes_gathered": ub_sum * (4 + 8) + 2 * nnz_w * 8 + out_bytes,
        "positions_equal_to_baseline": bool(torch.equal(e, e2) and torch.equal(rowptr, rowptr2)),
        "max_rel_value_difference": float(((v - v2).abs() / v2.abs().clamp(min=1e-30)).max()) if nnz else 0.0,
    }
    doc["gathered_gb_per_s"] = doc["bytes_gathered"] / (kern["median"] * 1e-3) / 1e9
    del e2, v2
    if dense:
        print("%s: the reference's dense route" % name, file=sys.stderr, flush=True)
        doc["dense_route_ms"] = timed(lambda: ops.two_hop_torch(g, w, dense_n=1 << 30), args.warmup, args.reps)
        doc["dense_route_over_kernel"] = doc["dense_route_ms"]["median"] / kern["median"]
    torch.cuda.empty_cache()
    return doc


def ops_ub(rp, col, nnz_w):
    """The rows' width bounds (sum of the neighbour rows' lengths), in torch."""
    lens = (rp[1:] - rp[:-1]).long()
    per = lens[col[:nnz_w].long()]
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=per.device), torch.cumsum(per, 0)])
    return csum[rp[1:].long()] - csum[rp[:-1].long()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-reps", type=int, default=1)
    ap.add_argument("--full-nnz", type=int, default=50_000_000)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rewire_bench: no GPU, nothing to measure")
    if args.reps < 10:
        sys.exit("rewire_bench: --reps must be at least 10")
    doc = {"device": torch.cuda.get_device_name(0), "build_id": gnpde.build_info()["build_id"],
           "lds_max": ops.TWO_HOP_LDS_MAX, "cases": {}}
    doc["cases"]["Cora-sized"] = case("Cora-sized", synthetic.CORA_N, synthetic.CORA_E, args, dense=True)
    N, E, tried = synthetic.ARXIV_N, synthetic.ARXIV_E, []
    while N >= 1024:
        try:
            doc["cases"]["G-arxiv-like"] = dict(case("G-arxiv-like", N, E, args, dense=False), too_large=tried)
            break
        except ValueError as exc:   # 2^31 positions or more: halve the graph
            tried.append({"nodes": N, "edges": E, "error": str(exc)})
            torch.cuda.empty_cache()
            N, E = N // 2, E // 2
    out = json.dumps(doc, indent=1)
    print(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(out + "\n")


if __name__ == "__main__":
    main()
