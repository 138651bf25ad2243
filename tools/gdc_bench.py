#!/usr/bin/env python
"""The GDC rewiring (ops.gdc: diffusion column blocks on K1 + the column top-k kernel) at the
sizes it runs at, both shapes in one process (the default --shapes), between HIP events after
warm-up (median / min / max):

  Cora-sized (N = 2,708, the RMAT graph of gnpde.synthetic made undirected, k = 64, ppr
  alpha = 0.05), in full;  G-arxiv (N = 169,343): --blocks column blocks of 128 seeds, the
  per-block time and the IMPLIED total (x ceil(N / 128) blocks; implied, not measured).

Per shape: one K1 product at W = 128 (a plain A·x launch, and the mean over a block's fused
stage launches); a block's recurrence with both seed-term variants ('operand': E_J passed as a
stage operand; 'diagonal': added to the block's diagonal after each launch); topk_cols against
torch.topk on the transposed block on the same device; the block pipeline (or the whole
ops.gdc at Cora size) against its torch restatement (torch.sparse.mm products,
ops.topk_cols_torch — what a user without the kernels would write; it is not the code under
test); at Cora size also torch.linalg.inv of the dense system, the reference's exact method.

Prints one JSON document (--out FILE also writes it, again after every shape, so a run cut
short at the second shape keeps the first).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

import gnpde  # noqa: E402
from gnpde import _lib, ops, synthetic  # noqa: E402
from gnpde.graph_rewiring import to_undirected  # noqa: E402

SHAPES = {"Cora-sized": (synthetic.CORA_N, synthetic.CORA_E, True),
          "G-arxiv": (synthetic.ARXIV_N, synthetic.ARXIV_E, False)}
K, ALPHA, W = 64, 0.05, 128


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gdc_bench: no GPU, nothing to measure")
    dev = "cuda:0"
    doc = {"device": torch.cuda.get_device_name(0), "build_id": gnpde.build_info()["build_id"], "k": K,
           "alpha": ALPHA, "block": W, "cases": {},
           "note": "implied_total_s = per-block time x column_blocks: implied, not measured, unless the case "
                   "has a whole-gdc entry"}
    sched = ops.diffusion_schedule('ppr', alpha=ALPHA)
    for name in args.shapes.split(","):
        N, E, full = SHAPES[name]
        print("%s: graph" % name, file=sys.stderr, flush=True)
        ei = to_undirected(synthetic.rmat_edges(N, E // 2, seed=0, device=dev), N)
        row, col, val = ops.gdc_matrix(ei, None, N, 1.0)
        e3 = torch.stack([row, col]).unsqueeze(0).contiguous()
        tw = ops.norm_weights(e3, val.unsqueeze(0).contiguous(), N, _lib.NORM_GCN)
        g = ops.GraphCSR(e3, N, validate=False)
        w = g.gather_weights(tw)
        Tm = torch.sparse_coo_tensor(torch.stack([row, col]), tw.reshape(-1), (N, N)).coalesce()
        n_blocks = (N + W - 1) // W
        j0s = [(i * (n_blocks - 1) // max(args.blocks - 1, 1)) * W for i in range(args.blocks)]
        ent = {"N": N, "edges_undirected": int(ei.shape[1]), "nnz_T": int(row.numel()), "products_per_block":
               sched.products, "column_blocks": n_blocks}
        x = synthetic.features(1, N, W, device=dev)[0].contiguous()
        ent["k1_plain_product"] = timed(lambda: ops.spmm_rhs(g, w, x, rhs=False), args.warmup, args.reps)
        for seed in ("operand", "diagonal"):
            print("%s: recurrence, seed %s" % (name, seed), file=sys.stderr, flush=True)
            t = timed(lambda: ops.diffusion_block(g, w, j0s[0], W, sched, seed=seed), args.warmup, args.reps)
            t["per_product_us"] = 1e3 * t["median_ms"] / sched.products
            ent["recurrence_block_seed_" + seed] = t
        Y = ops.diffusion_block(g, w, j0s[0], W, sched)
        print("%s: selection" % name, file=sys.stderr, flush=True)
        ent["topk_cols"] = timed(lambda: ops.topk_cols(Y, K), args.warmup, args.reps)
        ent["torch_topk_transposed"] = timed(lambda: torch.topk(Y.t(), K, dim=1), args.warmup, args.reps)
        idx = ops.topk_cols(Y, K)[0]
        ent["topk_index_agreement_with_torch"] = float(
            (idx.long().sort(1).values == torch.topk(Y.t(), K, dim=1).indices.sort(1).values).float().mean())

        def blocks_native():
            for j0 in j0s:
                ops.topk_cols(ops.diffusion_block(g, w, j0, min(W, N - j0), sched), K)

        def blocks_torch():
            for j0 in j0s:
                ops.topk_cols_torch(ops.diffusion_block_torch(Tm, j0, min(W, N - j0), sched), K)

        print("%s: block pipeline" % name, file=sys.stderr, flush=True)
        nat = timed(blocks_native, 1, args.reps)
        tor = timed(blocks_torch, 1, args.baseline_reps)
        for t in (nat, tor):
            t["blocks"] = len(j0s)
            t["per_block_ms"] = t["median_ms"] / len(j0s)
            t["implied_total_s"] = t["per_block_ms"] * n_blocks / 1e3
        ent["block_pipeline"] = nat
        ent["block_pipeline_torch"] = tor
        if full:
            print("%s: whole gdc" % name, file=sys.stderr, flush=True)
            ent["gdc"] = timed(lambda: ops.gdc(ei, None, N, alpha=ALPHA, k=K), 1, args.reps)
            ent["gdc_torch"] = timed(lambda: ops.gdc_torch(ei, None, N, alpha=ALPHA, k=K), 1, args.baseline_reps)
            A = torch.eye(N, device=dev) - (1.0 - ALPHA) * Tm.to_dense()
            ent["torch_linalg_inv_dense"] = timed(lambda: torch.linalg.inv(A), 1, args.baseline_reps)
            ea, wa = ops.gdc(ei, None, N, alpha=ALPHA, k=K)
            eb, wb = ops.gdc_torch(ei, None, N, alpha=ALPHA, k=K)
            ent["gdc_edge_set_overlap_with_torch"] = float(
                torch.isin(ea[0] * N + ea[1], eb[0] * N + eb[1]).float().mean())
        doc["cases"][name] = ent
        print(json.dumps({name: ent}), file=sys.stderr, flush=True)
        text = json.dumps(doc, indent=1, sort_keys=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
