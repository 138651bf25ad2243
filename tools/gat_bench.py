#!/usr/bin/env python
"""The GAT RHS (gnpde.function_GAT_attention) on the benchmark's G-arxiv graph
(synthetic.rw_graph, N = 169,343, E' = 1,200,000, C = 128), heads 2 and 4 (dk = 16),
both attention_norm_idx: the fused K1 (gnpde_attn_gat_rhs_f32) against the weights pass +
the plain K1, in ONE process, alternating, each replayed from a captured graph and timed
with HIP events; medians over the rounds, with the spread.  The outputs of the two paths
are compared bit for bit first.  Prints the algorithmic bytes of each launch and one JSON
document (--out FILE also writes it).  No GPU: it fails (nothing to measure).

For context only (not a bar): the transformer RHS on this graph is 0.141 / 0.149 ms
(DESIGN.md §6)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

from gnpde import ops, synthetic  # noqa: E402

TRANSFORMER_RHS_MS = (0.141, 0.149)  # DESIGN.md §6, context only


def launch_bytes(R, nnz, C, H, norm_idx):
    """Algorithmic bytes of each launch (the operands read and written once; gathers counted
    per edge): state fp32, node-score pairs fp64 [R,2H], statistics m fp64 + rl fp32 [R,H]."""
    idx = 4 * nnz                                   # the other endpoint of every edge
    pair_row, sr = 16 * H, 8 * H
    stats_out = 12 * H * R
    b = {}
    b["gat_scores"] = 4 * R * C + pair_row * R
    # statistics: one item row per group + the other endpoint's half of the pair per edge
    b["softmax_stats"] = idx + nnz * sr + R * sr + stats_out
    k1 = idx + 4 * nnz * C + 2 * 4 * R * C          # gathered rows, x_r in, f out
    per_edge_stats = nnz * 12 * H if norm_idx == 1 else 0
    per_row_stats = R * 12 * H if norm_idx == 0 else 0
    b["attn_weights"] = 2 * idx + nnz * pair_row + nnz * 12 * H + 4 * nnz
    b["spmm_rhs"] = k1 + 4 * nnz
    b["attn_gat_rhs"] = k1 + nnz * sr + R * sr + per_edge_stats + per_row_stats
    b["unfused_total"] = b["gat_scores"] + b["softmax_stats"] + b["attn_weights"] + b["spmm_rhs"]
    b["fused_total"] = b["gat_scores"] + b["softmax_stats"] + b["attn_gat_rhs"]
    return b


def captured(fn):
    fn()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        fn()
    torch.cuda.synchronize()
    return cg


def time_ms(cg, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        cg.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=200)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    N, E, C = a.nodes, a.edges, a.dim
    ei, _ = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    g = ops.GraphCSR(ei, N)
    alpha = torch.tensor(0.0, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    res = {"graph": "G-arxiv" if (N, E) == (synthetic.ARXIV_N, synthetic.ARXIV_E) else "custom", "N": N,
           "E": int(ei.shape[2]), "C": C, "rounds": a.rounds, "reps": a.reps,
           "transformer_rhs_ms_context": list(TRANSFORMER_RHS_MS), "cases": []}
    with torch.no_grad():
        for H in (2, 4):
            att = 16 * H
            W = torch.randn(C, att, generator=gen, device=dev) * (0.3 / (C / 12.0) ** 0.5)
            av = torch.randn(2 * 16, generator=gen, device=dev) * 0.5
            ws = ops.gat_workspace(x, 1)
            for norm_idx in (0, 1):
                outs = {k: torch.empty_like(x) for k in ("fused", "unfused")}

                def rhs(fuse, out):
                    ns = ops.gat_scores(g, x, W, av, H, 0.2, ws=ws)
                    ops.attn_rhs(g, ns, None, None, norm_idx, x, alpha=alpha, fuse=fuse, out=out.view(-1, C))

                graphs = {"fused": captured(lambda: rhs(True, outs["fused"])),
                          "unfused": captured(lambda: rhs(False, outs["unfused"]))}
                same = bool(torch.equal(outs["fused"], outs["unfused"]))
                for cg in graphs.values():  # warm both
                    time_ms(cg, 20)
                t = {"fused": [], "unfused": []}
                for r in range(a.rounds):  # alternating, the order swapped every round
                    for k in (("fused", "unfused") if r % 2 == 0 else ("unfused", "fused")):
                        t[k].append(time_ms(graphs[k], a.reps))
                case = {"heads": H, "attention_dim": att, "norm_idx": norm_idx, "bitwise_equal": same,
                        "bytes": launch_bytes(g.R, g.nnz, C, H, norm_idx)}
                for k in t:
                    case[k + "_ms"] = {"median": round(statistics.median(t[k]), 5), "min": round(min(t[k]), 5),
                                       "max": round(max(t[k]), 5)}
                case["fused_over_unfused"] = round(case["fused_ms"]["median"] / case["unfused_ms"]["median"], 4)
                res["cases"].append(case)
                print("h=%d norm_idx=%d: fused %.4f ms, unfused %.4f ms (ratio %.3f), bitwise equal %s; "
                      "bytes fused %.1f MB unfused %.1f MB; transformer RHS for context %.3f / %.3f ms" % (
                          H, norm_idx, case["fused_ms"]["median"], case["unfused_ms"]["median"],
                          case["fused_over_unfused"], same, case["bytes"]["fused_total"] / 1e6,
                          case["bytes"]["unfused_total"] / 1e6, *TRANSFORMER_RHS_MS), flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
