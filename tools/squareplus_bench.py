#!/usr/bin/env python
"""The squareplus transformer RHS (opt['square_plus'], csrc/squareplus.hip) on the benchmark's
G-arxiv graph (synthetic.rw_graph, N = 169,343, E' = 1,200,000), C = 128, fp32, two heads
(attention_dim 32), against the softmax RHS as it stands — in ONE process, the variants
interleaved, each replayed from a captured graph and timed with HIP events; medians over the
rounds, with the spread.

Row "reference_n1" (the fork's scaled_dot scores, attention_norm_idx 1): the softmax RHS
(ops.attn_rhs), the squareplus RHS with the fused K1 (gnpde_attn_sp_rhs_f32) and with the
separate weights pass; the two squareplus outputs are compared bit for bit first.
Row "per_edge_n0" (per-edge scaled_dot, attention_norm_idx 0): the softmax RHS (one fused
pass, gnpde_attn_dot_rhs_f32) and the squareplus RHS (score max + stored scores, statistics,
weights pass, K1).  The squareplus passes are also timed one by one, so the table says which
pass carries a difference.  Prints one JSON document (--out FILE also writes it).  No GPU:
it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

from gnpde import ops, synthetic  # noqa: E402


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


def interleaved(graphs, rounds, reps):
    """Medians (+ min / max) of the captured graphs, timed alternately, the order rotated every round."""
    names = list(graphs)
    for cg in graphs.values():
        time_ms(cg, 20)
    t = {k: [] for k in names}
    for r in range(rounds):
        order = names[r % len(names):] + names[:r % len(names)]
        for k in order:
            t[k].append(time_ms(graphs[k], reps))
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
            for k, v in t.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--heads", type=int, default=2)
    p.add_argument("--attention-dim", type=int, default=32)
    p.add_argument("--rounds", type=int, default=15)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("squareplus_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    N, E, C, H, att = a.nodes, a.edges, a.dim, a.heads, a.attention_dim
    ei, _ = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    g = ops.GraphCSR(ei, N)
    alpha = torch.tensor(0.0, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    Wq, Wk = [torch.randn(att, C, generator=gen, device=dev) * 0.05 for _ in range(2)]
    bq, bk = [torch.randn(att, generator=gen, device=dev) * 0.05 for _ in range(2)]
    wcat = (torch.cat([Wq, Wk], 0).contiguous(), torch.cat([bq, bk], 0).contiguous())
    res = {"graph": "G-arxiv" if (N, E) == (synthetic.ARXIV_N, synthetic.ARXIV_E) else "custom", "N": N,
           "E": int(ei.shape[2]), "C": C, "heads": H, "attention_dim": att, "rounds": a.rounds, "reps": a.reps,
           "rows": {}}
    with torch.no_grad():
        for row, mode, norm_idx in (("reference_n1", "reference", 1), ("per_edge_n0", "per_edge", 0)):
            def scores():
                return ops.node_scores(g, x, Wq, bq, Wk, bk, H, 'scaled_dot', mode,
                                       wcat=wcat if mode == "per_edge" else None)

            ns0 = scores()
            bufs = ops.squareplus_buffers(g, ns0.mode, H, dev)
            outs = {k: torch.empty_like(x) for k in ("softmax", "squareplus_fused", "squareplus_unfused")}

            def softmax(out):
                ops.attn_rhs(g, scores(), None, None, norm_idx, x, alpha=alpha, out=out.view(-1, C))

            def squareplus(fuse, out):
                ops.squareplus_rhs(g, scores(), norm_idx, x, alpha=alpha, fuse=fuse, bufs=bufs, out=out.view(-1, C))

            graphs = {"softmax": captured(lambda: softmax(outs["softmax"]))}
            if mode == "reference":
                graphs["squareplus_fused"] = captured(lambda: squareplus(True, outs["squareplus_fused"]))
            graphs["squareplus_unfused"] = captured(lambda: squareplus(False, outs["squareplus_unfused"]))
            case = {"score_mode": mode, "norm_idx": norm_idx, "rhs_ms": interleaved(graphs, a.rounds, a.reps)}
            if mode == "reference":
                case["fused_bitwise_equal_unfused"] = bool(torch.equal(outs["squareplus_fused"],
                                                                       outs["squareplus_unfused"]))
            # the squareplus passes one by one (each captured alone, on the operands of a full run)
            sq = ops.score_max(g, ns0, bufs)
            rl = ops.squareplus_stats(g, ns0, sq, norm_idx)
            w = ops.squareplus_weights(g, ns0, sq, rl, norm_idx)
            o = torch.empty_like(x)
            passes = {"node_scores": captured(scores),
                      "score_max": captured(lambda: ops.score_max(g, ns0, bufs)),
                      "squareplus_stats": captured(lambda: ops.squareplus_stats(g, ns0, sq, norm_idx)),
                      "squareplus_weights": captured(lambda: ops.squareplus_weights(g, ns0, sq, rl, norm_idx)),
                      "k1_plain": captured(lambda: ops.spmm_rhs(g, w, x, alpha=alpha, out=o.view(-1, C)))}
            if mode == "reference":
                fw = ops.RefDstSquareplusWeights(sq.pn, rl, H)
                passes["k1_fused"] = captured(lambda: ops.spmm_rhs(g, fw, x, alpha=alpha, out=o.view(-1, C)))
                passes["softmax_stats"] = captured(lambda: ops.softmax_stats(g, ns0, 1, packed=H == 2))
            case["pass_ms"] = interleaved(passes, max(3, a.rounds // 3), a.reps)
            ms = case["rhs_ms"]
            best = min((k for k in ms if k != "softmax"), key=lambda k: ms[k]["median"])
            case["best_squareplus"] = best
            case["squareplus_over_softmax"] = round(ms[best]["median"] / ms["softmax"]["median"], 4)
            res["rows"][row] = case
            print("%s: %s; squareplus/softmax %.3f (%s)" % (
                row, ", ".join("%s %.4f ms" % (k, v["median"]) for k, v in ms.items()),
                case["squareplus_over_softmax"], best), flush=True)
            print("   passes: " + ", ".join("%s %.4f" % (k, v["median"]) for k, v in case["pass_ms"].items()),
                  flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
