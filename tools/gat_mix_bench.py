#!/usr/bin/env python
"""The GAT RHS with mix_features (gnpde.function_GAT_attention) on the benchmark's G-arxiv
graph (synthetic.rw_graph, N = 169,343, E' = 1,200,000, C = 128), two heads, attention_dim
64 and 128, both attention_norm_idx, in ONE process:

  (a) new       node scores, statistics, wx = x W (gnpde_linear_f32), z = A_mean wx (the
                GAT-weight K1 at width attention_dim), gnpde_linear_rhs_f32 (z Wout with
                the epilogue a (ax - x) + b x0 fused);
  (b) composed  the same RHS from the kernels that existed before gnpde_linear_rhs_f32:
                ax = gnpde_linear_f32(z, Wout^T), then torch elementwise
                sigmoid(alpha) (ax - x) + beta x0 (device scalars, no host sync);
  (c) plain     the mix_features=False GAT RHS (gnpde_attn_gat_rhs_f32 over x), beside them.

Each path is replayed from a captured graph and timed with HIP events, the paths
alternating and their order rotating every round; medians over the rounds (at least nine),
with the spread (max - min over the rounds).  The outputs of (a) and (b) are compared first
(<= 1e-6 of max |f|).  The output stage alone (gnpde_linear_rhs_f32 against gnpde_linear_f32
+ the elementwise epilogue) is timed the same way, and so is one fixed-grid Runge-Kutta
stage (k_i stored and the next stage input formed) fused into the product against f followed
by gnpde_stage_apply_f32 (their outputs compared bit for bit).  Bar: (a) is not slower than (b) by more
than the measured spread (the larger of the two paths').  Prints one JSON document
(--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

from gnpde import ops, synthetic  # noqa: E402


def stage_bytes(R, K, C):
    """Algorithmic bytes of the output stage (every operand once; fp32)."""
    new = 4 * (R * K + C * K + 3 * R * C)                   # z, Wout^T, x, x0 in; f out
    ax_round_trip = 2 * 4 * R * C                           # ax written by the product, read by the epilogue
    return {"linear_rhs": new, "linear_then_epilogue": new + ax_round_trip}


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


def alternate(graphs, rounds, reps):
    """{name: [ms per round]}: every round times each graph once, the order rotating."""
    names = list(graphs)
    for cg in graphs.values():  # warm all
        time_ms(cg, 20)
    t = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            t[k].append(time_ms(graphs[k], reps))
    return t


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--att", type=int, nargs="*", default=[64, 128])
    p.add_argument("--rounds", type=int, default=11)
    p.add_argument("--reps", type=int, default=100)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("gat_mix_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("gat_mix_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    N, E, C, H = a.nodes, a.edges, a.dim, 2
    ei, _ = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    x0 = synthetic.features(1, N, C, seed=3, device=dev)
    g = ops.GraphCSR(ei, N)
    alpha = torch.tensor(0.3, device=dev)
    beta = torch.tensor(0.6, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    res = {"graph": "G-arxiv" if (N, E) == (synthetic.ARXIV_N, synthetic.ARXIV_E) else "custom", "N": N,
           "E": int(ei.shape[2]), "C": C, "heads": H, "rounds": a.rounds, "reps": a.reps,
           "library": os.path.basename(os.environ.get("GNPDE_LIB", "libgnpde.so")), "cases": []}
    with torch.no_grad():
        for att in a.att:
            W = torch.randn(C, att, generator=gen, device=dev) * (0.3 / (C / 12.0) ** 0.5)
            Wout = torch.randn(att, C, generator=gen, device=dev) * (0.3 / (att / 12.0) ** 0.5)
            av = torch.randn(2 * (att // H), generator=gen, device=dev) * 0.5
            Wt, Wot = W.t().contiguous(), Wout.t().contiguous()
            ws = ops.gat_workspace(x, 1)
            for norm_idx in (0, 1):
                fuse = ops.gat_fuse_default(H, norm_idx)
                outs = {k: torch.empty_like(x) for k in ("new", "composed", "plain")}
                zbuf = {}

                def front():
                    ns = ops.gat_scores(g, x, W, av, H, 0.2, ws=ws)
                    wx = ops.linear(x, Wt)[0].view(1, N, att)
                    return ops.attn_rhs(g, ns, None, None, norm_idx, wx, rhs=False, fuse=fuse)

                def epilogue_torch(ax, out):
                    # three in-place passes, no temporaries of the state's size
                    torch.sub(ax.view_as(x), x, out=out)
                    out.mul_(torch.sigmoid(alpha))
                    out.addcmul_(x0, beta)

                def new():
                    z = front()
                    zbuf["z"] = z
                    ops.linear_rhs(z, Wot, x, x0=x0, alpha=alpha, beta=beta, add_source=True,
                                   out=outs["new"].view(-1, C))

                def composed():
                    z = front()
                    epilogue_torch(ops.linear(z, Wot)[0], outs["composed"])

                def plain():
                    ns = ops.gat_scores(g, x, W, av, H, 0.2, ws=ws)
                    ops.attn_rhs(g, ns, None, None, norm_idx, x, x0=x0, alpha=alpha, beta=beta, add_source=True,
                                 fuse=fuse, out=outs["plain"].view(-1, C))

                graphs = {"new": captured(new), "composed": captured(composed), "plain": captured(plain)}
                dev_ab = float((outs["new"] - outs["composed"]).abs().max() / outs["composed"].abs().max())
                t = alternate(graphs, a.rounds, a.reps)
                # the output stage alone, on the z of this case
                z = zbuf["z"].clone()
                so = {k: torch.empty_like(x) for k in ("linear_rhs", "linear_then_epilogue")}
                sg = {"linear_rhs": captured(lambda: ops.linear_rhs(z, Wot, x, x0=x0, alpha=alpha, beta=beta,
                                                                    add_source=True,
                                                                    out=so["linear_rhs"].view(-1, C))),
                      "linear_then_epilogue": captured(lambda: epilogue_torch(ops.linear(z, Wot)[0],
                                                                              so["linear_then_epilogue"]))}
                ts = alternate(sg, a.rounds, a.reps)
                # a fixed-grid stage (k_i stored, the next stage input y0 + c1 k1 + c2 k2 + cf f): fused
                # into the product against f + the stage pass
                sb = {k: torch.randn(x.shape, generator=gen, device=dev) for k in ("y0", "k1", "k2", "ki", "out")}
                stage = ops.Stage(f_out=sb["ki"], outs=[(sb["out"], sb["y0"], 1.0, 0.125,
                                                         [(sb["k1"], 0.25), (sb["k2"], -0.5)])])
                ftmp = torch.empty_like(x)

                def stage_unfused():
                    ops.linear_rhs(z, Wot, x, x0=x0, alpha=alpha, beta=beta, add_source=True, out=ftmp.view(-1, C))
                    ops.stage_apply(stage, ftmp, x, x)

                tg = {"fused": captured(lambda: ops.linear_rhs(z, Wot, x, x0=x0, alpha=alpha, beta=beta,
                                                               add_source=True, stage=stage))}
                fused_out = sb["out"].clone()
                tg["f_then_stage_apply"] = captured(stage_unfused)
                stage_equal = bool(torch.equal(fused_out, sb["out"]))
                tt = alternate(tg, a.rounds, a.reps)
                case = {"attention_dim": att, "norm_idx": norm_idx, "gat_k1_fused": bool(fuse),
                        "new_vs_composed_rel": dev_ab, "outputs_agree": dev_ab <= 1e-6,
                        "rhs_ms": {k: stats(v) for k, v in t.items()},
                        "output_stage_ms": {k: stats(v) for k, v in ts.items()},
                        "output_stage_bytes": stage_bytes(g.R, att, C),
                        "rk_stage_ms": {k: stats(v) for k, v in tt.items()}, "rk_stage_bitwise_equal": stage_equal}
                spread = max(case["rhs_ms"][k]["max"] - case["rhs_ms"][k]["min"] for k in ("new", "composed"))
                case["spread_ms"] = round(spread, 5)
                case["new_minus_composed_ms"] = round(case["rhs_ms"]["new"]["median"] -
                                                      case["rhs_ms"]["composed"]["median"], 5)
                case["within_bar"] = case["new_minus_composed_ms"] <= spread
                res["cases"].append(case)
                print("att=%d norm_idx=%d: RHS new %.4f ms, composed %.4f ms, plain GAT %.4f ms (spread %.4f ms, "
                      "within bar %s); output stage: linear_rhs %.4f ms, linear + epilogue %.4f ms; rk stage: fused "
                      "%.4f ms, f + stage_apply %.4f ms (bitwise equal %s); new vs composed %.2e" % (
                          att, norm_idx, case["rhs_ms"]["new"]["median"], case["rhs_ms"]["composed"]["median"],
                          case["rhs_ms"]["plain"]["median"], spread, case["within_bar"],
                          case["output_stage_ms"]["linear_rhs"]["median"],
                          case["output_stage_ms"]["linear_then_epilogue"]["median"],
                          case["rk_stage_ms"]["fused"]["median"], case["rk_stage_ms"]["f_then_stage_apply"]["median"],
                          stage_equal, dev_ab), flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
