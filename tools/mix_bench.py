#!/usr/bin/env python
"""The transformer RHS with mix_features (gnpde.function_transformer_attention) on the
benchmark's G-arxiv graph (synthetic.rw_graph, N = 169,343, E' = 1,200,000, C = 128), the
fork's scaled_dot scores, (heads, attention_dim) in {(2,128), (8,128), (4,64)}, both
attention_norm_idx (0 is the uniform case: cached per-head weights), in ONE process:

  (a) new       the whole RHS — node scores, statistics, per-head attention, v = V(x)
                (gnpde_linear_f32), z by gnpde_head_aggregate_f32, Wout with its bias and
                the epilogue (gnpde_linear_rhs_bias_f32) — and the aggregation alone;
  (b) composed  the same aggregation from kernels unchanged from the parent commit: per
                head gnpde_gather_head_f32 (scaled by 1/heads) and the plain K1 over that
                head's dk columns of v (the head slices laid out ahead of the timed part),
                summed;
  (c) plain K1  over v at width attention_dim with head-mean weights: the byte-equivalent
                yardstick (it computes something else), beside them, not a bar.

The two ways to the per-head weights are timed too, each with its producer (norm_idx 1):
the attention pass writing aggregation-CSR order [nnz, heads] (ops.head_weights) + the
aggregation, against the COO attention (ops.edge_attention) + the aggregation reading it
through the CSR's perm; and the aggregation alone with either input.  One fixed-grid
Runge-Kutta stage fused into gnpde_linear_rhs_bias_f32 against f followed by
gnpde_stage_apply_f32 (compared bit for bit).  Each path is replayed from a captured graph
and timed with HIP events, the paths alternating and their order rotating every round;
medians over the rounds (at least nine), with the spread (max - min over the rounds).  The
outputs of (a) and (b) are compared first (<= 1e-6 of max |z|).  Bar: (a) is not slower
than (b) by more than the measured spread (the larger of the two paths').  Prints one JSON
document (--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

from gnpde import ops, synthetic  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s (MI355X)


def agg_bytes(nnz, R, heads, att):
    """Algorithmic bytes of the per-head aggregation (fp32 / int32)."""
    return nnz * att * 4 + nnz * (heads + 1) * 4 + R * (att // heads) * 4


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


def spread_of(d, keys):
    return max(d[k]["max"] - d[k]["min"] for k in keys)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--dim", type=int, default=128)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("mix_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    N, E, C = a.nodes, a.edges, a.dim
    ei, _ = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    x0 = synthetic.features(1, N, C, seed=3, device=dev)
    g = ops.GraphCSR(ei, N)
    alpha = torch.tensor(0.3, device=dev)
    beta = torch.tensor(0.6, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    res = {"graph": "G-arxiv" if (N, E) == (synthetic.ARXIV_N, synthetic.ARXIV_E) else "custom", "N": N,
           "E": int(ei.shape[2]), "C": C, "rounds": a.rounds, "reps": a.reps, "hbm_peak_bytes_per_s": HBM_PEAK,
           "cases": []}
    with torch.no_grad():
        for H, att in ((2, 128), (8, 128), (4, 64)):
            dk = att // H
            Wq, Wk = [torch.randn(att, C, generator=gen, device=dev) * 0.05 for _ in range(2)]
            bq, bk = [torch.randn(att, generator=gen, device=dev) * 0.05 for _ in range(2)]
            Wv = torch.randn(att, C, generator=gen, device=dev) * (0.3 / (C / 12.0) ** 0.5)
            bv = torch.randn(att, generator=gen, device=dev) * 0.3
            Wo = torch.randn(C, dk, generator=gen, device=dev) * (0.3 / (dk / 12.0) ** 0.5)
            bo = torch.randn(C, generator=gen, device=dev) * 0.3
            for norm_idx in (0, 1):
                uniform = norm_idx == 0
                if uniform:
                    ns_u = ops.uniform_scores(H)
                    m_u, rl_u = ops.softmax_stats(g, ns_u, 0)
                    wh_u = ops.head_weights(g, ns_u, m_u, rl_u, 0)
                fout = torch.empty_like(x)
                keep = {}

                def weights():
                    if uniform:
                        return wh_u
                    ns = ops.node_scores(g, x, Wq, bq, Wk, bk, H, 'scaled_dot', 'reference')
                    m, rl = ops.softmax_stats(g, ns, norm_idx)
                    return ops.head_weights(g, ns, m, rl, norm_idx)

                def rhs_new():
                    wh = weights()
                    v = ops.linear(x, Wv, bv)[0]
                    z = ops.head_aggregate(g, wh, v)
                    keep["wh"], keep["v"] = wh, v
                    ops.linear_rhs(z, Wo, x, x0=x0, alpha=alpha, beta=beta, add_source=True, bias=bo,
                                   out=fout.view(-1, C))

                g_rhs = captured(rhs_new)
                g_rhs.replay()  # keep[...] live in the capture's pool: filled by a replay
                torch.cuda.synchronize()
                wh_csr, v = keep["wh"].clone(), keep["v"].clone()
                wh = torch.empty(1, g.E, H, device=dev)  # the same weights in COO order
                wh.view(-1, H)[g.csr.perm.long()] = wh_csr
                vh = [v[:, h * dk:(h + 1) * dk].contiguous() for h in range(H)]
                w_mean = g.gather_weights(wh)
                zs = {k: torch.empty(g.R, dk, device=dev) for k in ("new", "new_coo_weights", "composed",
                                                                    "route_csr", "route_perm")}
                if not uniform:
                    ns1 = ops.node_scores(g, x, Wq, bq, Wk, bk, H, 'scaled_dot', 'reference')
                    m1, rl1 = ops.softmax_stats(g, ns1, norm_idx)
                zfull = torch.empty(g.R, att, device=dev)

                def composed():
                    acc = zs["composed"]
                    for h in range(H):
                        w_h = ops.gather_head(g.csr, wh, h, 1.0 / H)
                        if h == 0:
                            ops.spmm_rhs(g, w_h, vh[h], rhs=False, out=acc)
                        else:
                            acc.add_(ops.spmm_rhs(g, w_h, vh[h], rhs=False))

                graphs = {
                    "rhs_new": g_rhs,
                    "agg_new": captured(lambda: ops.head_aggregate(g, wh_csr, v, out=zs["new"])),
                    "agg_new_coo_weights": captured(lambda: ops.head_aggregate(g, wh, v, coo=True,
                                                                               out=zs["new_coo_weights"])),
                    "agg_composed": captured(composed),
                    "k1_plain_width_att": captured(lambda: ops.spmm_rhs(g, w_mean, v, rhs=False, out=zfull)),
                }
                if not uniform:  # producer + aggregation of either route
                    graphs["route_csr_weights"] = captured(lambda: ops.head_aggregate(
                        g, ops.head_weights(g, ns1, m1, rl1, norm_idx), v, out=zs["route_csr"]))
                    graphs["route_coo_through_perm"] = captured(lambda: ops.head_aggregate(
                        g, ops.edge_attention(g, ns1, m1, rl1, norm_idx), v, coo=True, out=zs["route_perm"]))
                dev_ab = float((zs["new"] - zs["composed"]).abs().max() / zs["composed"].abs().max())
                routes_equal = bool(torch.equal(zs["new"], zs["new_coo_weights"]))
                if not uniform:
                    routes_equal = routes_equal and bool(torch.equal(zs["route_csr"], zs["route_perm"]))
                t = {k: stats(vv) for k, vv in alternate(graphs, a.rounds, a.reps).items()}
                # a fixed-grid stage (k_i stored, the next stage input y0 + c1 k1 + c2 k2 + cf f): fused
                # into the product against f + the stage pass
                z = zs["new"].clone()
                sb = {k: torch.randn(x.shape, generator=gen, device=dev) for k in ("y0", "k1", "k2", "ki", "out")}
                stage = ops.Stage(f_out=sb["ki"], outs=[(sb["out"], sb["y0"], 1.0, 0.125,
                                                         [(sb["k1"], 0.25), (sb["k2"], -0.5)])])
                ftmp = torch.empty_like(x)
                kw = dict(x0=x0, alpha=alpha, beta=beta, add_source=True, bias=bo)

                def stage_unfused():
                    ops.linear_rhs(z, Wo, x, out=ftmp.view(-1, C), **kw)
                    ops.stage_apply(stage, ftmp, x, x)

                tg = {"fused": captured(lambda: ops.linear_rhs(z, Wo, x, stage=stage, **kw))}
                fused_out = sb["out"].clone()
                tg["f_then_stage_apply"] = captured(stage_unfused)
                stage_equal = bool(torch.equal(fused_out, sb["out"]))
                tt = {k: stats(vv) for k, vv in alternate(tg, a.rounds, a.reps).items()}
                nbytes = agg_bytes(g.nnz, g.R, H, att)
                spread = spread_of(t, ("agg_new", "agg_composed"))
                case = {"heads": H, "attention_dim": att, "dk": dk, "norm_idx": norm_idx, "uniform": uniform,
                        "new_vs_composed_rel": dev_ab, "outputs_agree": dev_ab <= 1e-6,
                        "weight_routes_bitwise_equal": routes_equal, "ms": t,
                        "agg_bytes": nbytes,
                        "agg_new_bytes_per_s": round(nbytes / (t["agg_new"]["median"] * 1e-3)),
                        "agg_new_fraction_of_hbm_peak": round(nbytes / (t["agg_new"]["median"] * 1e-3) / HBM_PEAK, 4),
                        "spread_ms": round(spread, 5),
                        "new_minus_composed_ms": round(t["agg_new"]["median"] - t["agg_composed"]["median"], 5),
                        "rk_stage_ms": tt, "rk_stage_bitwise_equal": stage_equal}
                case["within_bar"] = case["new_minus_composed_ms"] <= spread
                if not uniform:
                    case["route_csr_minus_perm_ms"] = round(t["route_csr_weights"]["median"] -
                                                            t["route_coo_through_perm"]["median"], 5)
                res["cases"].append(case)
                print("heads=%d att=%d norm_idx=%d: RHS %.4f ms; aggregation new %.4f ms (COO weights via perm %.4f), "
                      "composed %.4f ms, plain K1 at width att %.4f ms (spread %.4f ms, within bar %s, %.1f %% of "
                      "HBM peak); rk stage: fused %.4f ms, f + stage_apply %.4f ms (bitwise equal %s); new vs "
                      "composed %.2e" % (H, att, norm_idx, t["rhs_new"]["median"], t["agg_new"]["median"],
                                         t["agg_new_coo_weights"]["median"], t["agg_composed"]["median"],
                                         t["k1_plain_width_att"]["median"], spread, case["within_bar"],
                                         100 * case["agg_new_fraction_of_hbm_peak"], tt["fused"]["median"],
                                         tt["f_then_stage_apply"]["median"], stage_equal, dev_ab), flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
