#!/usr/bin/env python
"""The beltrami exp_kernel RHS (opt['gnpde_beltrami_kernel']) beside plain exp_kernel at
attention_dim doubled, on the benchmark's G-arxiv graph (synthetic.rw_graph, N = 169,343,
E' = 1,200,000) at BLEND's C = 162 (F = 64, P = 98, attention_dim 32, heads 2), both
attention_norm_idx, in ONE process:

  (a) beltrami  ops.node_scores over the folded operand W' [4 att, C] (heads 2, dk' = 2 dk,
                p0 = ovx ovp, p1 = 1) + ops.attn_rhs;
  (b) plain     the same two calls with a dense [Wq; Wk] of the same shape (exp_kernel at
                attention_dim 2 att): the same launches, so the two should agree within the
                run-to-run spread.  The zero blocks of W' cost MFMA work and no bytes.

Each path is replayed from a captured graph and timed with HIP events, the paths
alternating and their order rotating every round; medians over the rounds (at least nine),
with the spread (max - min over the rounds).  Beside them one training step (forward +
backward of <gout, f>, eager, a device synchronise at the end) of the two layers — the
beltrami layer's backward runs gnpde_score_grad_split_f32, the plain layer's
gnpde_score_grad_f32 — and the two score-gradient kernels alone (both sides, with the
parameter terms, captured).  The folded RHS is first compared with the float64 formula on a
sample of edges' scores.  Prints one JSON document (--out FILE also writes it; default
profiles/beltrami_bench.json).  None of the numbers is a bar.  No GPU: it fails."""
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

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'add_source': False, 'block': 'constant',
       'function': 'transformer', 'augment': False, 'adjoint': False, 'tol_scale': 1, 'time': 1, 'method': 'rk4',
       'no_alpha_sigmoid': False, 'reweight_attention': False, 'step_size': 1, 'square_plus': False,
       'max_nfe': 10 ** 9, 'data_norm': 'rw', 'max_iters': 100, 'multi_modal': False, 'mix_features': False,
       'attention_type': 'exp_kernel'}


def captured(fn):
    fn()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        fn()
    torch.cuda.synchronize()
    return cg


def time_ms(run, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def alternate(runs, rounds, reps):
    """{name: [ms per round]}: every round times each path once, the order rotating."""
    names = list(runs)
    for r in runs.values():
        time_ms(r, max(2, reps // 5))
    t = {k: [] for k in names}
    for r in range(rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            t[k].append(time_ms(runs[k], reps))
    return t


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def compare(t, a, b):
    s = {k: stats(v) for k, v in t.items()}
    spread = max(s[k]["max"] - s[k]["min"] for k in (a, b))
    diff = s[a]["median"] - s[b]["median"]
    return dict(ms=s, spread_ms=round(spread, 5), diff_ms=round(diff, 5), within_spread=abs(diff) <= spread)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--feat", type=int, default=64)
    p.add_argument("--pos", type=int, default=98)
    p.add_argument("--att", type=int, default=32)
    p.add_argument("--heads", type=int, default=2)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--train-reps", type=int, default=3)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "beltrami_bench.json"))
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("beltrami_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("beltrami_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    N, E, F, P, att, H = a.nodes, a.edges, a.feat, a.pos, a.att, a.heads
    C = F + P
    ei, _ = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    gout = synthetic.features(1, N, C, seed=5, device=dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(2)
    res = {"graph": "G-arxiv" if (N, E) == (synthetic.ARXIV_N, synthetic.ARXIV_E) else "custom", "N": N,
           "E": int(ei.shape[2]), "C": C, "F": F, "P": P, "attention_dim": att, "heads": H, "rounds": a.rounds,
           "reps": a.reps, "train_reps": a.train_reps, "cases": []}
    for norm_idx in (0, 1):
        base = dict(OPT, hidden_dim=C, heads=H, attention_norm_idx=norm_idx)
        bel = gnpde.ODEFuncTransformerAtt(C, C, dict(base, attention_dim=att, beltrami=True, feat_hidden_dim=F,
                                                      pos_enc_hidden_dim=P, gnpde_beltrami_kernel=True), dev).to(dev)
        pla = gnpde.ODEFuncTransformerAtt(C, C, dict(base, attention_dim=2 * att, beltrami=False), dev).to(dev)
        lb, lp = bel.multihead_att_layer, pla.multihead_att_layer
        with torch.no_grad():
            for lin in (lb.Qx, lb.Kx, lb.Qp, lb.Kp, lp.Q, lp.K):
                w = lin.weight
                lin.weight.copy_(torch.randn(w.shape, generator=gen, device=dev) * (0.5 / w.shape[1] ** 0.5))
                lin.bias.copy_(torch.randn(w.shape[0], generator=gen, device=dev) * 0.1)
            for prm, v in ((lb.output_var_x, 1.6), (lb.lengthscale_x, 0.7), (lb.output_var_p, 1.5),
                           (lb.lengthscale_p, 1.9), (lp.output_var, 2.4), (lp.lengthscale, 1.0)):
                prm.fill_(v)
            for f in (bel, pla):
                f.alpha_train.fill_(0.3)
        bel.edge_index = pla.edge_index = ei
        g = bel.graph_for(x)
        pla.graph_for(x)
        alpha = torch.tensor(0.3, device=dev)
        fo = {k: torch.empty_like(x) for k in ("beltrami", "plain")}
        wb, wp = lb.wcat(), lp.wcat()
        assert wb[0].shape == wp[0].shape == (4 * att, C)
        pb, pp = lb._score_params(), lp._score_params()

        def rhs(wcat, p0, p1, out):
            ns = ops.node_scores(g, x, None, None, None, None, H, 'exp_kernel', 'reference', p0, p1, wcat=wcat)
            ops.attn_rhs(g, ns, None, None, norm_idx, x, alpha=alpha, out=out)
            return ns

        with torch.no_grad():
            # the folded scores against the float64 formula on a sample of edges
            ns = rhs(wb, pb[0], pb[1], fo["beltrami"])
            sel = torch.randint(0, int(ei.shape[2]), (4096,), generator=gen, device=dev)
            src, dst = ei[0, 0, sel], ei[0, 1, sel]
            xd = x[0].double()
            xf, xp = torch.cat([xd[:, :F], xd[:, F + P:]], 1), xd[:, F:F + P]

            def sq(Q, K, z):
                q = (z @ Q.weight.double().t() + Q.bias.double()).view(N, H, att // H)
                k = (z @ K.weight.double().t() + K.bias.double()).view(N, H, att // H)
                return ((q[src] - k[dst]) ** 2).sum(-1)
            want = 1.6 ** 2 * torch.exp(-sq(lb.Qx, lb.Kx, xf) / (2 * 0.7 ** 2)) * \
                1.5 ** 2 * torch.exp(-sq(lb.Qp, lb.Kp, xp) / (2 * 1.9 ** 2))
            d = (ns.q[src] - ns.k[dst]).double().view(-1, H, 2 * att // H)
            got = pb[0] ** 2 * torch.exp(-(d ** 2).sum(-1) / 2)
            score_err = float((got - want).abs().max() / want.abs().max())
            graphs = {"beltrami": captured(lambda: rhs(wb, pb[0], pb[1], fo["beltrami"])),
                      "plain": captured(lambda: rhs(wp, pp[0], pp[1], fo["plain"]))}
            t_rhs = compare(alternate({k: cg.replay for k, cg in graphs.items()}, a.rounds, a.reps), "beltrami",
                            "plain")

        def train(func):
            def run():
                for prm in func.parameters():
                    prm.grad = None
                xt = x.detach().requires_grad_(True)
                (func(None, xt) * gout).sum().backward()
            return run

        t_train = compare(alternate({"beltrami": train(bel), "plain": train(pla)}, a.rounds, a.train_reps),
                          "beltrami", "plain")
        with torch.no_grad():
            nsb = rhs(wb, pb[0], pb[1], fo["beltrami"])
            nsp = rhs(wp, pp[0], pp[1], fo["plain"])
            gs = torch.randn(1, int(ei.shape[2]), H, generator=gen, device=dev)

            def k_split():
                ops.score_grad_split(g.csr, 0, nsb, gs, att // H, with_params=True)
                ops.score_grad_split(g.csc, 1, nsb, gs, att // H)

            def k_plain():
                ops.score_grad(g.csr, 0, nsp, gs, with_params=True)
                ops.score_grad(g.csc, 1, nsp, gs)

            kg = {"split": captured(k_split), "plain": captured(k_plain)}
            t_kernel = compare(alternate({k: cg.replay for k, cg in kg.items()}, a.rounds, a.reps), "split", "plain")
        case = {"norm_idx": norm_idx, "folded_score_rel_err_vs_float64": score_err, "rhs": t_rhs,
                "training_step": t_train, "score_grad_both_sides": t_kernel}
        res["cases"].append(case)
        print("norm_idx=%d: RHS beltrami %.4f ms, plain exp_kernel at 2 att %.4f ms (spread %.4f ms, within %s); "
              "training step %.3f / %.3f ms (spread %.3f); score gradient, both sides: split %.4f ms, plain %.4f ms "
              "(spread %.4f); folded score vs float64 %.2e"
              % (norm_idx, t_rhs["ms"]["beltrami"]["median"], t_rhs["ms"]["plain"]["median"], t_rhs["spread_ms"],
                 t_rhs["within_spread"], t_train["ms"]["beltrami"]["median"], t_train["ms"]["plain"]["median"],
                 t_train["spread_ms"], t_kernel["ms"]["split"]["median"], t_kernel["ms"]["plain"]["median"],
                 t_kernel["spread_ms"], score_err), flush=True)
    doc = json.dumps(res, indent=1)
    print(doc)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(doc + "\n")


if __name__ == "__main__":
    main()
