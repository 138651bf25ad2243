#!/usr/bin/env python
"""The short-row phase of the headline K1 launch, measured on its own.

On the bench graph (G-arxiv, C = 128 fp32) in the solve's node numbering: recount the
row-length table on the device graph, find short_begin (the first item of the plan's
length classes 0 and 1, at most 3 edges) and time the fused-stage K1 (the stage-2
epilogue of the rk4 step) over
  (a) the whole plan,
  (b) items[:short_begin] with the hub table,
  (c) items[short_begin:] with no hub table,
  (d) the items of at most one edge alone
— ordinary launches on sub-lists of a valid plan; each writes the rows it owns.
HIP events, 20 launches after 3 warm-up launches, the median of three windows.
Prints one JSON object (--out FILE also writes it)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

import gnpde  # noqa: E402
from gnpde import ops, synthetic  # noqa: E402


def time_us(fn, reps=20, warm=3, windows=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    wins = []
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(windows):
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        torch.cuda.synchronize()
        wins.append(s.elapsed_time(e) / reps * 1e3)
    return sorted(wins)[len(wins) // 2]


def sub_plan(plan, lo, hi, heavy):
    """The plan's items [lo, hi) as a plan of their own (a view: nothing is copied)."""
    return ops.Plan(plan.items[lo * 4:], plan.heavy, hi - lo, plan.n_heavy if heavy else 0, plan.n_slots, plan.chunk)


def stage_bytes(n_rows, n_edges, C):
    """Algorithmic bytes of the stage-2 launch over n_rows rows with n_edges edges: the gathers,
    the own row, the base and one operand read, one output row written, the plan and the CSR."""
    return 4 * C * (n_edges + 4 * n_rows) + 16 * n_rows + 8 * n_edges


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    N, E, C = synthetic.ARXIV_N, synthetic.ARXIV_E, 128
    dev = torch.device("cuda", 0)
    ei, w = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    opt = {'hidden_dim': C, 'block': 'constant', 'add_source': False, 'no_alpha_sigmoid': False, 'max_nfe': 10 ** 9,
           'multi_modal': False}
    func = gnpde.LaplacianODEFunc(C, C, opt, dev).to(dev)
    func.edge_index, func.edge_weight = ei, w
    res = {"N": N, "E": E, "C": C, "library": gnpde.build_info()["library"]}
    with torch.no_grad():
        g = func.graph_for(x)
        lay = func.node_layout(x)
        gp, y0 = (lay.graph, lay.to_internal(x)) if lay is not None else (g, x)
        wc = func.csr_weights(gp, w, 'w')
        alpha = func.alpha_train.detach()
        plan = gp.csr.plan
        it = plan.items[:plan.n_items * 4].view(-1, 4).cpu()
        ln = (it[:, 2] - it[:, 1])
        short = ln <= 3
        short_begin = int(torch.nonzero(short)[0]) if bool(short.any()) else plan.n_items
        one_begin = int(torch.nonzero(ln <= 1)[0]) if bool((ln <= 1).any()) else plan.n_items
        assert bool(short[short_begin:].all()) and bool((ln[one_begin:] <= 1).all()), "items are not in class order"
        assert bool((it[short_begin:, 3] < 0).all()), "a hub chunk lies behind short_begin"
        rows = it[it[:, 3] < 0]
        rl = rows[:, 2] - rows[:, 1]
        nrows, nedges = int(rows.shape[0]), int(rl.sum())
        res["table"] = [{"max_len": k, "rows": int((rl <= k).sum()), "row_share": round(float((rl <= k).sum()) / nrows, 4),
                         "edge_share": round(float(rl[rl <= k].sum()) / nedges, 4)} for k in (1, 2, 3)]
        res.update(n_items=plan.n_items, n_heavy=plan.n_heavy, short_begin=short_begin, one_begin=one_begin)
        x2, x3 = torch.randn_like(y0), torch.empty_like(y0)
        parts = {"a": (0, plan.n_items, True), "b": (0, short_begin, True), "c": (short_begin, plan.n_items, False),
                 "d": (one_begin, plan.n_items, False)}
        full = gp.csr.plan
        try:
            for name, (lo, hi, heavy) in parts.items():
                gp.csr.plan = sub_plan(full, lo, hi, heavy)
                st = ops.Stage(outs=[(x3, x2, -1.0, 0.005, [(y0, 2.0)])])
                t = time_us(lambda: ops.spmm_rhs(gp, wc, x2, alpha=alpha, stage=st))
                sel = it[lo:hi]
                nr = int((sel[:, 3] < 0).sum()) if name != "b" else nrows - (plan.n_items - short_begin)
                ne = int((sel[:, 2] - sel[:, 1]).sum())
                res["t_" + name + "_us"] = round(t, 2)
                res["bytes_" + name] = stage_bytes(nr, ne, C)
        finally:
            gp.csr.plan = full
    res["t_c_over_t_a"] = round(res["t_c_us"] / res["t_a_us"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
