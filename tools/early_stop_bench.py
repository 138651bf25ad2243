#!/usr/bin/env python
"""The early-stop test integrator's score (gnpde_decode_score_f32, gnpde.early_stop_solver)
at ogbn-arxiv size (N = 169,343, state width 162, 40 classes, every node in a split) and at
Pubmed size (N = 19,717, width 128, 3 classes, the Planetoid split: 60 / 500 / 1,000 nodes),
in ONE process:

  (a) per scored state, the fused kernel (one launch into a slot of the device record, no
      host read) against the torch restatement the reference's evaluate / test amount to —
      relu, F.linear, max, three masked compares and sums, three .item() reads.  Both are
      timed as a solve meets them: the host enqueues one score behind a queued RHS launch
      and the clock runs until the device is idle (wall clock, medians over the rounds);
      the kernel and one Laplacian RHS evaluation on the same graph are also timed alone,
      replayed from captured graphs between HIP events;
  (b) the early-stop dopri5 solve (max_test_steps 100, interval [0, earlystopxT T]) against
      gnpde.odeint over the same interval, same tolerances: wall clock per solve, the two
      alternating, medians over the rounds.

No bar is set: nobody had measured either.  Prints one JSON document (--out FILE also
writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import gnpde  # noqa: E402
from gnpde import integrator as gi, ops, synthetic  # noqa: E402
from gnpde.early_stop_solver import EarlyStopInt  # noqa: E402

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 6, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'dopri5', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': False, 'max_nfe': 10 ** 9,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16}

# name -> nodes, edges (self loops included), width, classes, (train, val, test) sizes (None: all nodes, 54/18/28 %),
#         T, tol_scale (src/best_params.py), earlystopxT
SIZES = {
    "ogbn-arxiv": (synthetic.ARXIV_N, synthetic.ARXIV_E, 162, 40, None, 3.676, 11353.6, 3.0),
    "Pubmed": (19717, 19717 + 88648, 128, 3, (60, 500, 1000), 12.942, 1932.0, 5.0),
}


def captured(fn):
    fn()
    torch.cuda.synchronize()
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        fn()
    torch.cuda.synchronize()
    return cg


def replay_ms(cg, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(10):
        cg.replay()
    s.record()
    for _ in range(reps):
        cg.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def torch_score(y, W, b, data, Cd):
    """The reference's evaluate + test, as intended: about fifteen launches and three host reads."""
    z = y[..., :Cd] if Cd != y.shape[-1] else y
    z = F.linear(F.relu(z), W, b)
    pred = z.max(-1)[1]
    accs = []
    for mask in (data.train_mask, data.val_mask, data.test_mask):
        accs.append(pred[mask].eq(data.y[mask]).sum().item() / mask.sum().item())
    return accs


def case(name, a, dev):
    N, E, C, K, sizes, T, ts, xT = SIZES[name]
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    ei, w = synthetic.rw_graph(N, E, seed=0, device=dev)
    y = synthetic.features(1, N, C, seed=1, device=dev)
    W = torch.randn(K, C, generator=gen, device=dev) * 0.3
    b = torch.randn(K, generator=gen, device=dev) * 0.1
    perm = torch.randperm(N, generator=gen, device=dev)
    if sizes is None:
        sizes = (int(0.54 * N), int(0.18 * N), N - int(0.54 * N) - int(0.18 * N))
    masks, o = [], 0
    for n in sizes:
        m = torch.zeros(N, dtype=torch.bool, device=dev)
        m[perm[o:o + n]] = True
        masks.append(m.view(1, N))
        o += n
    data = types.SimpleNamespace(y=torch.randint(0, K, (1, N), generator=gen, device=dev), train_mask=masks[0],
                                 val_mask=masks[1], test_mask=masks[2])
    split, label, _ = ops.pack_splits(data, N, dev)
    rec = torch.zeros(128, 3, dtype=torch.int32, device=dev)
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C), dev).to(dev)
    func.edge_index, func.edge_weight = ei, w
    out = {"nodes": N, "edges": E, "width": C, "classes": K, "masked_rows": int(sum(sizes))}

    # the two scorers agree (the torch one through its accuracies)
    rec.zero_()
    ops.decode_score(y, W, b, split, label, rec[0])
    got = [c / n for c, n in zip(rec[0].tolist(), sizes)]
    want = torch_score(y, W, b, data, C)
    out["accuracies_kernel"], out["accuracies_torch"] = got, want
    out["max_accuracy_difference"] = max(abs(u - v) for u, v in zip(got, want))

    with torch.no_grad():
        f_buf = torch.empty_like(y)
        rhs = captured(lambda: func.rhs_stage(0.0, y, ops.Stage(f_out=f_buf)))
        kern = captured(lambda: ops.decode_score(y, W, b, split, label, rec[1]))

        def step_kernel():
            rhs.replay()
            ops.decode_score(y, W, b, split, label, rec[2])

        def step_torch():
            rhs.replay()
            torch_score(y, W, b, data, C)

        def step_none():
            rhs.replay()

        t = {k: [] for k in ("rhs_graph_ms", "score_kernel_graph_ms", "step_rhs_only_wall_ms",
                             "step_rhs_plus_kernel_wall_ms", "step_rhs_plus_torch_wall_ms")}
        for r in range(a.rounds):
            t["rhs_graph_ms"].append(replay_ms(rhs, a.reps))
            t["score_kernel_graph_ms"].append(replay_ms(kern, a.reps))
            order = [("step_rhs_only_wall_ms", step_none), ("step_rhs_plus_kernel_wall_ms", step_kernel),
                     ("step_rhs_plus_torch_wall_ms", step_torch)]
            for k, fn in order[r % 3:] + order[:r % 3]:
                t[k].append(wall_ms(fn, a.reps))
    out.update({k: stats(v) for k, v in t.items()})
    base = out["step_rhs_only_wall_ms"]["median"]
    out["score_cost_per_step_kernel_ms"] = round(out["step_rhs_plus_kernel_wall_ms"]["median"] - base, 5)
    out["score_cost_per_step_torch_ms"] = round(out["step_rhs_plus_torch_wall_ms"]["median"] - base, 5)
    out["score_kernel_over_rhs"] = round(out["score_kernel_graph_ms"]["median"] / out["rhs_graph_ms"]["median"], 3)

    # (b) the solves
    opt = dict(OPT, hidden_dim=C, method='dopri5', earlystopxT=xT, max_test_steps=100, tol_scale=ts)
    es = EarlyStopInt(T, opt, dev)
    es.data, es.m2_weight, es.m2_bias = data, W, b
    rtol, atol = ts * 1e-9, ts * 1e-7

    def solve_early():
        return es(func, y, None, rtol=rtol, atol=atol)

    def solve_plain():
        with torch.no_grad():
            return gnpde.odeint(func, y, es.t, rtol=rtol, atol=atol, method='dopri5')

    for _ in range(3):  # warm: captures the step graphs both share
        ze, zp = solve_early(), solve_plain()
    out["solve_bit_equal"] = bool(torch.equal(ze, zp))
    out["solve_steps"] = {"attempts": es.solver.n_attempts, "scored": len(es.solver.times), "path": gi.odeint.last_path,
                          "interval": [0.0, float(es.t[1])]}
    ts_ = {"solve_early_stop_ms": [], "solve_plain_ms": []}
    for r in range(a.rounds):
        pair = [("solve_early_stop_ms", solve_early), ("solve_plain_ms", solve_plain)]
        for k, fn in (pair if r % 2 == 0 else pair[::-1]):
            ts_[k].append(wall_ms(fn, a.solves))
    out.update({k: stats(v) for k, v in ts_.items()})
    n = max(len(es.solver.times), 1)
    out["solve_extra_per_scored_step_ms"] = round(
        (out["solve_early_stop_ms"]["median"] - out["solve_plain_ms"]["median"]) / n, 5)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--solves", type=int, default=5)
    p.add_argument("--cases", default="ogbn-arxiv,Pubmed")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("early_stop_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("early_stop_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"device": torch.cuda.get_device_name(dev), "rounds": a.rounds, "reps": a.reps, "solves": a.solves,
           "cases": {name: case(name, a, dev) for name in a.cases.split(",")}}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
