#!/usr/bin/env python
"""The ODE regularisers' passes and training steps at G-arxiv shape (169,343 x 128, fp32), in ONE
process:

  (a) gnpde_row_energy_f32 over 4 arrays (into the fp64 row accumulator, accumulating) against
      gnpde_rk_combine_f32 reading 4 arrays, and gnpde_row_axpy_f32 with a base and 2 terms (3
      arrays read) against gnpde_rk_combine_f32 reading 3: each a single launch replayed from a
      captured graph between HIP events, the kernels alternating inside every round, medians over
      the rounds; achieved bytes/s = the bytes the pass must move (computed from shapes) over that
      time.  The bars: each row pass reaches at least 0.9 of its rk_combine's bytes/s.
  (b) ms per rk4 step of a training step (forward plus backward of a 4-step solve, wall clock over
      the solve divided by 4; ConstantODEblock over the Laplacian RHS) of: the unregularised fused solve; kinetic_energy only; kinetic_energy +
      directional_penalty on the fused path; the same on the per-RHS path — the four alternating,
      medians with the spread, and each one's ratio to the unregularised step.

Prints one JSON document (--out FILE also writes it).  No GPU: it fails (nothing to measure)."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-neural-pde_amd"))
import torch  # noqa: E402

import gnpde  # noqa: E402
from gnpde import integrator as gi, ops, synthetic  # noqa: E402
from gnpde import regularized_ODE_function as R  # noqa: E402

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 128, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'rk4', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': False, 'max_nfe': 10 ** 9,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16,
       'gnpde_regularization': True}


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
    for _ in range(5):
        cg.replay()
    s.record()
    for _ in range(reps):
        cg.replay()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def stats(v):
    return {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def kernels(a, dev, N, C):
    n = N * C
    gen = torch.Generator(device=dev)
    gen.manual_seed(3)
    arr = lambda: torch.randn(N, C, generator=gen, device=dev)  # noqa: E731
    ks = [arr() for _ in range(4)]
    base, out = arr(), torch.empty(N, C, device=dev)
    acc = torch.zeros(N, dtype=torch.float64, device=dev)
    g0, g1 = torch.randn(N, generator=gen, device=dev), torch.randn(N, generator=gen, device=dev)
    cs = [0.125, 0.375, 0.375, 0.125]
    runs = {
        "row_energy_4": captured(lambda: ops.row_energy(ks, cs, acc=acc, accumulate=True)),
        "rk_combine_read4": captured(lambda: ops.rk_combine(None, ks, cs, 0.25, out=out)),
        "row_axpy_2": captured(lambda: ops.row_axpy(base, [(0.5, g0, ks[0]), (0.25, g1, ks[1])], out=out)),
        "rk_combine_read3": captured(lambda: ops.rk_combine(base, ks[:2], cs[:2], 0.25, out=out)),
    }
    # bytes each pass must move: arrays read and written (4 n each) and the per-row vectors
    nbytes = {"row_energy_4": 4 * 4 * n + 2 * 8 * N, "rk_combine_read4": 5 * 4 * n,
              "row_axpy_2": 4 * 4 * n + 2 * 4 * N, "rk_combine_read3": 4 * 4 * n}
    names = list(runs)
    t = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            t[k].append(replay_ms(runs[k], a.reps))
    res = {}
    for k in names:
        st = stats(t[k])
        res[k] = {"ms": st, "bytes": nbytes[k], "bytes_per_s": round(nbytes[k] / (st["median"] * 1e-3), 0)}
    for k, ref in (("row_energy_4", "rk_combine_read4"), ("row_axpy_2", "rk_combine_read3")):
        ratio = res[k]["bytes_per_s"] / res[ref]["bytes_per_s"]
        res["bar_" + k] = {"over_rk_combine_bytes_per_s": round(ratio, 4), "bar": 0.9, "met": ratio >= 0.9}
    return res


def steps(a, dev, N, E, C):
    ei, w = synthetic.rw_graph(N, E, seed=0, device=dev)
    x = synthetic.features(1, N, C, seed=1, device=dev)
    n_steps, dt = 4, 0.25
    cases = {
        "unregularised_fused": ((), True),
        "kinetic_fused": ((R.quadratic_cost,), True),
        "kinetic_directional_fused": ((R.quadratic_cost, R.directional_derivative), True),
        "kinetic_directional_per_rhs": ((R.quadratic_cost, R.directional_derivative), False),
    }
    blocks, info = {}, {}
    for k, (fns, fused) in cases.items():
        blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, list(fns), dict(OPT, hidden_dim=C, step_size=dt), dev,
                                     t=torch.tensor([0.0, dt * n_steps])).to(dev).train()
        blk.odefunc.edge_index, blk.odefunc.edge_weight = ei, w
        blocks[k] = blk

    def run(k):
        fns, fused = cases[k]
        blk = blocks[k]
        blk.odefunc.nfe = 0
        keep = gi.FUSED_BACKWARD
        gi.FUSED_BACKWARD = fused
        try:
            xin = x.detach().requires_grad_(True)
            out = blk(xin, None)
            if fns:
                z, regs = out
                loss = z.sum() + sum(r.mean() for r in regs)
            else:
                loss = out.sum()
            blk.zero_grad()
            loss.backward()
        finally:
            gi.FUSED_BACKWARD = keep
        return xin.grad

    for k in cases:
        for _ in range(2):
            g = run(k)
        torch.cuda.synchronize()
        info[k] = {"path": gi.odeint.last_reg_path if cases[k][0] else "fused (unregularised)",
                   "finite": bool(torch.isfinite(g).all())}
    names = list(cases)
    tm = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.solves):
                run(k)
            torch.cuda.synchronize()
            tm[k].append((time.perf_counter() - t0) * 1e3 / (a.solves * n_steps))
    res = {k: dict(stats(tm[k]), **info[k]) for k in names}
    base = res["unregularised_fused"]["median"]
    for k in names:
        res[k]["ratio_to_unregularised"] = round(res[k]["median"] / base, 3)
    return {"method": "rk4", "steps": n_steps, "dt": dt, "ms_per_training_step": res}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--solves", type=int, default=3)
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("reg_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("reg_bench: no GPU; nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"device": torch.cuda.get_device_name(dev), "shape": [a.nodes, a.width], "rounds": a.rounds, "reps": a.reps,
           "kernels": kernels(a, dev, a.nodes, a.width), "training_steps": steps(a, dev, a.nodes, a.edges, a.width)}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
