#!/usr/bin/env python
"""The multistep solvers' passes and steps at G-arxiv shape (169,343 x 128, fp32), in ONE process:

  (a) gnpde_adams_predict_f32 at H = 3, 6, 11 history arrays (explicit form: dy and x; and the
      implicit form with delta at H = 6), gnpde_adams_correct_f32, and gnpde_rk_combine_f32 at
      the operand count of predict H = 6 (y0 + 6 arrays): each a single launch replayed from a
      captured graph between HIP events, the kernels alternating inside every round, medians
      over the rounds; achieved bytes/s = the bytes the pass must move (arrays read + arrays
      written, 4 n each) over that time;
  (b) ms per step of whole solves on the G-arxiv graph (Laplacian RHS): explicit_adams at
      max_order 4 and 12, implicit_adams (with its mean corrector iterations per Adams step) and
      the fused rk4 solve, same step size and step count, wall clock around a synchronise, the
      four alternating, medians over the rounds.

The one bar: predict at H = 6 reaches at least 0.9 of rk_combine's bytes/s ("bar_predict_h6").
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
from gnpde import adams_coefficients as AC, integrator as gi, ops, synthetic  # noqa: E402

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 128, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'rk4', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': False, 'max_nfe': 10 ** 9,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16}


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
    arr = lambda: torch.randn(n, generator=gen, device=dev)  # noqa: E731
    hist = [arr() for _ in range(11)]
    y0, dy, x, delta, f = arr(), arr(), arr(), arr(), arr()
    out = torch.empty(n, device=dev)
    ws = ops.adams_workspace(dev)
    dt = 0.02
    runs, arrays = {}, {}
    for H in (3, 6, 11):
        cdy = [dt * c for c in AC.ADAMS_BASHFORTH[H]]
        runs["predict_h%d" % H] = captured(lambda H=H, cdy=cdy: ops.adams_predict(y0, hist[:H], cdy, dy, x))
        arrays["predict_h%d" % H] = H + 1 + 2
    cdy6 = [dt * c for c in AC.ADAMS_BASHFORTH[6]]
    cde6 = [dt * c for c in AC.ADAMS_MOULTON[7][1:]]
    runs["predict_h6_delta"] = captured(lambda: ops.adams_predict(y0, hist[:6], cdy6, dy, x, cdelta=cde6, delta=delta))
    arrays["predict_h6_delta"] = 6 + 1 + 3
    # rtol = atol = 0: the ratio is never < 1, so no launch of the replay is gated off
    runs["correct"] = captured(lambda: ops.adams_correct(f, delta, y0, dy, x, 0.3 * dt, 0.0, 0.0, ws))
    arrays["correct"] = 4 + 2
    runs["rk_combine_y0_6"] = captured(lambda: ops.rk_combine(y0, hist[:6], list(AC.ADAMS_BASHFORTH[6]), dt, out=out))
    arrays["rk_combine_y0_6"] = 6 + 1 + 1
    names = list(runs)
    t = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            t[k].append(replay_ms(runs[k], a.reps))
    res = {}
    for k in names:
        st = stats(t[k])
        nbytes = arrays[k] * 4 * n
        res[k] = {"ms": st, "arrays_moved": arrays[k], "bytes": nbytes,
                  "bytes_per_s": round(nbytes / (st["median"] * 1e-3), 0)}
    ratio = res["predict_h6"]["bytes_per_s"] / res["rk_combine_y0_6"]["bytes_per_s"]
    res["bar_predict_h6"] = {"predict_over_rk_combine_bytes_per_s": round(ratio, 4), "bar": 0.9, "met": ratio >= 0.9}
    return res


def solves(a, dev, N, E, C):
    ei, w = synthetic.rw_graph(N, E, seed=0, device=dev)
    y = synthetic.features(1, N, C, seed=1, device=dev)
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C), dev).to(dev)
    func.edge_index, func.edge_weight = ei, w
    dt, steps = a.dt, a.steps
    t = torch.tensor([0.0, dt * steps], device=dev)
    rtol, atol = 1e-7, 1e-5
    cases = {
        "explicit_adams_order4": ("explicit_adams", dict(gnpde_adams=True, step_size=dt, max_order=4)),
        "explicit_adams_order12": ("explicit_adams", dict(gnpde_adams=True, step_size=dt, max_order=12)),
        "implicit_adams_order12": ("implicit_adams", dict(gnpde_adams=True, step_size=dt, max_order=12, max_iters=4)),
        "rk4_fused": ("rk4", dict(step_size=dt)),
    }
    info = {}

    def run(k):
        method, opts = cases[k]
        with torch.no_grad():
            z = gi.odeint(func, y, t, rtol=rtol, atol=atol, method=method, options=opts)
        return z

    for k in cases:  # warm (rk4: captures its step graphs)
        for _ in range(2):
            z = run(k)
        torch.cuda.synchronize()
        info[k] = {"path": gi.odeint.last_path if k != "rk4_fused" else "fused rk4 (captured step graphs)",
                   "finite": bool(torch.isfinite(z[-1]).all()), "max_abs": float(z[-1].abs().max())}
        if k.startswith("implicit"):
            its = gi.odeint.last_adams['iterations']
            adams = [v for v in its if v]
            info[k]["mean_corrector_iterations"] = round(sum(adams) / max(len(adams), 1), 3)
            info[k]["all_converged"] = all(gi.odeint.last_adams['converged'])
    names = list(cases)
    tm = {k: [] for k in names}
    for r in range(a.rounds):
        for k in names[r % len(names):] + names[:r % len(names)]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.solves):
                run(k)
            torch.cuda.synchronize()
            tm[k].append((time.perf_counter() - t0) * 1e3 / (a.solves * steps))
    return {"dt": dt, "steps": steps, "rtol": rtol, "atol": atol,
            "ms_per_step": {k: dict(stats(tm[k]), **info[k]) for k in names}}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--solves", type=int, default=3)
    p.add_argument("--steps", type=int, default=32)
    p.add_argument("--dt", type=float, default=0.02)
    p.add_argument("--nodes", type=int, default=synthetic.ARXIV_N)
    p.add_argument("--edges", type=int, default=synthetic.ARXIV_E)
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.rounds < 9:
        raise SystemExit("adams_bench: medians of at least nine rounds")
    if not torch.cuda.is_available():
        raise SystemExit("adams_bench: no GPU; nothing is measured without one")
    warnings.simplefilter("ignore")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    doc = {"device": torch.cuda.get_device_name(dev), "shape": [a.nodes, a.width], "rounds": a.rounds, "reps": a.reps,
           "kernels": kernels(a, dev, a.nodes, a.width), "solves": solves(a, dev, a.nodes, a.edges, a.width)}
    txt = json.dumps(doc, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt + "\n")


if __name__ == "__main__":
    main()
