#!/usr/bin/env python
"""Golden-vector generator for the ODE regularisers (opt['gnpde_regularization']).

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference tree through
gen_golden.py); nothing under tests/ imports it.  It loads gen_golden.py as a module for its
stand-ins, BASE_OPT and random_graph.

The fixtures hold, for the reference's own ``LaplacianODEFunc`` (src/function_laplacian_diffusion.py)
in float64 on small seeded inputs (generated in float32 and up-cast):

  * ``f``           the RHS;
  * ``kinetic``     the reference's ``quadratic_cost(x, t, f, None)`` (src/regularized_ODE_function.py:66-69);
  * ``directional`` the reference's ``total_derivative(x, t, f + 0*t, None)`` (:36-54): its own
    ``directional_derivative`` (:57-63) raises for any shape (``.view(x.size(0), x.size(1) -1)``), and
    ``total_derivative`` computes the same directional term plus the partial time derivative,
    which is exactly 0 for f + 0*t.

Graphs: B in {1, 2}, duplicate edges, self loops and isolated rows (gen_golden.random_graph).
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "reg")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
import regularized_ODE_function as ref_reg  # noqa: E402  (the reference's, on gen_golden's sys.path entry)

f32 = gg.f32


def run(name, seed, B, N, E, C, add_source, no_alpha_sigmoid, alpha, beta):
    rng = np.random.default_rng(seed)
    opt = dict(gg.BASE_OPT, hidden_dim=C, block='constant', add_source=add_source,
               no_alpha_sigmoid=no_alpha_sigmoid)
    ei = gg.random_graph(rng, B, N, E, dup_frac=0.1, n_isolated=2)
    x = f32(rng.standard_normal((B, N, C)))
    x0 = f32(rng.standard_normal((B, N, C)))
    w = f32(rng.uniform(0.05, 1.0, (B, E)))
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    dt = torch.float64
    func = gg.ref_lap.LaplacianODEFunc(C, C, opt, 'cpu').to(dt)
    with torch.no_grad():
        func.alpha_train.fill_(alpha)
        func.beta_train.fill_(beta)
    func.edge_index = torch.from_numpy(ei)
    func.edge_weight = torch.from_numpy(w).to(dt)
    func.x0 = torch.from_numpy(x0).to(dt)
    xt = torch.from_numpy(x).to(dt).requires_grad_(True)
    t = torch.tensor(0.0, dtype=dt, requires_grad=True)
    f = func(t, xt)
    kinetic = ref_reg.quadratic_cost(xt, t, f, None)
    directional = ref_reg.total_derivative(xt, t, f + 0 * t, None)
    meta = dict(kind='reg', B=B, N=N, E=E, C=C, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid)
    os.makedirs(OUT_DIR, exist_ok=True)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0,
                        weights=w, alpha_train=f32(alpha), beta_train=f32(beta), f=f.detach().numpy(),
                        kinetic=kinetic.detach().numpy(), directional=directional.detach().numpy())
    return name


def main():
    names = [
        run('reg_b1_c5', 11, 1, 23, 90, 5, False, False, 0.3, 0.7),
        run('reg_b2_c12_src', 12, 2, 17, 70, 12, True, False, -0.4, 0.6),
        run('reg_b2_c7_noalpha', 13, 2, 19, 60, 7, True, True, 0.8, -0.3),
    ]
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump({'generator': 'tests/golden/gen_golden_reg.py', 'files': [n + '.npz' for n in names]}, fh,
                  indent=1)
        fh.write('\n')
    print('\n'.join(names))


if __name__ == '__main__':
    main()
