#!/usr/bin/env python
"""Golden-vector generator for the Laplacian ODE function's multi_modal branch.

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference
tree through gen_golden.py); nothing under tests/ imports it.  It loads
gen_golden.py as a module for its stand-ins, BASE_OPT, random_graph and _grads.

The reference cannot run the branch: its constructor calls an ``init_weights`` the
Laplacian class does not define (:33) and its forward calls ``torch.nn.softmax`` (:63), a
name torch does not have.  The fixtures therefore build the reference's own
``LaplacianODEFunc`` with ``multi_modal=False``, attach ``Q2`` / ``K2`` / ``V2``
(``nn.Linear`` of the shapes of :32-36), restate line :63 with ``torch.softmax(dim=-1)``
(as the transformer layer's multi_modal branch spells it, :171),

    x~ = matmul(softmax(matmul(Q2(x), K2(y).transpose(-2, -1) / sqrt(dk)), dim=-1), V2(y)),

and feed x~ to the reference's own ``forward`` (the COO -> to_dense aggregation and the
epilogue of :65-77).  Float64, plus a float32 run stored as ``f_ref32``.

Outputs: inputs + f (x~ as ``xt`` in the small fixture only; x0 = 0 without add_source) to
``tests/golden/multimodal/mm_*.npz`` and fp64 autograd gradients of <gout, f> w.r.t. x, y,
alpha_train, beta_train and the three projections to ``mmgrad_*.npz``, with a
MANIFEST.json; each file under 100 KB (which is what bounds the row counts: B*N = 70 rows
of C = 48 with their fp64 and fp32 results come to about 90 KB).

Draws: weights and biases ~ N(0, 0.3^2), unit-variance x / y (and one sharp-softmax case,
weights ~ N(0, 1) with x scaled by 3: scores of a standard deviation of tens, meta
``score_std``).  Every
fixture is redrawn until its float32 run is within 5e-6 of the float64 one (max error
over max reference): half of the bar the device path is held to.
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "multimodal")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
ref_lap = gg.ref_lap

f32 = gg.f32
REF32_CAP = 5e-6
MAX_BYTES = 100 * 1000
PNAMES = ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv')


def _opt(C, D2, add_source, no_alpha_sigmoid):
    return dict(gg.BASE_OPT, hidden_dim=C, block='constant', function='laplacian', add_source=add_source,
                no_alpha_sigmoid=no_alpha_sigmoid, multi_modal=False, second_modality_dim=D2)


def _func(opt, C, D2, dt, P, ei, w, x0):
    func = ref_lap.LaplacianODEFunc(C, C, opt, 'cpu')
    func.Q2 = torch.nn.Linear(C, C)        # :32, :34, :36
    func.V2 = torch.nn.Linear(D2, C)
    func.K2 = torch.nn.Linear(D2, C)
    func = func.to(dt)
    with torch.no_grad():
        func.alpha_train.fill_(P['alpha'])
        func.beta_train.fill_(P['beta'])
        for n, t in _params(func).items():
            t.copy_(torch.from_numpy(P[n]))
    func.edge_index = torch.from_numpy(ei)
    func.edge_weight = torch.from_numpy(w).to(dt)
    func.x0 = torch.from_numpy(x0).to(dt)
    return func


def _params(func):
    return dict(Wq=func.Q2.weight, bq=func.Q2.bias, Wk=func.K2.weight, bk=func.K2.bias, Wv=func.V2.weight,
                bv=func.V2.bias)


def _xtilde(func, x, y):
    """:62-63 with torch.softmax(..., dim=-1)."""
    dk = func.in_features
    return torch.matmul(torch.softmax(torch.matmul(func.Q2(x), func.K2(y).transpose(-2, -1) / np.sqrt(dk)), dim=-1),
                        func.V2(y))


def _forward(func, x, y):
    xt = _xtilde(func, x, y)
    return func(torch.tensor(0.0), xt), xt


def _draw(rng, B, N, E, C, M, D2, wstd, xscale, add_source, gkw):
    ei = gg.random_graph(rng, B, N, E, **gkw)
    w = f32(rng.uniform(0.05, 1.0, (B, E)))
    x = f32(rng.standard_normal((B, N, C)) * xscale)
    y = f32(rng.standard_normal((B, M, D2)))
    x0 = f32(rng.standard_normal((B, N, C))) if add_source else np.zeros((B, N, C), np.float32)
    P = dict(Wq=f32(rng.standard_normal((C, C)) * wstd), bq=f32(rng.standard_normal((C,)) * wstd),
             Wk=f32(rng.standard_normal((C, D2)) * wstd), bk=f32(rng.standard_normal((C,)) * wstd),
             Wv=f32(rng.standard_normal((C, D2)) * wstd), bv=f32(rng.standard_normal((C,)) * wstd))
    return ei, w, x, y, x0, P


def _runs(opt, C, D2, P, ei, w, x, y, x0):
    out = {}
    for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
        func = _func(opt, C, D2, dt, P, ei, w, x0)
        with torch.no_grad():
            f, xt = _forward(func, torch.from_numpy(x).to(dt), torch.from_numpy(y).to(dt))
        out['f' + tag], out['xt' + tag] = f.numpy(), xt.numpy()
    dev = float(np.abs(out['f_ref32'].astype(np.float64) - out['f']).max() / np.abs(out['f']).max())
    return out, dev


def _save(name, **arrays):
    path = os.path.join(OUT_DIR, name + '.npz')
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, (name, size)
    return size


def run_mm(name, rng, B, N, E, C, M, D2, add_source=False, no_alpha_sigmoid=False, alpha=0.3, beta=0.7, wstd=0.3,
           xscale=1.0, grad=False, store_xt=False, **gkw):
    opt = _opt(C, D2, add_source, no_alpha_sigmoid)
    draws = 0
    while True:
        draws += 1
        ei, w, x, y, x0, P = _draw(rng, B, N, E, C, M, D2, wstd, xscale, add_source, gkw)
        gout = f32(rng.standard_normal((B, N, C)))
        P.update(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
        out, dev = _runs(opt, C, D2, P, ei, w, x, y, x0)
        if dev <= REF32_CAP:
            break
        assert draws < 50, name
    s = (np.einsum('bnc,bmc->bnm', x.astype(np.float64) @ P['Wq'].T.astype(np.float64) + P['bq'],
                   y.astype(np.float64) @ P['Wk'].T.astype(np.float64) + P['bk']) / np.sqrt(C))
    meta = dict(kind='multimodal_grad' if grad else 'multimodal', B=B, N=N, E=int(ei.shape[2]), C=C, M=M, D2=D2,
                add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid, multi_modal=True, wstd=wstd, xscale=xscale,
                ref32_dev=dev, draws=draws, score_std=float(s.std()))
    arrays = dict(meta=json.dumps(meta), edge_index=ei, edge_weight=w, x=x, y=y, x0=x0, alpha_train=f32(P['alpha']),
                  beta_train=f32(P['beta']), f=out['f'], f_ref32=out['f_ref32'], **{n: P[n] for n in PNAMES})
    if grad:
        func = _func(opt, C, D2, torch.float64, P, ei, w, x0)
        xt_ = torch.from_numpy(x).double().requires_grad_(True)
        yt_ = torch.from_numpy(y).double().requires_grad_(True)
        go = torch.from_numpy(gout).double()
        named = [('x', xt_), ('y', yt_), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train)] + \
            list(_params(func).items())
        g = gg._grads(lambda: (_forward(func, xt_, yt_)[0] * go).sum(), named)
        assert all(g['g_' + n].any() for n in ('x', 'y') + PNAMES), name
        arrays.update(gout=gout, **g)
    elif store_xt:
        arrays.update(xt=out['xt'])
    size = _save(name, **arrays)
    print('%-22s %6d bytes, fp32 run deviates %.2e from fp64 (draw %d), score std %.1f'
          % (name, size, dev, draws, meta['score_std']))
    return name


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20261021)
    made = []
    # B*N = 70 rows, C = 48, M = 45, D2 = 20: add_source off / on, and no_alpha_sigmoid on one graph of 70 nodes
    made.append(run_mm('mm_b2_c48', rng, 2, 35, 160, 48, 45, 20))
    made.append(run_mm('mm_b2_c48_src', rng, 2, 35, 160, 48, 45, 20, add_source=True))
    made.append(run_mm('mm_n70_c48_noalpha', rng, 1, 70, 320, 48, 45, 20, add_source=True, no_alpha_sigmoid=True,
                       alpha=0.8, beta=-0.3))
    # a sharp softmax: N(0, 1) weights, x scaled by 3
    made.append(run_mm('mm_c20_sharp', rng, 1, 40, 180, 20, 17, 12, wstd=1.0, xscale=3.0, store_xt=True))
    made.append(run_mm('mmgrad_b2_src', rng, 2, 24, 110, 20, 17, 12, add_source=True, grad=True))
    made.append(run_mm('mmgrad_noalpha', rng, 1, 33, 150, 12, 9, 7, no_alpha_sigmoid=True, alpha=0.8, beta=-0.3,
                       grad=True))
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump(sorted(made), fh, indent=1)
    print('wrote', len(made), 'fixtures to', OUT_DIR)


if __name__ == '__main__':
    main()
