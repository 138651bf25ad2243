#!/usr/bin/env python
"""Golden-vector generator for the GAT attention ODE function.

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference
tree through gen_golden.py); nothing under tests/ imports it.  It loads
gen_golden.py as a module for its stand-ins, BASE_OPT, random_graph and _grads,
imports the reference's own

  * src/function_GAT_attention.py (ODEFuncAtt :9-71, SpGraphAttentionLayer :74-139)

and runs it on small seeded inputs in float64 (plus a float32 run stored as
``f_ref32`` / ``attention_ref32``), writing inputs + outputs to
``tests/golden/gat/gat_*.npz`` and fp64 autograd gradients to
``tests/golden/gat/gatgrad_*.npz`` (a directory of its own with its own MANIFEST.json:
tests/golden/MANIFEST.json lists the fixtures of tests/golden/ itself).
The gradients differentiate the reference layer's own forward (:117-136) and the dense product of multiply_attention (:40-47) built with
index_put: the installed torch's backward of ``sparse.permute(0, 3, 1, 2).to_dense()``
(:46-47) returns wrong values, so ODEFuncAtt's own autograd is not the derivative of its
forward (grad_gat.forward; ``g_x_ref_autograd`` and meta ``ref_autograd_dev_x`` keep the
evidence; tests/test_gat_oracle_golden.py checks the stored gradients against central
differences).  Inputs are generated in float32 and up-cast.
W ~ N(0, 0.3^2), a ~ N(0, 0.5^2) (the layer's xavier draws are replaced so the
values are reproducible from the file).  Gradient fixtures are redrawn until
every LeakyReLU pre-activation |sl[src,h] + sr[dst,h]| >= 1e-4 (the minimum is
stored in meta): the kink stays away from central differences and fp32 sign flips.
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "gat")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
import function_GAT_attention as ref_gat  # noqa: E402  (gen_golden put the reference on sys.path)

f32 = gg.f32
KINK_MIN = 1e-4


def _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope):
    return dict(gg.BASE_OPT, hidden_dim=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
                add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid, function='GAT', leaky_relu_slope=slope)


def _func(opt, C, dt, W, a, alpha, beta, ei, x0):
    func = ref_gat.ODEFuncAtt(C, C, opt, 'cpu').to(dt)
    lay = func.multihead_att_layer
    # nn.Parameter(...).to('cpu') (:97-103) is the Parameter itself: registered, converted by .to(dt)
    assert all(isinstance(p, torch.nn.Parameter) and p.dtype == dt for p in (lay.W, lay.a, lay.Wout))
    with torch.no_grad():
        lay.W.copy_(torch.from_numpy(W))
        lay.a.copy_(torch.from_numpy(a).reshape(1, -1, 1, 1))
        func.alpha_train.fill_(alpha)
        func.beta_train.fill_(beta)
    func.edge_index = torch.from_numpy(ei)
    func.x0 = torch.from_numpy(x0).to(dt)
    func.y = None
    return func, lay


def _preact(x, W, a, ei, heads):
    """sl[src,h] + sr[dst,h] in fp64 [B,E,h] (the LeakyReLU pre-activation)."""
    B, N, C = x.shape
    dk = W.shape[1] // heads
    wx = (x.astype(np.float64) @ W.astype(np.float64)).reshape(B, N, heads, dk)
    sl = wx @ a[:dk].astype(np.float64)
    sr = wx @ a[dk:].astype(np.float64)
    b = np.arange(B)[:, None]
    return sl[b, ei[:, 0]] + sr[b, ei[:, 1]]


def run_gat(name, rng, B, N, E, C, heads, att_dim, norm_idx, add_source=False, no_alpha_sigmoid=False, alpha=0.2,
            beta=0.5, slope=0.2, ei=None, pre_max=None, **gkw):
    opt = _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope)
    if ei is None:
        ei = gg.random_graph(rng, B, N, E, **gkw)
    x = f32(rng.standard_normal((B, N, C)))
    x0 = f32(rng.standard_normal((B, N, C)))
    W = f32(rng.standard_normal((C, att_dim)) * 0.3)
    a = f32(rng.standard_normal((2 * (att_dim // heads),)) * 0.5)
    if pre_max is not None:  # W scaled so that max |pre-activation| is about pre_max
        W = f32(W * (pre_max / np.abs(_preact(x, W, a, ei, heads)).max()))
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    out = {}
    for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
        func, lay = _func(opt, C, dt, W, a, alpha, beta, ei, x0)
        xt = torch.from_numpy(x).to(dt)
        with torch.no_grad():
            att, _ = lay(xt, func.edge_index, None)
            f = func(torch.tensor(0.0), xt)
        out['f' + tag] = f.numpy()
        out['attention' + tag] = att.numpy()
    pre = np.abs(_preact(x, W, a, ei, heads))
    meta = dict(kind='gat', B=B, N=N, E=int(ei.shape[2]), C=C, heads=heads, attention_dim=att_dim,
                attention_norm_idx=norm_idx, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid,
                leaky_relu_slope=slope, preact_max=float(pre.max()), preact_min=float(pre.min()))
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0, W=W,
                        a=a, alpha_train=f32(alpha), beta_train=f32(beta), f=out['f'], attention=out['attention'],
                        f_ref32=out['f_ref32'], attention_ref32=out['attention_ref32'])
    return name, ei


def grad_gat(name, rng, B, N, E, C, heads, att_dim, norm_idx, add_source=False, no_alpha_sigmoid=False, alpha=0.2,
             beta=0.5, slope=0.2, **gkw):
    """Gradients of <gout, f> through the reference ODEFuncAtt.forward w.r.t. x,
    alpha_train, beta_train, W and a (Wout gets none: dead for mix_features=False)."""
    opt = _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope)
    draws = 0
    while True:  # the kink condition: a condition on the inputs
        draws += 1
        ei = gg.random_graph(rng, B, N, E, **gkw)
        x = f32(rng.standard_normal((B, N, C)))
        x0 = f32(rng.standard_normal((B, N, C)))
        W = f32(rng.standard_normal((C, att_dim)) * 0.3)
        a = f32(rng.standard_normal((2 * (att_dim // heads),)) * 0.5)
        gout = f32(rng.standard_normal((B, N, C)))
        pre_min = float(np.abs(_preact(x, W, a, ei, heads)).min())
        if pre_min >= KINK_MIN:
            break
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    func, lay = _func(opt, C, torch.float64, W, a, alpha, beta, ei, x0)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    go = torch.from_numpy(gout).double()
    named = [('x', xt), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train), ('W', lay.W),
             ('a', lay.a), ('Wout', lay.Wout)]
    with torch.no_grad():
        f = func(torch.tensor(0.0), xt).numpy()
        att = lay(xt, func.edge_index, None)[0].numpy()

    def forward():
        """ODEFuncAtt.forward (:50-68) with the reference layer's own forward (:117-136)
        and multiply_attention's dense product (:40-47) built with index_put instead of
        sparse_coo_tensor(...).permute(0, 3, 1, 2).to_dense(): the same dense [B,h,N,N]
        tensor (duplicates summed), but differentiable — the installed torch's backward of
        a permuted sparse tensor's to_dense() returns wrong values (zeros for part of
        them, also for sorted duplicate-free indices), so the reference's own autograd is
        not the derivative of its forward there (g_x_ref_autograd keeps it as evidence)."""
        a_, _ = lay(xt, func.edge_index, None)
        eidx = func.edge_index
        bi = torch.arange(B)[:, None, None].expand(B, E, heads)
        hi = torch.arange(heads)[None, None, :].expand(B, E, heads)
        dense = torch.zeros(B, heads, N, N, dtype=torch.float64).index_put(
            (bi, hi, eidx[:, 0][:, :, None].expand(B, E, heads), eidx[:, 1][:, :, None].expand(B, E, heads)), a_,
            accumulate=True)
        ax = torch.mean(torch.matmul(dense, xt.unsqueeze(1)), dim=1)
        alpha_ = func.alpha_train if no_alpha_sigmoid else torch.sigmoid(func.alpha_train)
        out = alpha_ * (ax - xt)
        return out + func.beta_train * func.x0 if add_source else out

    with torch.no_grad():
        assert float((forward() - torch.from_numpy(f)).abs().max()) <= 1e-13 * max(1.0, float(np.abs(f).max()))
    g = gg._grads(lambda: (forward() * go).sum(), named)
    ref = gg._grads(lambda: (func(torch.tensor(0.0), xt) * go).sum(), named)
    assert not g['g_Wout'].any() and not ref['g_Wout'].any(), "Wout is dead for mix_features=False"
    del g['g_Wout']
    g['g_a'] = g['g_a'].reshape(-1)
    g['g_x_ref_autograd'] = ref['g_x']
    meta = dict(kind='gat_grad', B=B, N=N, E=E, C=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
                add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid, leaky_relu_slope=slope,
                preact_min=pre_min, draws=draws,
                ref_autograd_dev_x=float(np.abs(ref['g_x'] - g['g_x']).max() / np.abs(g['g_x']).max()))
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0, W=W,
                        a=a, alpha_train=f32(alpha), beta_train=f32(beta), f=f, attention=att, gout=gout, **g)
    return name


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20250921)
    made = []
    n, ei = run_gat('gat_n0_h2', rng, 1, 60, 320, 12, 2, 16, 0)
    made.append(n)
    made.append(run_gat('gat_n1_h2', rng, 1, 60, 320, 12, 2, 16, 1, ei=ei)[0])  # the same graph
    made.append(run_gat('gat_n1_h8_b2', rng, 2, 50, 240, 20, 8, 32, 1)[0])
    made.append(run_gat('gat_n0_h1_b3', rng, 3, 30, 100, 9, 1, 4, 0)[0])
    made.append(run_gat('gat_n0_h4_src', rng, 1, 70, 350, 16, 4, 16, 0, add_source=True, no_alpha_sigmoid=True,
                        alpha=0.8, beta=-0.3, slope=0.05)[0])
    made.append(run_gat('gat_n1_c128', rng, 1, 300, 2400, 128, 2, 32, 1, dup_frac=0.1, n_isolated=5)[0])
    made.append(run_gat('gat_n0_c128_h4', rng, 1, 300, 2400, 128, 4, 64, 0, dup_frac=0.1, n_isolated=5)[0])
    made.append(run_gat('gat_n0_c162', rng, 1, 150, 900, 162, 2, 32, 0)[0])
    made.append(run_gat('gat_n1_wide', rng, 1, 60, 320, 12, 2, 16, 1, pre_max=30.0)[0])
    made.append(grad_gat('gatgrad_n0_h2', rng, 1, 60, 320, 12, 2, 16, 0))
    made.append(grad_gat('gatgrad_n1_h2', rng, 1, 60, 320, 12, 2, 16, 1))
    made.append(grad_gat('gatgrad_n1_h8_b2', rng, 2, 40, 200, 16, 8, 32, 1))
    made.append(grad_gat('gatgrad_n0_src', rng, 1, 50, 260, 10, 2, 8, 0, add_source=True, no_alpha_sigmoid=True,
                         alpha=0.8, beta=-0.3))
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump(sorted(made), fh, indent=1)
    print('wrote', len(made), 'fixtures to', OUT_DIR)


if __name__ == '__main__':
    main()
