#!/usr/bin/env python
"""Golden-vector generator for the GAT attention ODE function with mix_features.

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference
tree through gen_golden.py); nothing under tests/ imports it.  It loads
gen_golden.py as a module for its stand-ins, BASE_OPT, random_graph and _grads,
imports the reference's own

  * src/function_GAT_attention.py (ODEFuncAtt :9-71 with the mix_features branch of
    multiply_attention :29-38, SpGraphAttentionLayer :74-139)

and runs it with ``mix_features=True`` on small seeded inputs in float64 (plus a
float32 run stored as ``f_ref32``), writing inputs + outputs (f, attention, wx) to
``tests/golden/gat_mix/gatmix_*.npz`` and fp64 autograd gradients to
``tests/golden/gat_mix/gatmixgrad_*.npz`` (a directory of its own with its own
MANIFEST.json).  The gradients differentiate the reference layer's own forward
(:117-136) and the dense product of multiply_attention (:29-38) built with index_put,
as gen_golden_gat.py does and for its reason (the installed torch's backward of
``sparse.permute(0, 3, 1, 2).to_dense()`` is not the derivative of its forward); the
rebuilt forward is asserted equal to the reference's to 1e-13.  ``g_Wout`` is stored:
Wout is live under mix_features.  Inputs are generated in float32 and up-cast.
W, Wout ~ N(0, 0.3^2), a ~ N(0, 0.5^2).  Gradient fixtures are redrawn until every
LeakyReLU pre-activation |sl[src,h] + sr[dst,h]| >= 1e-4 (stored in meta).
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "gat_mix")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
import function_GAT_attention as ref_gat  # noqa: E402  (gen_golden put the reference on sys.path)

f32 = gg.f32
KINK_MIN = 1e-4


def _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope):
    return dict(gg.BASE_OPT, hidden_dim=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
                add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid, function='GAT', leaky_relu_slope=slope,
                mix_features=True)


def _func(opt, C, dt, W, Wout, a, alpha, beta, ei, x0):
    func = ref_gat.ODEFuncAtt(C, C, opt, 'cpu').to(dt)
    lay = func.multihead_att_layer
    assert all(isinstance(p, torch.nn.Parameter) and p.dtype == dt for p in (lay.W, lay.a, lay.Wout))
    with torch.no_grad():
        lay.W.copy_(torch.from_numpy(W))
        lay.Wout.copy_(torch.from_numpy(Wout))
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


def _draw(rng, B, N, C, att_dim, heads):
    x = f32(rng.standard_normal((B, N, C)))
    x0 = f32(rng.standard_normal((B, N, C)))
    W = f32(rng.standard_normal((C, att_dim)) * 0.3)
    Wout = f32(rng.standard_normal((att_dim, C)) * 0.3)
    a = f32(rng.standard_normal((2 * (att_dim // heads),)) * 0.5)
    return x, x0, W, Wout, a


def run_mix(name, rng, B, N, E, C, heads, att_dim, norm_idx, add_source=False, no_alpha_sigmoid=False, alpha=0.2,
            beta=0.5, slope=0.2, **gkw):
    opt = _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope)
    ei = gg.random_graph(rng, B, N, E, **gkw)
    x, x0, W, Wout, a = _draw(rng, B, N, C, att_dim, heads)
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    out = {}
    for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
        func, lay = _func(opt, C, dt, W, Wout, a, alpha, beta, ei, x0)
        xt = torch.from_numpy(x).to(dt)
        with torch.no_grad():
            att, wx = lay(xt, func.edge_index, None)
            f = func(torch.tensor(0.0), xt)
        out['f' + tag] = f.numpy()
        out['attention' + tag] = att.numpy()
        out['wx' + tag] = wx.numpy()
    pre = np.abs(_preact(x, W, a, ei, heads))
    dev32 = float(np.abs(out['f_ref32'].astype(np.float64) - out['f']).max() / np.abs(out['f']).max())
    meta = dict(kind='gat_mix', B=B, N=N, E=int(ei.shape[2]), C=C, heads=heads, attention_dim=att_dim,
                attention_norm_idx=norm_idx, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid,
                leaky_relu_slope=slope, preact_max=float(pre.max()), preact_min=float(pre.min()), ref32_dev=dev32)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0, W=W,
                        Wout=Wout, a=a, alpha_train=f32(alpha), beta_train=f32(beta), f=out['f'],
                        attention=out['attention'], wx=out['wx'], f_ref32=out['f_ref32'])
    print('%-22s fp32 run deviates %.2e from fp64' % (name, dev32))
    return name


def grad_mix(name, rng, B, N, E, C, heads, att_dim, norm_idx, add_source=False, no_alpha_sigmoid=False, alpha=0.2,
             beta=0.5, slope=0.2, **gkw):
    """Gradients of <gout, f> through the reference ODEFuncAtt.forward with mix_features
    w.r.t. x, alpha_train, beta_train, W, a and Wout."""
    opt = _opt(C, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid, slope)
    draws = 0
    while True:  # the kink condition: a condition on the inputs
        draws += 1
        ei = gg.random_graph(rng, B, N, E, **gkw)
        x, x0, W, Wout, a = _draw(rng, B, N, C, att_dim, heads)
        gout = f32(rng.standard_normal((B, N, C)))
        pre_min = float(np.abs(_preact(x, W, a, ei, heads)).min())
        if pre_min >= KINK_MIN:
            break
    alpha, beta = float(np.float32(alpha)), float(np.float32(beta))
    func, lay = _func(opt, C, torch.float64, W, Wout, a, alpha, beta, ei, x0)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    go = torch.from_numpy(gout).double()
    named = [('x', xt), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train), ('W', lay.W),
             ('a', lay.a), ('Wout', lay.Wout)]
    with torch.no_grad():
        f = func(torch.tensor(0.0), xt).numpy()
        att, wx = [t.numpy() for t in lay(xt, func.edge_index, None)]

    def forward():
        """ODEFuncAtt.forward (:50-68) with the reference layer's own forward (:117-136) and
        the mix_features product of multiply_attention (:29-38) with its dense [B,h,N,N]
        tensor built by index_put (duplicates summed; differentiable — gen_golden_gat.py)."""
        a_, wx_ = lay(xt, func.edge_index, None)
        eidx = func.edge_index
        bi = torch.arange(B)[:, None, None].expand(B, E, heads)
        hi = torch.arange(heads)[None, None, :].expand(B, E, heads)
        dense = torch.zeros(B, heads, N, N, dtype=torch.float64).index_put(
            (bi, hi, eidx[:, 0][:, :, None].expand(B, E, heads), eidx[:, 1][:, :, None].expand(B, E, heads)), a_,
            accumulate=True)
        wm = torch.mean(torch.matmul(dense, wx_.unsqueeze(1)), dim=1)      # :37
        ax = torch.matmul(wm, lay.Wout)                                    # :38
        alpha_ = func.alpha_train if no_alpha_sigmoid else torch.sigmoid(func.alpha_train)
        out = alpha_ * (ax - xt)
        return out + func.beta_train * func.x0 if add_source else out

    with torch.no_grad():
        assert float((forward() - torch.from_numpy(f)).abs().max()) <= 1e-13 * max(1.0, float(np.abs(f).max()))
    g = gg._grads(lambda: (forward() * go).sum(), named)
    assert g['g_Wout'].any(), "Wout is live under mix_features"
    g['g_a'] = g['g_a'].reshape(-1)
    meta = dict(kind='gat_mix_grad', B=B, N=N, E=E, C=C, heads=heads, attention_dim=att_dim,
                attention_norm_idx=norm_idx, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid,
                leaky_relu_slope=slope, preact_min=pre_min, draws=draws)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0, W=W,
                        Wout=Wout, a=a, alpha_train=f32(alpha), beta_train=f32(beta), f=f, attention=att, wx=wx,
                        gout=gout, **g)
    return name


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20251020)
    made = []
    made.append(run_mix('gatmix_n0_h2', rng, 1, 40, 160, 12, 2, 8, 0))
    made.append(run_mix('gatmix_n1_h8_b2', rng, 2, 33, 150, 16, 8, 16, 1, add_source=True))
    made.append(run_mix('gatmix_n1_c128_h4', rng, 1, 70, 400, 128, 4, 64, 1, dup_frac=0.1, n_isolated=3))
    made.append(run_mix('gatmix_n0_c128_a128', rng, 1, 70, 400, 128, 2, 128, 0, add_source=True,
                        no_alpha_sigmoid=True, alpha=0.8, beta=-0.3, slope=0.05))
    made.append(run_mix('gatmix_n0_c162', rng, 1, 45, 200, 162, 4, 48, 0, add_source=True))
    made.append(run_mix('gatmix_n1_c80_a20', rng, 1, 45, 200, 80, 4, 20, 1, no_alpha_sigmoid=True, alpha=0.6))
    made.append(run_mix('gatmix_n1_h1_b3', rng, 3, 37, 120, 64, 1, 16, 1))
    made.append(grad_mix('gatmixgrad_n0_h2', rng, 1, 60, 320, 12, 2, 16, 0))
    made.append(grad_mix('gatmixgrad_n1_h2', rng, 1, 60, 320, 12, 2, 16, 1))
    made.append(grad_mix('gatmixgrad_n1_h8_b2', rng, 2, 40, 200, 16, 8, 32, 1))
    made.append(grad_mix('gatmixgrad_n0_src', rng, 1, 50, 260, 10, 2, 8, 0, add_source=True, no_alpha_sigmoid=True,
                         alpha=0.8, beta=-0.3))
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump(sorted(made), fh, indent=1)
    print('wrote', len(made), 'fixtures to', OUT_DIR)


if __name__ == '__main__':
    main()
