#!/usr/bin/env python
"""Golden-vector generator for the transformer attention ODE function with mix_features.

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference
tree through gen_golden.py); nothing under tests/ imports it.  It loads
gen_golden.py as a module for its stand-ins, BASE_OPT, random_graph and _grads.

The reference's call site is broken under ``mix_features`` (forward hands
multiply_attention the tuple ``(v, prods)``, :50, and :29 reads ``v.shape``), so the
fixtures compose the reference's own pieces as the call site intends, in float64
(plus a float32 run stored as ``f_ref32``):

  * SpGraphTransAttentionLayer.forward (:159-267) -> attention, (v, prods);
  * ODEFuncTransformerAtt.multiply_attention(x, attention, values[0]) (:23-32);
  * the epilogue of :52-59.

score_mode 'per_edge' (upstream GRAND's q_src . k_dst / sqrt(dk), not in the fork) takes
the layer's own Q / K projections multiplied per edge and the reference's utils.softmax;
``square_plus`` takes utils.squareplus(prods, edge[:, norm_idx, :], None) on the layer's
prods, both as gen_golden_squareplus.py composes them.  v is always the layer's own.

Outputs: inputs + (f, attention, v [B,N,att] with head h in columns h*dk ..) to
``tests/golden/mix/mix_*.npz`` and fp64 autograd gradients to ``mixgrad_*.npz`` with a
MANIFEST.json.  The gradients differentiate the same composition with the dense
[B,h,N,N] tensor built by index_put (the installed torch's backward of
``sparse.permute(0, 3, 1, 2).to_dense()`` is not the derivative of its forward:
gen_golden_gat_mix.py); the rebuilt forward is asserted equal to the reference's to
1e-13.  All parameters are random: weights ~ N(0, 0.3^2) (Q / K: N(0, wstd^2), as the
other transformer fixtures), biases non-zero, Wout.bias and V.bias included.  The
squareplus gradient fixture is redrawn until the largest score of every batch element
exceeds the next distinct one by 1e-3 (gen_golden_squareplus.py's arg-max margin rule).
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "mix")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
ref_att, ref_utils = gg.ref_att, gg.ref_utils

f32 = gg.f32
MARGIN_MIN = 1e-3
OV, LS = float(np.float32(1.3)), float(np.float32(0.8))
PNAMES = ('Wq', 'bq', 'Wk', 'bk', 'Wv', 'bv', 'Wout', 'bout')


def _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid):
    return dict(gg.BASE_OPT, hidden_dim=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
                attention_type=attention_type, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid,
                function='transformer', square_plus=False, mix_features=True)


def _params(lay):
    return dict(Wq=lay.Q.weight, bq=lay.Q.bias, Wk=lay.K.weight, bk=lay.K.bias, Wv=lay.V.weight, bv=lay.V.bias,
                Wout=lay.Wout.weight, bout=lay.Wout.bias)


def _func(opt, C, dt, P, ei, x0):
    func = ref_att.ODEFuncTransformerAtt(C, C, opt, 'cpu').to(dt)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(P['alpha'])
        func.beta_train.fill_(P['beta'])
        for n, t in _params(lay).items():
            t.copy_(torch.from_numpy(P[n]))
        if opt['attention_type'] == 'exp_kernel':
            lay.output_var.fill_(OV)
            lay.lengthscale.fill_(LS)
    func.edge_index = torch.from_numpy(ei)
    func.x0 = torch.from_numpy(x0).to(dt)
    func.y = None
    return func, lay


def _attention(lay, xt, edge, score_mode, square_plus):
    """(attention, v [B,N,dk,h], prods): the layer's own forward; per_edge / square_plus recomposed."""
    att, (v, prods) = lay(xt, edge, None)
    nidx = lay.opt['attention_norm_idx']
    if score_mode == 'per_edge':
        assert lay.opt['attention_type'] == 'scaled_dot'
        B, N = xt.shape[0], xt.shape[1]
        q = lay.Q(xt).view(B, N, lay.h, lay.d_k)
        k = lay.K(xt).view(B, N, lay.h, lay.d_k)
        b = torch.arange(B)[:, None]
        prods = (q[b, edge[:, 0]] * k[b, edge[:, 1]]).sum(-1) / np.sqrt(lay.d_k)
        if not square_plus:
            att = ref_utils.softmax(prods, edge[:, nidx, :])
    if square_plus:
        att = ref_utils.squareplus(prods, edge[:, nidx, :], None)
    return att, v, prods


def _epilogue(func, ax, xt):
    alpha = func.alpha_train if func.opt['no_alpha_sigmoid'] else torch.sigmoid(func.alpha_train)
    f = alpha * (ax - xt)
    if func.opt['add_source']:
        f = f + func.beta_train * func.x0
    return f


def _forward(func, lay, xt, score_mode, square_plus):
    """The reference's pieces -> (f, attention, v [B,N,dk,h], prods)."""
    att, v, prods = _attention(lay, xt, func.edge_index, score_mode, square_plus)
    ax = func.multiply_attention(xt, att, v)
    return _epilogue(func, ax, xt), att, v, prods


def _forward_dense(func, lay, xt, score_mode, square_plus):
    """The same with the dense [B,h,N,N] tensor of :29-31 built by index_put (differentiable)."""
    att, v, _ = _attention(lay, xt, func.edge_index, score_mode, square_plus)
    e = func.edge_index
    B, _, E = e.shape
    H, N = lay.h, xt.shape[1]
    bi = torch.arange(B)[:, None, None].expand(B, E, H)
    hi = torch.arange(H)[None, None, :].expand(B, E, H)
    dense = torch.zeros(B, H, N, N, dtype=att.dtype).index_put(
        (bi, hi, e[:, 0][:, :, None].expand(B, E, H), e[:, 1][:, :, None].expand(B, E, H)), att, accumulate=True)
    vx = torch.mean(torch.matmul(dense, v.permute(0, 3, 1, 2)), dim=1)     # :31
    return _epilogue(func, lay.Wout(vx), xt)                                # :32


def _flat_v(v):
    """[B,N,dk,h] -> [B,N,att] with head h in columns h*dk .. (the layout of V(x))."""
    v = v.numpy()
    return np.ascontiguousarray(v.transpose(0, 1, 3, 2)).reshape(v.shape[0], v.shape[1], -1)


def _margin(prods):
    out = []
    for pb in prods:
        s = np.sort(np.asarray(pb, np.float64).reshape(-1))
        top = s[-1]
        rest = s[s < top - 1e-9 * max(1.0, abs(top))]
        out.append(float(top - rest[-1]) if rest.size else float('inf'))
    return out


def _draw(rng, B, N, E, C, heads, att_dim, wstd, gkw):
    dk = att_dim // heads
    ei = gg.random_graph(rng, B, N, E, **gkw)
    x = f32(rng.standard_normal((B, N, C)))
    x0 = f32(rng.standard_normal((B, N, C)))
    P = dict(Wq=f32(rng.standard_normal((att_dim, C)) * wstd), bq=f32(rng.standard_normal((att_dim,)) * wstd),
             Wk=f32(rng.standard_normal((att_dim, C)) * wstd), bk=f32(rng.standard_normal((att_dim,)) * wstd),
             Wv=f32(rng.standard_normal((att_dim, C)) * 0.3), bv=f32(rng.standard_normal((att_dim,)) * 0.3),
             Wout=f32(rng.standard_normal((C, dk)) * 0.3), bout=f32(rng.standard_normal((C,)) * 0.3))
    return ei, x, x0, P


def _meta(kind, B, N, E, C, heads, att_dim, norm_idx, attention_type, score_mode, square_plus, add_source,
          no_alpha_sigmoid, **extra):
    m = dict(kind=kind, B=B, N=N, E=E, C=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
             attention_type=attention_type, score_mode=score_mode, square_plus=square_plus, add_source=add_source,
             no_alpha_sigmoid=no_alpha_sigmoid, mix_features=True,
             output_var=OV if attention_type == 'exp_kernel' else None,
             lengthscale=LS if attention_type == 'exp_kernel' else None)
    m.update(extra)
    return m


def run_mix(name, rng, B, N, E, C, heads, att_dim, norm_idx, attention_type='scaled_dot', score_mode='reference',
            square_plus=False, add_source=False, no_alpha_sigmoid=False, alpha=0.2, beta=0.5, wstd=0.1, **gkw):
    opt = _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid)
    ei, x, x0, P = _draw(rng, B, N, E, C, heads, att_dim, wstd, gkw)
    P.update(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
    out = {}
    for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
        func, lay = _func(opt, C, dt, P, ei, x0)
        with torch.no_grad():
            f, att, v, _ = _forward(func, lay, torch.from_numpy(x).to(dt), score_mode, square_plus)
        out['f' + tag], out['attention' + tag], out['v' + tag] = f.numpy(), att.numpy(), _flat_v(v)
    dev32 = float(np.abs(out['f_ref32'].astype(np.float64) - out['f']).max() / np.abs(out['f']).max())
    meta = _meta('mix', B, N, int(ei.shape[2]), C, heads, att_dim, norm_idx, attention_type, score_mode, square_plus,
                 add_source, no_alpha_sigmoid, ref32_dev=dev32)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0,
                        alpha_train=f32(P['alpha']), beta_train=f32(P['beta']), f=out['f'],
                        attention=out['attention'], v=out['v'], f_ref32=out['f_ref32'], **{n: P[n] for n in PNAMES})
    print('%-26s fp32 run deviates %.2e from fp64' % (name, dev32))
    return name


def grad_mix(name, rng, B, N, E, C, heads, att_dim, norm_idx, attention_type='scaled_dot', score_mode='reference',
             square_plus=False, add_source=False, no_alpha_sigmoid=False, alpha=0.2, beta=0.5, wstd=0.1, **gkw):
    """Gradients of <gout, f> through the composition w.r.t. x, alpha_train, beta_train, Q, K, V, Wout
    (weights and biases) and exp_kernel's two parameters."""
    opt = _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid)
    draws = 0
    while True:
        draws += 1
        ei, x, x0, P = _draw(rng, B, N, E, C, heads, att_dim, wstd, gkw)
        gout = f32(rng.standard_normal((B, N, C)))
        P.update(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
        func, lay = _func(opt, C, torch.float64, P, ei, x0)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        with torch.no_grad():
            f, att, v, prods = _forward(func, lay, xt, score_mode, square_plus)
        margin = _margin(prods.numpy())
        if not square_plus or min(margin) >= MARGIN_MIN:
            break
        assert draws < 200, name
    go = torch.from_numpy(gout).double()
    named = [('x', xt), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train)] + \
        list(_params(lay).items())
    if attention_type == 'exp_kernel':
        named += [('output_var', lay.output_var), ('lengthscale', lay.lengthscale)]
    with torch.no_grad():
        rebuilt = _forward_dense(func, lay, xt, score_mode, square_plus)
        assert float((rebuilt - f).abs().max()) <= 1e-13 * max(1.0, float(f.abs().max())), name
    g = gg._grads(lambda: (_forward_dense(func, lay, xt, score_mode, square_plus) * go).sum(), named)
    assert g['g_Wout'].any() and g['g_Wv'].any() and g['g_bout'].any() and g['g_bv'].any()
    for n in ('g_output_var', 'g_lengthscale'):
        if n in g:
            g[n] = g[n].reshape(-1)
    meta = _meta('mix_grad', B, N, E, C, heads, att_dim, norm_idx, attention_type, score_mode, square_plus,
                 add_source, no_alpha_sigmoid, draws=draws, max_margin=margin if square_plus else None)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0,
                        alpha_train=f32(P['alpha']), beta_train=f32(P['beta']), f=f.numpy(), attention=att.numpy(),
                        v=_flat_v(v), gout=gout, **{n: P[n] for n in PNAMES}, **g)
    return name


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20261020)
    made = []
    # scaled_dot reference: the uniform case (norm_idx 0) and norm_idx 1
    made.append(run_mix('mix_sd_n0_h2', rng, 1, 40, 160, 12, 2, 8, 0))
    made.append(run_mix('mix_sd_n1_h8_b2', rng, 2, 33, 150, 128, 8, 128, 1, add_source=True))
    # per_edge under both groupings
    made.append(run_mix('mix_pe_n0_h4_c128', rng, 1, 70, 400, 128, 4, 64, 0, score_mode='per_edge', dup_frac=0.1,
                        n_isolated=3))
    made.append(run_mix('mix_pe_n1_h2_dk64', rng, 1, 60, 300, 128, 2, 128, 1, score_mode='per_edge',
                        no_alpha_sigmoid=True, alpha=0.8, beta=-0.3))
    made.append(run_mix('mix_exp_n1_h1', rng, 1, 45, 200, 12, 1, 16, 1, attention_type='exp_kernel'))
    made.append(run_mix('mix_cos_n0_h2_c162', rng, 1, 45, 200, 162, 2, 16, 0, attention_type='cosine_sim',
                        add_source=True))
    made.append(run_mix('mix_pearson_n1_h4', rng, 1, 45, 200, 12, 4, 32, 1, attention_type='pearson'))
    # the plain kernels: dk % 4 != 0, heads = 3
    made.append(run_mix('mix_sd_n1_dk5', rng, 1, 40, 180, 12, 2, 10, 1))
    made.append(run_mix('mix_pe_n0_h3', rng, 1, 40, 180, 12, 3, 12, 0, score_mode='per_edge'))
    made.append(run_mix('mix_sp_n1_h2', rng, 1, 50, 240, 12, 2, 16, 1, square_plus=True))
    made.append(grad_mix('mixgrad_sd_n1_h2', rng, 1, 60, 320, 12, 2, 16, 1))
    made.append(grad_mix('mixgrad_pe_n0_h2', rng, 1, 60, 320, 12, 2, 16, 0, score_mode='per_edge'))
    made.append(grad_mix('mixgrad_exp_n1_h2', rng, 1, 50, 260, 10, 2, 8, 1, attention_type='exp_kernel',
                         add_source=True, no_alpha_sigmoid=True, alpha=0.8, beta=-0.3))
    made.append(grad_mix('mixgrad_sd_n1_h8_b2', rng, 2, 40, 200, 16, 8, 32, 1))
    made.append(grad_mix('mixgrad_sp_n0_pe', rng, 1, 50, 260, 12, 2, 16, 0, score_mode='per_edge', square_plus=True))
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump(sorted(made), fh, indent=1)
    print('wrote', len(made), 'fixtures to', OUT_DIR)


if __name__ == '__main__':
    main()
