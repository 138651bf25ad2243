#!/usr/bin/env python
"""Golden-vector generator for the squareplus attention normalisation (opt['square_plus']).

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference tree
through gen_golden.py); nothing under tests/ imports it.  It loads gen_golden.py as a
module for its stand-ins, BASE_OPT, random_graph and _grads.

The reference's own call site of squareplus is broken (function_transformer_attention.py:264
passes a 2-D slice and omits num_nodes), so the fixtures compose the reference's own pieces
the way that line intends:

  1. the reference layer, run with square_plus=False, returns its own ``prods`` [B,E,h]
     (SpGraphTransAttentionLayer.forward :218-259, second output);
  2. the reference's own ``utils.squareplus(prods, edge[:, norm_idx, :], None)`` (:129-140);
  3. the reference function's ``multiply_attention`` (:20-42) and the epilogue of its
     forward (:52-59), restated here line by line.

``score_mode='per_edge'`` (upstream GRAND's q_src . k_dst / sqrt(dk), which the fork's :249
does not compute) takes the reference layer's own Q and K projections and forms the
per-edge product here; steps 2 and 3 are the same.

Everything runs in float64 (inputs generated in float32 and up-cast); a float32 run of the
same composition is stored as ``f_ref32`` / ``attention_ref32``.  Forward fixtures
``tests/golden/squareplus/sp_*.npz``, fp64 autograd gradients ``spgrad_*.npz`` (x, alpha,
beta, Q / K weights and biases, for exp_kernel also output_var and lengthscale), with a
MANIFEST.json of their own.

Conditions on the inputs (asserted / redrawn until they hold, the figures stored in meta):
  * ``sp_sd_n1_h8_b3``: the three global maxima M_b differ pairwise by at least 1, so a
    maximum taken across the batch gives another result;
  * ``sp_sd_n1_wide``: node scores with a standard deviation of about 50; the reference
    formula (t + sqrt(t^2 + 4)) / 2 evaluated in float32 numpy misses the forward bar
    (attention 2e-5 absolute) on it, so the case tells the stable form from the literal one;
  * gradient fixtures: the largest score of each batch element exceeds the next distinct
    score by at least 1e-3 (``max_margin``): torch.amax spreads the derivative of the
    maximum evenly over ties, which is the same total when the ties are copies of one score
    (all out-edges of one source under the fork's scaled_dot, duplicate edges).
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "squareplus")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
ref_att, ref_utils = gg.ref_att, gg.ref_utils

f32 = gg.f32
ATT_ATOL = 2e-5      # the forward bar on the attention (tests/test_gpu_squareplus.py)
MARGIN_MIN = 1e-3
OV, LS = float(np.float32(1.3)), float(np.float32(0.8))


def _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid):
    return dict(gg.BASE_OPT, hidden_dim=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
                attention_type=attention_type, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid,
                function='transformer', square_plus=False)


def _func(opt, C, dt, P, ei, x0):
    func = ref_att.ODEFuncTransformerAtt(C, C, opt, 'cpu').to(dt)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(P['alpha'])
        func.beta_train.fill_(P['beta'])
        lay.Q.weight.copy_(torch.from_numpy(P['Wq']))
        lay.Q.bias.copy_(torch.from_numpy(P['bq']))
        lay.K.weight.copy_(torch.from_numpy(P['Wk']))
        lay.K.bias.copy_(torch.from_numpy(P['bk']))
        if opt['attention_type'] == 'exp_kernel':
            lay.output_var.fill_(OV)
            lay.lengthscale.fill_(LS)
    func.edge_index = torch.from_numpy(ei)
    func.x0 = torch.from_numpy(x0).to(dt)
    func.y = None
    return func, lay


def _prods(lay, xt, edge, score_mode):
    """Step 1: the reference layer's own prods; per_edge: its Q / K projections, multiplied per edge."""
    if score_mode == 'per_edge':
        assert lay.opt['attention_type'] == 'scaled_dot'
        B, N = xt.shape[0], xt.shape[1]
        q = lay.Q(xt).view(B, N, lay.h, lay.d_k)
        k = lay.K(xt).view(B, N, lay.h, lay.d_k)
        b = torch.arange(B)[:, None]
        return (q[b, edge[:, 0]] * k[b, edge[:, 1]]).sum(-1) / np.sqrt(lay.d_k)
    return lay(xt, edge, None)[1][1]


def _forward(func, lay, xt, score_mode):
    """Steps 1-3 -> (f, attention, prods)."""
    opt = func.opt
    edge = func.edge_index
    prods = _prods(lay, xt, edge, score_mode)
    att = ref_utils.squareplus(prods, edge[:, opt['attention_norm_idx'], :], None)
    ax = func.multiply_attention(xt, att, None)
    alpha = func.alpha_train if opt['no_alpha_sigmoid'] else torch.sigmoid(func.alpha_train)
    f = alpha * (ax - xt)
    if opt['add_source']:
        f = f + func.beta_train * func.x0
    return f, att, prods


def _margin(prods):
    """Per batch element: the largest score minus the next distinct one (copies of the
    maximum, equal to rounding, count as the maximum)."""
    out = []
    for pb in prods:
        v = np.sort(np.asarray(pb, np.float64).reshape(-1))
        top = v[-1]
        rest = v[v < top - 1e-9 * max(1.0, abs(top))]
        out.append(float(top - rest[-1]) if rest.size else float('inf'))
    return out


def _draw(rng, B, N, E, C, att_dim, wstd, xscale, gkw):
    ei = gg.random_graph(rng, B, N, E, **gkw)
    x = f32(rng.standard_normal((B, N, C)))
    if xscale is not None:
        x = f32(x * np.asarray(xscale, np.float32).reshape(B, 1, 1))
    P = dict(Wq=f32(rng.standard_normal((att_dim, C)) * wstd), bq=f32(rng.standard_normal((att_dim,)) * wstd),
             Wk=f32(rng.standard_normal((att_dim, C)) * wstd), bk=f32(rng.standard_normal((att_dim,)) * wstd))
    return ei, x, f32(rng.standard_normal((B, N, C))), P


def _meta(kind, B, N, E, C, heads, att_dim, norm_idx, attention_type, score_mode, add_source, no_alpha_sigmoid,
          prods, **extra):
    m = dict(kind=kind, B=B, N=N, E=E, C=C, heads=heads, attention_dim=att_dim, attention_norm_idx=norm_idx,
             attention_type=attention_type, score_mode=score_mode, add_source=add_source,
             no_alpha_sigmoid=no_alpha_sigmoid, square_plus=True,
             output_var=OV if attention_type == 'exp_kernel' else None,
             lengthscale=LS if attention_type == 'exp_kernel' else None,
             M=[float(p.max()) for p in prods], max_margin=_margin(prods),
             score_std=float(np.std(prods)))
    m.update(extra)
    return m


def run_sp(name, rng, B, N, E, C, heads, att_dim, norm_idx, attention_type='scaled_dot', score_mode='reference',
           add_source=False, no_alpha_sigmoid=False, alpha=0.2, beta=0.5, wstd=0.1, xscale=None, ei=None,
           check=None, score_std=None, **gkw):
    opt = _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid)
    draws = 0
    while True:
        draws += 1
        ei_d, x, x0, P = _draw(rng, B, N, E, C, att_dim, wstd, xscale, gkw)
        if ei is not None:
            ei_d = ei
        P.update(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
        if score_std is not None:  # the scores are linear in (Wq, bq): scaled to the asked spread
            func, lay = _func(opt, C, torch.float64, P, ei_d, x0)
            with torch.no_grad():
                sd = float(_forward(func, lay, torch.from_numpy(x).double(), score_mode)[2].std())
            P['Wq'], P['bq'] = f32(P['Wq'] * (score_std / sd)), f32(P['bq'] * (score_std / sd))
        out = {}
        for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
            func, lay = _func(opt, C, dt, P, ei_d, x0)
            with torch.no_grad():
                f, att, prods = _forward(func, lay, torch.from_numpy(x).to(dt), score_mode)
            out['f' + tag], out['attention' + tag], out['prods' + tag] = f.numpy(), att.numpy(), prods.numpy()
        extra = {} if check is None else check(out, ei_d, norm_idx)
        if extra is not None:
            break
        assert draws < 200, name
    meta = _meta('squareplus', B, N, int(ei_d.shape[2]), C, heads, att_dim, norm_idx, attention_type, score_mode,
                 add_source, no_alpha_sigmoid, out['prods'], draws=draws, **extra)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei_d, x=x, x0=x0,
                        Wq=P['Wq'], bq=P['bq'], Wk=P['Wk'], bk=P['bk'], alpha_train=f32(P['alpha']),
                        beta_train=f32(P['beta']), f=out['f'], attention=out['attention'], f_ref32=out['f_ref32'],
                        attention_ref32=out['attention_ref32'])
    return name, ei_d


def _check_batch_maxima(out, ei, norm_idx):
    """The global maxima of the batch elements differ pairwise by at least 1."""
    M = sorted(float(p.max()) for p in out['prods'])
    gap = min(b - a for a, b in zip(M, M[1:]))
    return dict(M_gap=gap) if gap >= 1.0 else None


def _check_wide(out, ei, norm_idx):
    """The literal fp32 formula misses the attention bar (node scores of std ~ 50: score_std)."""
    s = out['prods'].astype(np.float32)
    t = s - s.max(axis=(1, 2), keepdims=True)
    sp = (t + np.sqrt(t * t + np.float32(4.0))) / np.float32(2.0)
    att = np.empty_like(sp)
    n = int(ei.max()) + 1
    for b in range(sp.shape[0]):
        sm = np.zeros((n, sp.shape[2]), np.float32)
        np.add.at(sm, ei[b, norm_idx], sp[b])
        att[b] = sp[b] / (sm[ei[b, norm_idx]] + np.float32(1e-16))
    err = float(np.abs(att.astype(np.float64) - out['attention']).max())
    assert err > ATT_ATOL, "the literal fp32 formula passes the bar (%.3e): the case tells nothing apart" % err
    return dict(literal_fp32_attention_err=err)


def grad_sp(name, rng, B, N, E, C, heads, att_dim, norm_idx, attention_type='scaled_dot', score_mode='reference',
            add_source=False, no_alpha_sigmoid=False, alpha=0.2, beta=0.5, wstd=0.1, **gkw):
    """fp64 autograd gradients of <gout, f> through the composition of _forward."""
    opt = _opt(C, heads, att_dim, norm_idx, attention_type, add_source, no_alpha_sigmoid)
    draws = 0
    while True:  # a unique maximum (up to copies of one score) per batch element
        draws += 1
        ei, x, x0, P = _draw(rng, B, N, E, C, att_dim, wstd, None, gkw)
        gout = f32(rng.standard_normal((B, N, C)))
        P.update(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
        func, lay = _func(opt, C, torch.float64, P, ei, x0)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        with torch.no_grad():
            f, att, prods = _forward(func, lay, xt, score_mode)
        if min(_margin(prods.numpy())) >= MARGIN_MIN:
            break
        assert draws < 200, name
    go = torch.from_numpy(gout).double()
    named = [('x', xt), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train), ('Wq', lay.Q.weight),
             ('bq', lay.Q.bias), ('Wk', lay.K.weight), ('bk', lay.K.bias)]
    if attention_type == 'exp_kernel':
        named += [('output_var', lay.output_var), ('lengthscale', lay.lengthscale)]
    g = gg._grads(lambda: (_forward(func, lay, xt, score_mode)[0] * go).sum(), named)
    meta = _meta('squareplus_grad', B, N, E, C, heads, att_dim, norm_idx, attention_type, score_mode, add_source,
                 no_alpha_sigmoid, prods.numpy(), draws=draws)
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), edge_index=ei, x=x, x0=x0,
                        Wq=P['Wq'], bq=P['bq'], Wk=P['Wk'], bk=P['bk'], alpha_train=f32(P['alpha']),
                        beta_train=f32(P['beta']), gout=gout, f=f.numpy(), attention=att.numpy(), **g)
    return name


BEST_PARAMS_KEYS = ('block', 'function', 'heads', 'attention_dim', 'attention_norm_idx', 'add_source', 'square_plus',
                    'hidden_dim', 'method', 'time', 'step_size', 'tol_scale', 'tol_scale_adjoint', 'adjoint',
                    'adjoint_method', 'attention_type', 'att_samp_pct', 'no_alpha_sigmoid', 'self_loop_weight',
                    'leaky_relu_slope', 'reweight_attention', 'beltrami', 'augment', 'max_nfe', 'mix_features',
                    'data_norm')


def write_best_params():
    """The settings (values only) of the best_params entries that set square_plus
    (src/best_params.py), restricted to the keys the ODE block reads:
    tests/golden/squareplus/best_params_squareplus.json."""
    import best_params  # noqa: E402  (gen_golden put the reference on sys.path)
    out = {name: {k: bp[k] for k in BEST_PARAMS_KEYS if k in bp}
           for name, bp in best_params.best_params_dict.items() if bp.get('square_plus')}
    assert sorted(out) == ['Citeseer', 'CoauthorCS', 'Cora', 'Pubmed'], sorted(out)
    with open(os.path.join(OUT_DIR, 'best_params_squareplus.json'), 'w') as fh:
        json.dump(out, fh, indent=1, sort_keys=True)


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    write_best_params()
    rng = np.random.default_rng(20251019)
    made = []
    n, ei = run_sp('sp_sd_n0_h2', rng, 1, 60, 320, 16, 2, 16, 0)  # uniform: 1/outdeg
    made.append(n)
    made.append(run_sp('sp_sd_n1_h2', rng, 1, 60, 320, 16, 2, 16, 1, ei=ei)[0])  # the same graph
    made.append(run_sp('sp_sd_n1_h1', rng, 1, 40, 200, 16, 1, 8, 1, wstd=0.2)[0])
    made.append(run_sp('sp_sd_n1_h8_b3', rng, 3, 50, 240, 16, 8, 32, 1, wstd=0.3, xscale=(1.0, 1.6, 2.3),
                       check=_check_batch_maxima)[0])
    made.append(run_sp('sp_sd_n1_src', rng, 1, 70, 350, 16, 4, 16, 1, add_source=True, alpha=0.8, beta=-0.3)[0])
    made.append(run_sp('sp_sd_n1_c128', rng, 1, 300, 2400, 128, 2, 32, 1, wstd=0.05, dup_frac=0.1, n_isolated=5)[0])
    made.append(run_sp('sp_sd_n1_c162', rng, 1, 150, 900, 162, 2, 32, 1, wstd=0.05)[0])
    made.append(run_sp('sp_sd_n1_wide', rng, 1, 200, 2000, 16, 2, 16, 1, score_std=50.0, check=_check_wide)[0])
    n, ei = run_sp('sp_pe_n0_h2', rng, 1, 60, 320, 16, 2, 16, 0, score_mode='per_edge', wstd=0.3)
    made.append(n)
    made.append(run_sp('sp_pe_n1_h2', rng, 1, 60, 320, 16, 2, 16, 1, score_mode='per_edge', wstd=0.3, ei=ei)[0])
    made.append(run_sp('sp_pe_n0_nosig', rng, 2, 40, 200, 16, 4, 16, 0, score_mode='per_edge', wstd=0.3,
                       no_alpha_sigmoid=True, alpha=0.7)[0])
    made.append(run_sp('sp_pe_n1_c128_h8', rng, 1, 160, 1200, 128, 8, 128, 1, score_mode='per_edge', wstd=0.05,
                       dup_frac=0.1, n_isolated=3)[0])
    for st in ('exp_kernel', 'cosine_sim', 'pearson'):
        for ni in (0, 1):
            made.append(run_sp('sp_%s_n%d' % (st, ni), rng, 2, 40, 200, 16, 2, 8, ni, attention_type=st,
                               wstd=0.3)[0])
    made.append(grad_sp('spgrad_sd_n0_h2', rng, 1, 60, 320, 16, 2, 16, 0))
    made.append(grad_sp('spgrad_sd_n1_h2', rng, 1, 60, 320, 16, 2, 16, 1))
    made.append(grad_sp('spgrad_sd_n1_h8_b2', rng, 2, 40, 200, 16, 8, 32, 1, wstd=0.2))
    made.append(grad_sp('spgrad_sd_n1_src', rng, 1, 50, 260, 16, 2, 8, 1, add_source=True, no_alpha_sigmoid=True,
                        alpha=0.8, beta=-0.3))
    for ni in (0, 1):
        made.append(grad_sp('spgrad_pe_n%d' % ni, rng, 2, 40, 200, 16, 2, 8, ni, score_mode='per_edge', wstd=0.3))
    for st in ('exp_kernel', 'cosine_sim', 'pearson'):
        for ni in (0, 1):
            made.append(grad_sp('spgrad_%s_n%d' % (st, ni), rng, 2, 40, 200, 16, 2, 8, ni, attention_type=st,
                                wstd=0.3))
    with open(os.path.join(OUT_DIR, 'MANIFEST.json'), 'w') as fh:
        json.dump(sorted(made), fh, indent=1)
    print('wrote', len(made), 'fixtures to', OUT_DIR)


if __name__ == '__main__':
    main()
