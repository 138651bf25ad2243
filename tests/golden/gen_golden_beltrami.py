#!/usr/bin/env python
"""Golden-vector generator for the beltrami exp_kernel attention (opt['beltrami'],
attention_type='exp_kernel', opt['gnpde_beltrami_kernel']).

RUNS ONLY IN THE BUILD CONTAINER, by hand (it imports the read-only reference tree through
gen_golden.py); nothing under tests/ imports it.  It loads gen_golden.py as a module for its
stand-ins, BASE_OPT, random_graph and _grads.

The reference's branch slices the node axis where it means the feature axis
(function_transformer_attention.py:166-167, x[:, a:b] on a [B,N,C] state), so it cannot run.
The fixtures compose the reference's own pieces the way the branch means them:

  1. the reference layer constructed with beltrami=True, attention_type='exp_kernel' (its
     constructor works): its parameter names and its own Qx, Kx, Qp, Kp modules, in float64;
  2. the slice along the feature axis and the score, written here from the formula
       p = x[..., F:F+P], xf = cat(x[..., :F], x[..., F+P:])
       s = ovx^2 exp(-|Qx(xf)_src - Kx(xf)_dst|^2 / (2 lsx^2)) * ovp^2 exp(-|Qp(p)_src - Kp(p)_dst|^2 / (2 lsp^2))
     per head (the literal product of the two exponentials, unfolded projections);
  3. the reference's own utils.softmax / utils.squareplus(prods, edge[:, norm_idx, :], None);
  4. the reference function's multiply_attention (:20-42, v = None) and the epilogue of its
     forward (:52-59), restated line by line;
  5. float64 autograd for the gradients of a random linear loss on f.

Everything runs in float64 (inputs generated in float32 and up-cast).  Two conditions are
asserted for every case (redrawn until they hold) and recorded in meta.json:
  * the same composition in FLOAT32 torch is within FP32_BAR = 3e-6 of float64 (attention
    absolute, f relative): the kernels keep a margin under the project's 1e-5 bar;
  * within some normalisation group the scores span at least a factor SPAN_MIN = 10 (and the
    attention of some group a factor 2): a wrong score does not hide in a near-uniform attention.
Squareplus cases with gradients also keep the margin of gen_golden_squareplus.py between
the largest score and the next distinct one.

Writes tests/golden/beltrami/<case>.npz and meta.json (the cases' metadata and, as data, the
reference layer's state_dict key list).
"""
import importlib.util
import json
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "beltrami")
_spec = importlib.util.spec_from_file_location("gen_golden", os.path.join(HERE, "gen_golden.py"))
gg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gg)
ref_att, ref_utils = gg.ref_att, gg.ref_utils

f32 = gg.f32
FP32_BAR = 3e-6
SPAN_MIN = 10.0
MARGIN_MIN = 1e-3
OVX, LSX, OVP, LSP = (float(np.float32(v)) for v in (1.6, 0.7, 1.5, 1.9))
PNAMES = ("Wqx", "bqx", "Wkx", "bkx", "Wqp", "bqp", "Wkp", "bkp")
SNAMES = ("output_var_x", "lengthscale_x", "output_var_p", "lengthscale_p")


def _opt(C, F, P, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid):
    return dict(gg.BASE_OPT, hidden_dim=C, feat_hidden_dim=F, pos_enc_hidden_dim=P, heads=heads,
                attention_dim=att_dim, attention_norm_idx=norm_idx, attention_type='exp_kernel', beltrami=True,
                add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid, function='transformer', square_plus=False)


def _func(opt, C, dt, Pm, ei, x0):
    func = ref_att.ODEFuncTransformerAtt(C, C, opt, 'cpu').to(dt)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(Pm['alpha'])
        func.beta_train.fill_(Pm['beta'])
        for lin, w, b in ((lay.Qx, 'Wqx', 'bqx'), (lay.Kx, 'Wkx', 'bkx'), (lay.Qp, 'Wqp', 'bqp'),
                          (lay.Kp, 'Wkp', 'bkp')):
            lin.weight.copy_(torch.from_numpy(Pm[w]))
            lin.bias.copy_(torch.from_numpy(Pm[b]))
        lay.output_var_x.fill_(OVX)
        lay.lengthscale_x.fill_(LSX)
        lay.output_var_p.fill_(OVP)
        lay.lengthscale_p.fill_(LSP)
    func.edge_index = torch.from_numpy(ei)
    func.x0 = torch.from_numpy(x0).to(dt)
    func.y = None
    return func, lay


def _prods(lay, xt, edge):
    """Step 2: the slices along the feature axis and the literal product of the two kernels."""
    F, P = lay.opt['feat_hidden_dim'], lay.opt['pos_enc_hidden_dim']
    p = xt[..., F:F + P]
    xf = torch.cat((xt[..., :F], xt[..., F + P:]), dim=-1)
    B, N = xt.shape[0], xt.shape[1]
    b = torch.arange(B)[:, None]

    def sqdist(Q, K, z):
        q = Q(z).view(B, N, lay.h, lay.d_k)
        k = K(z).view(B, N, lay.h, lay.d_k)
        return torch.sum((q[b, edge[:, 0]] - k[b, edge[:, 1]]) ** 2, dim=-1)

    return lay.output_var_x ** 2 * torch.exp(-sqdist(lay.Qx, lay.Kx, xf) / (2 * lay.lengthscale_x ** 2)) \
        * lay.output_var_p ** 2 * torch.exp(-sqdist(lay.Qp, lay.Kp, p) / (2 * lay.lengthscale_p ** 2))


def _forward(func, lay, xt, square_plus):
    """Steps 2-4 -> (f, attention, prods)."""
    opt = func.opt
    edge = func.edge_index
    prods = _prods(lay, xt, edge)
    index = edge[:, opt['attention_norm_idx'], :]
    att = ref_utils.squareplus(prods, index, None) if square_plus else ref_utils.softmax(prods, index)
    ax = func.multiply_attention(xt, att, None)
    alpha = func.alpha_train if opt['no_alpha_sigmoid'] else torch.sigmoid(func.alpha_train)
    f = alpha * (ax - xt)
    if opt['add_source']:
        f = f + func.beta_train * func.x0
    return f, att, prods


def _spans(prods, att, ei, norm_idx):
    """(largest max/min of the scores within a group, the same of the attention), over the
    groups of at least two edges."""
    s_span = a_span = 1.0
    for b in range(prods.shape[0]):
        idx = ei[b, norm_idx]
        for n in np.unique(idx):
            sel = idx == n
            if sel.sum() < 2:
                continue
            for h in range(prods.shape[2]):
                s, a = prods[b, sel, h], att[b, sel, h]
                s_span = max(s_span, float(s.max() / s.min()))
                a_span = max(a_span, float(a.max() / a.min()))
    return s_span, a_span


def hub_graph(rng, N, E, hub, n_in):
    """One destination with n_in in-edges; the last node has no edge at all."""
    src = rng.integers(0, N - 1, size=E)
    dst = rng.integers(0, N - 1, size=E)
    dst[:n_in] = hub
    perm = rng.permutation(E)
    return np.stack([src[perm], dst[perm]])[None].astype(np.int64)


def run_case(name, rng, B, N, E, F, P, labels, heads, att_dim, norm_idx, grads=False, square_plus=False,
             add_source=False, no_alpha_sigmoid=False, alpha=0.2, beta=0.5, wstd=0.3, ei=None, **gkw):
    C = F + P + labels
    opt = _opt(C, F, P, heads, att_dim, norm_idx, add_source, no_alpha_sigmoid)
    draws = 0
    while True:
        draws += 1
        assert draws < 200, name
        ei_d = gg.random_graph(rng, B, N, E, **gkw) if ei is None else ei
        x = f32(rng.standard_normal((B, N, C)))
        x0 = f32(rng.standard_normal((B, N, C)))
        gout = f32(rng.standard_normal((B, N, C)))
        Pm = dict(alpha=float(np.float32(alpha)), beta=float(np.float32(beta)))
        for w, b, width in (('Wqx', 'bqx', C - P), ('Wkx', 'bkx', C - P), ('Wqp', 'bqp', P), ('Wkp', 'bkp', P)):
            Pm[w] = f32(rng.standard_normal((att_dim, width)) * wstd)
            Pm[b] = f32(rng.standard_normal((att_dim,)) * wstd)
        out = {}
        for dt, tag in ((torch.float64, ''), (torch.float32, '_ref32')):
            func, lay = _func(opt, C, dt, Pm, ei_d, x0)
            with torch.no_grad():
                f, att, prods = _forward(func, lay, torch.from_numpy(x).to(dt), square_plus)
            out['f' + tag], out['attention' + tag], out['prods' + tag] = f.numpy(), att.numpy(), prods.numpy()
        e_att = float(np.abs(out['attention_ref32'].astype(np.float64) - out['attention']).max())
        e_f = float(np.abs(out['f_ref32'].astype(np.float64) - out['f']).max() / np.abs(out['f']).max())
        s_span, a_span = _spans(out['prods'], out['attention'], ei_d, norm_idx)
        if e_att > FP32_BAR or e_f > FP32_BAR or s_span < SPAN_MIN or a_span < 2.0:
            continue
        margin = None
        if square_plus and grads:
            margin = gg_margin(out['prods'])
            if min(margin) < MARGIN_MIN:
                continue
        break
    meta = dict(name=name, B=B, N=N, E=int(ei_d.shape[2]), C=C, F=F, P=P, labels=labels, heads=heads,
                attention_dim=att_dim, attention_norm_idx=norm_idx, add_source=add_source,
                no_alpha_sigmoid=no_alpha_sigmoid, square_plus=square_plus, output_var_x=OVX, lengthscale_x=LSX,
                output_var_p=OVP, lengthscale_p=LSP, has_grad=bool(grads), draws=draws, fp32_attention_err=e_att,
                fp32_f_rel_err=e_f, score_span=s_span, attention_span=a_span, max_margin=margin)
    arrays = dict(edge_index=ei_d, x=x, x0=x0, alpha_train=f32(Pm['alpha']), beta_train=f32(Pm['beta']),
                  f=out['f'], attention=out['attention'], prods=out['prods'])
    arrays.update({n: Pm[n] for n in PNAMES})
    if grads:
        func, lay = _func(opt, C, torch.float64, Pm, ei_d, x0)
        xt = torch.from_numpy(x).double().requires_grad_(True)
        go = torch.from_numpy(gout).double()
        named = [('x', xt), ('alpha_train', func.alpha_train), ('beta_train', func.beta_train),
                 ('Wqx', lay.Qx.weight), ('bqx', lay.Qx.bias), ('Wkx', lay.Kx.weight), ('bkx', lay.Kx.bias),
                 ('Wqp', lay.Qp.weight), ('bqp', lay.Qp.bias), ('Wkp', lay.Kp.weight), ('bkp', lay.Kp.bias),
                 ('output_var_x', lay.output_var_x), ('lengthscale_x', lay.lengthscale_x),
                 ('output_var_p', lay.output_var_p), ('lengthscale_p', lay.lengthscale_p)]
        arrays.update(gg._grads(lambda: (_forward(func, lay, xt, square_plus)[0] * go).sum(), named))
        arrays['gout'] = gout
    np.savez_compressed(os.path.join(OUT_DIR, name + '.npz'), meta=json.dumps(meta), **arrays)
    return meta, ei_d


def gg_margin(prods):
    """Per batch element: the largest score minus the next distinct one (gen_golden_squareplus._margin)."""
    out = []
    for pb in prods:
        v = np.sort(np.asarray(pb, np.float64).reshape(-1))
        top = v[-1]
        rest = v[v < top - 1e-9 * max(1.0, abs(top))]
        out.append(float(top - rest[-1]) if rest.size else float('inf'))
    return out


def reference_state_dict_keys():
    """The reference layer's own state_dict keys, in registration order (data)."""
    opt = _opt(11, 6, 5, 2, 8, 0, False, False)
    lay = ref_att.SpGraphTransAttentionLayer(11, 11, opt, 'cpu')
    return list(lay.state_dict().keys())


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    rng = np.random.default_rng(20261020)
    cases = {}

    def add(meta):
        cases[meta['name']] = meta

    m, ei = run_case('team_n0', rng, 1, 48, 300, 6, 5, 0, 2, 8, 0, grads=True)
    add(m)
    add(run_case('team_n1', rng, 1, 48, 300, 6, 5, 0, 2, 8, 1, grads=True, ei=ei)[0])
    add(run_case('labels', rng, 1, 48, 300, 6, 5, 3, 2, 8, 1, grads=True)[0])
    add(run_case('lane', rng, 2, 40, 200, 4, 3, 0, 1, 6, 0, grads=True)[0])
    add(run_case('wide', rng, 1, 48, 300, 8, 8, 0, 8, 128, 1, wstd=0.1)[0])
    add(run_case('hub', rng, 1, 64, 600, 6, 5, 0, 2, 8, 1, grads=True, ei=hub_graph(rng, 64, 600, 7, 300))[0])
    m, ei = run_case('sp_n0', rng, 1, 48, 300, 6, 5, 0, 2, 8, 0, grads=True, square_plus=True)
    add(m)
    add(run_case('sp_n1', rng, 1, 48, 300, 6, 5, 0, 2, 8, 1, grads=True, square_plus=True, ei=ei)[0])
    add(run_case('src', rng, 1, 48, 300, 6, 5, 0, 2, 8, 1, add_source=True, no_alpha_sigmoid=True, alpha=0.8,
                 beta=-0.3)[0])
    with open(os.path.join(OUT_DIR, 'meta.json'), 'w') as fh:
        json.dump(dict(state_dict_keys=reference_state_dict_keys(), fp32_bar=FP32_BAR, span_min=SPAN_MIN,
                       cases=cases), fh, indent=1, sort_keys=True)
    print('wrote', len(cases), 'fixtures to', OUT_DIR)
    for n, m in cases.items():
        print('%-8s draws %3d fp32 att %.2e f %.2e span %.3g att span %.3g' % (
            n, m['draws'], m['fp32_attention_err'], m['fp32_f_rel_err'], m['score_span'], m['attention_span']))


if __name__ == '__main__':
    main()
