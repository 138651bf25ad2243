"""Float64 numpy restatement of the Laplacian ODE function's multi_modal branch (reference
src/function_laplacian_diffusion.py:29-37, :61-77, the softmax read as
``torch.softmax(..., dim=-1)``), on top of gnpde_oracle:

  q = x Wq^T + bq [B,N,C],  k = y Wk^T + bk,  v = y Wv^T + bv [B,M,C]
  x~ = softmax(q k^T / sqrt(C), dim=-1) v
  f  = alpha (A x~ - x~) [+ beta x0]

and its gradients, written out by hand (no autograd):  with g = dL/df, a = alpha,
  g_x~ = a (A^T g - g),   D = rowsum(g_x~ * x~),   dS = P * (g_x~ v^T - D),
  g_q = scale dS k,  g_k = scale dS^T q,  g_v = P^T g_x~,
  g_x = g_q Wq,  g_y = g_k Wk + g_v Wv,  g_W* = g_*^T input,  g_b* = sum g_*.
"""
import json

import numpy as np

import gnpde_oracle as O

PNAMES = ("Wq", "bq", "Wk", "bk", "Wv", "bv")


def _as64(a):
    return np.asarray(a, np.float64)


def cross_attention(q, k, v, scale, lse=False):
    """softmax_m(scale <q_n, k_m>) v [B,N,C] (and max + ln sum exp of the scaled scores [B,N])."""
    q, k, v = _as64(q), _as64(k), _as64(v)
    s = np.einsum('bnc,bmc->bnm', q, k) * float(scale)
    mx = s.max(axis=-1, keepdims=True)
    p = np.exp(s - mx)
    den = p.sum(axis=-1, keepdims=True)
    out = np.einsum('bnm,bmc->bnc', p / den, v)
    if lse:
        return out, (mx + np.log(den))[..., 0]
    return out


def projections(x, y, Wq, bq, Wk, bk, Wv, bv):
    return O.project(x, Wq, bq), O.project(y, Wk, bk), O.project(y, Wv, bv)


def xtilde(x, y, Wq, bq, Wk, bk, Wv, bv):
    """x~ (:61-63); dk = in_features = the width of x."""
    q, k, v = projections(x, y, Wq, bq, Wk, bk, Wv, bv)
    return cross_attention(q, k, v, 1.0 / np.sqrt(np.shape(x)[-1]))


def multimodal_rhs(edge_index, edge_weight, x, y, x0, Wq, bq, Wk, bk, Wv, bv, alpha_train, beta_train,
                   add_source=False, no_alpha_sigmoid=False):
    """(f, x~): LaplacianODEFunc.forward under multi_modal, block 'constant'."""
    xt = xtilde(x, y, Wq, bq, Wk, bk, Wv, bv)
    ax = O.aggregate(edge_index, edge_weight, xt)
    return O.rhs_epilogue(ax, xt, x0, alpha_train, beta_train, add_source, no_alpha_sigmoid), xt


def multimodal_grads(edge_index, edge_weight, x, y, x0, Wq, bq, Wk, bk, Wv, bv, alpha_train, beta_train, gout,
                     add_source=False, no_alpha_sigmoid=False):
    """Gradients of <gout, f> w.r.t. x, y, alpha_train, beta_train and Q2 / K2 / V2 (dict g_*)."""
    x, y, g = _as64(x), _as64(y), _as64(gout)
    Wq, Wk, Wv = _as64(Wq), _as64(Wk), _as64(Wv)
    C = x.shape[-1]
    scale = 1.0 / np.sqrt(C)
    q, k, v = projections(x, y, Wq, bq, Wk, bk, Wv, bv)
    s = np.einsum('bnc,bmc->bnm', q, k) * scale
    p = np.exp(s - s.max(axis=-1, keepdims=True))
    p /= p.sum(axis=-1, keepdims=True)
    xt = np.einsum('bnm,bmc->bnc', p, v)
    a = O.alpha_value(alpha_train, no_alpha_sigmoid)
    lin = O.aggregate(edge_index, edge_weight, xt) - xt                     # A x~ - x~
    ga = float((g * lin).sum())
    if not no_alpha_sigmoid:
        ga *= a * (1.0 - a)
    gb = float((g * _as64(x0)).sum()) if add_source else 0.0
    ei_t = np.asarray(edge_index)[:, ::-1, :]                               # A^T: the edges reversed
    gxt = a * (O.aggregate(ei_t, edge_weight, g) - g)
    dP = np.einsum('bnc,bmc->bnm', gxt, v)
    D = (gxt * xt).sum(axis=-1, keepdims=True)
    dS = p * (dP - D)
    gq = scale * np.einsum('bnm,bmc->bnc', dS, k)
    gk = scale * np.einsum('bnm,bnc->bmc', dS, q)
    gv = np.einsum('bnm,bnc->bmc', p, gxt)
    return dict(g_x=gq @ Wq, g_y=gk @ Wk + gv @ Wv, g_alpha_train=np.array(ga), g_beta_train=np.array(gb),
                g_Wq=np.einsum('bna,bnc->ac', gq, x), g_bq=gq.sum(axis=(0, 1)),
                g_Wk=np.einsum('bma,bmd->ad', gk, y), g_bk=gk.sum(axis=(0, 1)),
                g_Wv=np.einsum('bma,bmd->ad', gv, y), g_bv=gv.sum(axis=(0, 1)))


def _args(z, x=None, y=None):
    m = json.loads(str(z['meta']))
    pos = (z['edge_index'], z['edge_weight'], z['x'] if x is None else x, z['y'] if y is None else y, z['x0']) + \
        tuple(z[n] for n in PNAMES) + (float(z['alpha_train']), float(z['beta_train']))
    return pos, dict(add_source=m['add_source'], no_alpha_sigmoid=m['no_alpha_sigmoid'])


def fixture_rhs(z, x=None, y=None):
    """multimodal_rhs from a loaded fixture (tests/golden/multimodal/*.npz); x / y: other inputs."""
    pos, kw = _args(z, x, y)
    return multimodal_rhs(*pos, **kw)


def fixture_grads(z):
    pos, kw = _args(z)
    return multimodal_grads(*pos, z['gout'], **kw)
