"""Float64 numpy restatement of the beltrami exp_kernel attention (the product kernel of
src/function_transformer_attention.py:90-123, :164-216) as its branch means it, on top of
gnpde_oracle's softmax / squareplus, aggregation and epilogue.  With C = hidden_dim, F =
feat_hidden_dim, P = pos_enc_hidden_dim the state columns are [features F | positions P |
labels C - F - P] (GNN.py:23-40, base_classes.py:149-162):

  p  = x[..., F:F+P]                       (the reference writes x[:, F:F+P]: the node axis)
  xf = cat(x[..., :F], x[..., F+P:])       width C - P
  qx, kx = Qx(xf), Kx(xf);  qp, kp = Qp(p), Kp(p)      [B,N,att], head h in columns h*dk ..
  s[b,e,h] = ovx^2 exp(-|qx_src,h - kx_dst,h|^2 / (2 lsx^2)) * ovp^2 exp(-|qp_src,h - kp_dst,h|^2 / (2 lsp^2))
  attention = softmax(s, edge[:, norm_idx, :])          (or squareplus)
  f = alpha (A_mean x - x) [+ beta x0]                  (v = None: the plain aggregation of x)

``folded`` restates the same score through the folded operands q'_h = [qx_h / lsx | qp_h / lsp]
(one exp_kernel of width 2 dk, amplitude ovx ovp, lengthscale 1), what the GPU path computes.
"""
import json

import numpy as np

import gnpde_oracle as O

PNAMES = ("Wqx", "bqx", "Wkx", "bkx", "Wqp", "bqp", "Wkp", "bkp")
SNAMES = ("output_var_x", "lengthscale_x", "output_var_p", "lengthscale_p")


def split_state(x, F, P):
    """(xf [.., C-P], p [.., P]) along the FEATURE axis."""
    x = np.asarray(x, np.float64)
    return np.concatenate([x[..., :F], x[..., F + P:]], axis=-1), x[..., F:F + P]


def projections(x, W, F, P):
    """(qx, kx, qp, kp), each [B,N,att] fp64; W: a mapping with PNAMES."""
    xf, p = split_state(x, F, P)
    return (O.project(xf, W["Wqx"], W["bqx"]), O.project(xf, W["Wkx"], W["bkx"]),
            O.project(p, W["Wqp"], W["bqp"]), O.project(p, W["Wkp"], W["bkp"]))


def _sqdist(q, k, edge_index, heads):
    """[B,E,h]: |q_src,h - k_dst,h|^2."""
    B, N, A = q.shape
    dk = A // heads
    out = np.empty((B, edge_index.shape[2], heads))
    for b in range(B):
        d = q[b][edge_index[b, 0]] - k[b][edge_index[b, 1]]
        out[b] = (d.reshape(-1, heads, dk) ** 2).sum(axis=2)
    return out


def scores(x, edge_index, W, heads, F, P, ovx, lsx, ovp, lsp):
    """prods [B,E,h] (:211-214), the literal product of the two kernels."""
    edge_index = np.asarray(edge_index)
    qx, kx, qp, kp = projections(x, W, F, P)
    return (ovx ** 2 * np.exp(-_sqdist(qx, kx, edge_index, heads) / (2 * lsx ** 2)) *
            ovp ** 2 * np.exp(-_sqdist(qp, kp, edge_index, heads) / (2 * lsp ** 2)))


def folded(x, W, heads, F, P, lsx, lsp):
    """(q', k') [B,N,2 att]: head h owns columns h*2dk ..: [qx_h / lsx | qp_h / lsp]."""
    qx, kx, qp, kp = projections(x, W, F, P)
    B, N, A = qx.shape
    dk = A // heads

    def cat(a, b):
        return np.concatenate([a.reshape(B, N, heads, dk) / lsx, b.reshape(B, N, heads, dk) / lsp],
                              axis=3).reshape(B, N, 2 * A)
    return cat(qx, qp), cat(kx, kp)


def scores_folded(x, edge_index, W, heads, F, P, ovx, lsx, ovp, lsp):
    """The same prods as one exp_kernel over (q', k'): (ovx ovp)^2 exp(-|q' - k'|^2 / 2)."""
    q, k = folded(x, W, heads, F, P, lsx, lsp)
    return (ovx * ovp) ** 2 * np.exp(-_sqdist(q, k, np.asarray(edge_index), heads) / 2)


def attention(x, edge_index, W, heads, F, P, ovx, lsx, ovp, lsp, norm_idx, square_plus=False):
    s = scores(x, edge_index, W, heads, F, P, ovx, lsx, ovp, lsp)
    N = np.asarray(x).shape[1]
    index = np.asarray(edge_index)[:, norm_idx, :]
    return O.squareplus(s, index, N) if square_plus else O.edge_softmax(s, index, N)


def rhs(edge_index, x, x0, W, heads, F, P, ovx, lsx, ovp, lsp, norm_idx, alpha_train, beta_train,
        add_source=False, no_alpha_sigmoid=False, square_plus=False):
    """(f, attention, prods): ODEFuncTransformerAtt.forward over the beltrami product kernel."""
    s = scores(x, edge_index, W, heads, F, P, ovx, lsx, ovp, lsp)
    N = np.asarray(x).shape[1]
    index = np.asarray(edge_index)[:, norm_idx, :]
    att = O.squareplus(s, index, N) if square_plus else O.edge_softmax(s, index, N)
    ax = O.aggregate(edge_index, att.mean(axis=2), x)
    return O.rhs_epilogue(ax, x, x0, alpha_train, beta_train, add_source, no_alpha_sigmoid), att, s


def fixture_args(z, norm_idx=None, **over):
    """rhs's arguments from a loaded fixture (tests/golden/beltrami/*.npz); ``over``: other scalars."""
    m = json.loads(str(z["meta"]))
    sc = dict(ovx=m["output_var_x"], lsx=m["lengthscale_x"], ovp=m["output_var_p"], lsp=m["lengthscale_p"])
    sc.update(over)
    return m, dict(W={n: z[n] for n in PNAMES}, heads=m["heads"], F=m["F"], P=m["P"],
                   norm_idx=m["attention_norm_idx"] if norm_idx is None else norm_idx,
                   alpha_train=float(z["alpha_train"]), beta_train=float(z["beta_train"]),
                   add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"],
                   square_plus=m["square_plus"], **sc)


def fixture_rhs(z, x=None, **over):
    m, kw = fixture_args(z, **over)
    return rhs(z["edge_index"], z["x"] if x is None else x, z["x0"], **kw)


def score_grad_split(edge_index, q, k, gs, H, dk, dk_split, p0, p1=1.0):
    """fp64 reference of ops.score_grad_split for one batch element: q, k [N, H*dk], gs [E,H],
    edge_index [2,E] -> (g_q, g_k, S0, S1, S2) with s = p0^2 exp(-|q - k|^2 / (2 p1^2)) per head,
    S0 = sum gs 2 s / p0, S1 / S2 = sum gs s |q - k|^2 / p1^2 over the first dk_split / the other
    elements of each head."""
    q, k, gs = (np.asarray(a, np.float64) for a in (q, k, gs))
    src, dst = np.asarray(edge_index)
    d = (q[src] - k[dst]).reshape(-1, H, dk)
    da, db = (d[:, :, :dk_split] ** 2).sum(axis=2), (d[:, :, dk_split:] ** 2).sum(axis=2)
    s = p0 ** 2 * np.exp(-(da + db) / (2 * p1 ** 2))
    ge = (-(gs * s)[:, :, None] * d / p1 ** 2).reshape(-1, H * dk)   # dL/dq per edge; dL/dk = -that
    gq, gk = np.zeros_like(q), np.zeros_like(k)
    np.add.at(gq, src, ge)
    np.add.at(gk, dst, -ge)
    return gq, gk, (gs * 2 * s / p0).sum(), (gs * s * da).sum() / p1 ** 2, (gs * s * db).sum() / p1 ** 2
