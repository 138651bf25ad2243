"""Float64 numpy restatement of the transformer ODE function with mix_features (the value
projection), on top of gnpde_oracle.transformer_attention — the reference's pieces composed
as its call site intends (src/function_transformer_attention.py:224-238 the layer's v,
:23-32 multiply_attention(x, attention, values[0]), :52-59 the epilogue):

  v  = x Wv^T + bv                                   [B,N,att]; head h owns columns h*dk .. h*dk+dk-1
  z[b,i,d] = (1/heads) sum_{e: edge[b,0,e] = i} sum_h a[b,e,h] * v[b, edge[b,1,e], h*dk + d]     [B,N,dk]
  ax = z Wout^T + b_out,   f = alpha (ax - x) [+ beta x0]

Duplicate edges add (to_dense of a COO tensor); a row with no edge has z = 0, ax = b_out.
"""
import numpy as np

import gnpde_oracle as O


def values(x, Wv, bv):
    """v = V(x) [B,N,att] fp64 (:226)."""
    return O.project(x, Wv, bv)


def layer_values(v, heads):
    """The layer's returned layout [B,N,dk,h] (:232-238)."""
    return O.split_heads(v, heads)


def head_aggregate(edge_index, att, v):
    """z [B,N,dk]: per-head weights att [B,E,h] over v [B,N,h*dk], head mean (:29-31)."""
    edge_index = np.asarray(edge_index)
    att = np.asarray(att, np.float64)
    v = np.asarray(v, np.float64)
    B, N, A = v.shape
    H = att.shape[2]
    dk = A // H
    vh = v.reshape(B, N, H, dk)
    z = np.zeros((B, N, dk))
    for b in range(B):
        contrib = (att[b][:, :, None] * vh[b][edge_index[b, 1]]).sum(axis=1)     # [E,dk]
        np.add.at(z[b], edge_index[b, 0], contrib)
    return z / H


def multiply_attention(edge_index, att, v, Wout, bout):
    """ax = Wout(z) (:31-32)."""
    return head_aggregate(edge_index, att, v) @ np.asarray(Wout, np.float64).T + np.asarray(bout, np.float64)


def mix_rhs(edge_index, x, x0, Wq, bq, Wk, bk, Wv, bv, Wout, bout, heads, norm_idx, alpha_train, beta_train,
            attention_type='scaled_dot', score_mode='reference', add_source=False, no_alpha_sigmoid=False,
            square_plus=False, output_var=1.0, lengthscale=1.0):
    """(f, attention, v): ODEFuncTransformerAtt.forward under mix_features."""
    att = O.transformer_attention(x, edge_index, Wq, bq, Wk, bk, heads, norm_idx, attention_type, score_mode,
                                  square_plus, output_var, lengthscale)
    v = values(x, Wv, bv)
    ax = multiply_attention(edge_index, att, v, Wout, bout)
    return O.rhs_epilogue(ax, x, x0, alpha_train, beta_train, add_source, no_alpha_sigmoid), att, v


def fixture_rhs(z, x=None):
    """mix_rhs from a loaded fixture (tests/golden/mix/*.npz); x: another state."""
    import json
    m = json.loads(str(z['meta']))
    return mix_rhs(z['edge_index'], z['x'] if x is None else x, z['x0'], z['Wq'], z['bq'], z['Wk'], z['bk'], z['Wv'],
                   z['bv'], z['Wout'], z['bout'], m['heads'], m['attention_norm_idx'], float(z['alpha_train']),
                   float(z['beta_train']), m['attention_type'], m['score_mode'], m['add_source'],
                   m['no_alpha_sigmoid'], m['square_plus'], m['output_var'] or 1.0, m['lengthscale'] or 1.0)
