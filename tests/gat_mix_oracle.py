"""CPU restatement (float64 numpy) of the GAT ODE function with mix_features — test helper.

Restates the reference's src/function_GAT_attention.py for ``opt['mix_features']``:

* SpGraphAttentionLayer.forward, :117-136, returns (attention, wx) with wx = x W (:123);
  the attention is gat_oracle.gat_attention (unchanged by mix_features);
* ODEFuncAtt.multiply_attention, :29-38: per head the dense attention A_h multiplies the
  WHOLE wx [B,N,att] (wx.unsqueeze(1) broadcasts over the heads: no per-head slice), the
  heads are averaged (:37) and the result is mapped back by Wout (:38);
* ODEFuncAtt.forward, :60-68: the RHS epilogue.

The heads are aggregated one by one here, as the reference does, so the restatement does
not assume that the head mean commutes with the product (the project's kernels do).

Pinned against the reference's own float64 run by tests/test_gat_mix_oracle_golden.py
(tests/golden/gat_mix/gatmix_*.npz, tests/golden/gen_golden_gat_mix.py).
"""
import numpy as np

import gat_oracle as G
import gnpde_oracle as O


def gat_mix_project(x, W):
    """wx = x W — function_GAT_attention.py:123."""
    return np.asarray(x, np.float64) @ np.asarray(W, np.float64)


def gat_mix_multiply(edge_index, att, wx, Wout):
    """multiply_attention under mix_features — :29-38: mean_h(A_h wx) Wout."""
    att = np.asarray(att, np.float64)
    wx = np.asarray(wx, np.float64)
    heads = att.shape[2]
    acc = np.zeros_like(wx)
    for h in range(heads):                                  # :37, one dense [N,N] product per head
        acc += O.aggregate(edge_index, att[:, :, h], wx)
    return (acc / heads) @ np.asarray(Wout, np.float64)     # :37 mean, :38


def gat_mix_rhs(edge_index, x, x0, W, Wout, a, heads, norm_idx, slope, alpha_train, beta_train, add_source=False,
                no_alpha_sigmoid=False):
    """ODEFuncAtt.forward with mix_features — :50-68 with multiply_attention :29-38."""
    att = G.gat_attention(x, edge_index, W, a, heads, norm_idx, slope)
    ax = gat_mix_multiply(edge_index, att, gat_mix_project(x, W), Wout)
    return O.rhs_epilogue(ax, x, x0, alpha_train, beta_train, add_source, no_alpha_sigmoid)
