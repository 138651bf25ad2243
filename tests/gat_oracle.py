"""CPU restatement (float64 numpy) of the GAT attention ODE function — test helper.

Restates the reference's src/function_GAT_attention.py with the oracle's pieces
(gnpde_oracle.edge_softmax, aggregate, rhs_epilogue):

* SpGraphAttentionLayer.forward, :117-136: wx = x W (:123) viewed [B,N,h,dk] (:124),
  edge_e = leakyrelu(sum(a * [wx_src | wx_dst])) (:131-134; the same ``a`` for every
  head), attention = utils.softmax(edge_e, edge[:, attention_norm_idx]) (:135);
* ODEFuncAtt.multiply_attention, :40-47 (mix_features=False): the head-mean attention
  aggregated over edge row 0; ODEFuncAtt.forward, :50-68: the RHS epilogue.

Pinned against the reference's own float64 run by tests/test_gat_oracle_golden.py
(tests/golden/gat/gat_*.npz, tests/golden/gen_golden_gat.py).
"""
import numpy as np

import gnpde_oracle as O


def gat_preact(x, edge_index, W, a, heads):
    """sl[src,h] + sr[dst,h] [B,E,h]: sum(a * edge_h, dim=1) of :131-134 before the LeakyReLU."""
    x = np.asarray(x, np.float64)
    W = np.asarray(W, np.float64)
    a = np.asarray(a, np.float64).reshape(-1)
    edge_index = np.asarray(edge_index)
    B, N, _ = x.shape
    dk = W.shape[1] // heads
    wx = (x @ W).reshape(B, N, heads, dk)                   # :123-124
    sl = wx @ a[:dk]                                        # [B,N,h]
    sr = wx @ a[dk:]
    b = np.arange(B)[:, None]
    return sl[b, edge_index[:, 0]] + sr[b, edge_index[:, 1]]


def gat_attention(x, edge_index, W, a, heads, norm_idx, slope):
    """SpGraphAttentionLayer.forward -> attention [B,E,h] — function_GAT_attention.py:117-136."""
    t = gat_preact(x, edge_index, W, a, heads)
    s = np.where(t > 0, t, float(slope) * t)                # nn.LeakyReLU(slope), :106 / :134
    return O.edge_softmax(s, np.asarray(edge_index)[:, norm_idx], num_nodes=np.shape(x)[1])   # :135


def gat_rhs(edge_index, x, x0, W, a, heads, norm_idx, slope, alpha_train, beta_train, add_source=False,
            no_alpha_sigmoid=False):
    """ODEFuncAtt.forward — function_GAT_attention.py:50-68 with multiply_attention :40-47."""
    att = gat_attention(x, edge_index, W, a, heads, norm_idx, slope)
    ax = O.aggregate(edge_index, att.mean(axis=2), x)       # :47: mean over heads of A_h x
    return O.rhs_epilogue(ax, x, x0, alpha_train, beta_train, add_source, no_alpha_sigmoid)
