"""Drop-in ODEFuncAtt and SpGraphAttentionLayer
(reference src/function_GAT_attention.py:9-139).

Selected by ``set_function`` for ``opt['function'] == 'GAT'`` when the option
dict also sets ``opt['gnpde_gat'] = True`` (model_configurations.py; without the
key the registry raises NotImplementedError as before — INTEGRATION.md).

Per RHS evaluation the reference projects wx = x W (:123), gathers wx[src] and
wx[dst] per edge and head, scores LeakyReLU(a . [wx_src | wx_dst]) (:131-134),
runs utils.softmax over ``edge_index[:, attention_norm_idx]`` (:135) and
densifies the head-mean attention into [B,N,N] for a dense matmul (:40-47).

The score decomposes into per-node scalars — with dk = attention_dim / heads and
the same ``a`` for every head,

    sl[n,h] = sum_d a[d]      wx[n,h,d],     sr[n,h] = sum_d a[dk+d] wx[n,h,d],
    s[e,h]  = LeakyReLU(sl[src,h] + sr[dst,h]),

so [sl | sr] = x U with U [C, 2h] = W folded with a.  One RHS here is:

1. node scores: U formed on the device, then one pass over x (fp64 sums,
   gnpde_gat_scores_f32): no wx, no per-edge q/k gathers;
2. softmax statistics (max, 1/sum-exp) of the groups — the CSR rows for
   attention_norm_idx 0, the CSC for 1 — by the statistics kernel in score mode
   GAT (gnpde_seg_softmax_f32: hub chunks, long items);
3. K1, the gather-aggregate with the RHS / Runge-Kutta epilogue fused, forming
   each edge's head-mean weight in its gather loop (gnpde_attn_gat_rhs_f32), or
   the edge-parallel weights pass (gnpde_attn_weights_f32) and the plain K1 —
   the same bits; the fused pass is taken where it measured faster on the benchmark
   graph (ops.gat_fuse_default; GNPDE_GAT_FUSE=1 / 0 forces either).

``Wout`` is dead for ``mix_features=False`` (:38 is the only use) and is never
read; the parameter exists for state_dict compatibility and gets no gradient.
``mix_features=True`` is out of scope and ``multi_modal=True`` calls
``torch.nn.softmax``, which does not exist (:121): both raise
NotImplementedError.

Gradients: with autograd recording the layer's forward is ``_GatEdgeAttention``
— the same forward kernels, and a backward of graph passes: edge-softmax
backward per group, the LeakyReLU derivative per edge
(gnpde_gat_score_backward_f32), segment sums over the CSR (d sl) and the CSC
(d sr), gx = [dsl | dsr] U^T, dU as fp64 weighted column sums of x, and dU
unfolded into dW and da in fp64 torch ([C, 2h]-sized products).  The ODEFunc
composes it with the Laplacian RHS autograd, as ODEFuncTransformerAtt does.
Pinned by fp64 autograd fixtures of the reference layer's forward
(tests/golden/gat/gatgrad_*.npz; tests/golden/gen_golden_gat.py says why the dense
product is rebuilt there: torch's backward of the reference's permuted sparse
tensor is not the derivative of its forward).
"""
import torch
from torch import nn

from . import ops
from .base_classes import ODEFunc, _tensor_key
from .utils import MaxNFEException


def _check_supported(opt):
    if opt.get('mix_features', False):
        raise NotImplementedError("gnpde: function 'GAT' with mix_features=True is out of scope")
    if opt.get('multi_modal', False):
        raise NotImplementedError("gnpde: multi_modal is broken in the reference (torch.nn.softmax, "
                                  "function_GAT_attention.py:121) and out of scope")


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


def fold(W, a, heads):
    """U [C, 2h] fp64: W [C, att] folded with a [2dk] (the layout of gnpde_gat_scores_f32)."""
    C, att = W.shape
    dk = att // heads
    Wh = W.double().view(C, heads, dk)
    av = a.double().reshape(-1)
    return torch.cat([Wh @ av[:dk], Wh @ av[dk:]], 1)


class _GatEdgeAttention(torch.autograd.Function):
    """attention [B,E,h] (COO) = SpGraphAttentionLayer.forward's first output as a
    function of (x, W, a); backward in graph passes."""

    @staticmethod
    def forward(ctx, x, W, a, layer, g, norm_idx):
        ns = layer.node_scores(g, x.detach())
        m, rl = ops.softmax_stats(g, ns, norm_idx)
        att = ops.edge_attention(g, ns, m, rl, norm_idx)
        ctx.save_for_backward(x, W, a, att)
        ctx.g, ctx.ns, ctx.norm_idx, ctx.heads = g, ns, norm_idx, layer.h
        return att

    @staticmethod
    def backward(ctx, g_att):
        x, W, a, att = ctx.saved_tensors
        g, ns, norm_idx, H = ctx.g, ctx.ns, ctx.norm_idx, ctx.heads
        x, W, a = x.detach(), W.detach(), a.detach()
        grouped = g.csr if norm_idx == 0 else g.csc
        gs = ops.softmax_backward(grouped, att, g_att.float())
        ge = ops.gat_score_backward(g, ns, gs)
        gsp = torch.cat([ops.segment_sum(g.csr, ge), ops.segment_sum(g.csc, ge)], 1)     # [R,2h] = [dsl | dsr]
        B, N, C = g.B, g.N, x.shape[-1]
        U = fold(W, a, H)                                                                # [C,2h]
        zero = torch.zeros(B, C, dtype=torch.float64, device=x.device)
        gx = ops.score_input_grad(gsp, U.unsqueeze(0).expand(B, C, 2 * H), g.indeg, zero, B, N, C).view(x.shape)
        gU = ops.wcolsum(x, B, N, gsp)[:, :, :C].sum(0).t()                              # [C,2h]
        dk = W.shape[1] // H
        av = a.double().reshape(-1)
        Wh = W.double().view(C, H, dk)
        gW = gU[:, :H, None] * av[:dk] + gU[:, H:, None] * av[dk:]                       # [C,h,dk]
        ga = torch.cat([torch.einsum('ch,chd->d', gU[:, :H], Wh), torch.einsum('ch,chd->d', gU[:, H:], Wh)])
        return gx, gW.reshape(W.shape).to(W.dtype), ga.reshape(a.shape).to(a.dtype), None, None, None


class SpGraphAttentionLayer(nn.Module):
    """Sparse GAT layer, src/function_GAT_attention.py:74-139 (https://arxiv.org/abs/1710.10903)."""

    def __init__(self, in_features, out_features, opt, device, concat=True):
        super(SpGraphAttentionLayer, self).__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.alpha = opt['leaky_relu_slope']
        self.concat = concat
        self.device = device
        self.opt = opt
        self.h = int(opt['heads'])
        self.attention_dim = opt.get('attention_dim', out_features)
        assert self.attention_dim % self.h == 0, "Number of heads must be a factor of the dimension size"
        self.d_k = self.attention_dim // self.h
        _check_supported(opt)
        self.W = nn.Parameter(torch.zeros(size=(in_features, self.attention_dim)))
        nn.init.xavier_normal_(self.W.data, gain=1.414)
        self.Wout = nn.Parameter(torch.zeros(size=(self.attention_dim, self.in_features)))
        nn.init.xavier_normal_(self.Wout.data, gain=1.414)
        self.a = nn.Parameter(torch.zeros(size=(1, 2 * self.d_k, 1, 1)))
        nn.init.xavier_normal_(self.a.data, gain=1.414)
        self.leakyrelu = nn.LeakyReLU(self.alpha)
        self._graph = None
        self._graph_key = None
        self._folded = None  # (param versions, (W, a flat, the device scratch holding U))

    def graph_for(self, x, edge):
        key = (_tensor_key(edge), int(x.shape[1]))
        if self._graph is None or key != self._graph_key:
            self._graph = ops.GraphCSR(edge, int(x.shape[1]), chunk=self.opt.get('gnpde_chunk'))
            self._graph_key = key
        return self._graph

    def folded(self, x, B):
        """(W, a [2dk], U scratch) cached per parameter version and state shape: the
        operands gnpde_gat_scores_f32 folds into U on the device (stable buffers, so
        captured step graphs keep replaying)."""
        key = (_tensor_key(self.W), _tensor_key(self.a), int(B), int(x.shape[-1]), str(x.device))
        if self._folded is None or self._folded[0] != key:
            self._folded = (key, (self.W.detach().contiguous(), self.a.detach().reshape(-1).contiguous(),
                                  ops.gat_workspace(x, B)))
        return self._folded[1]

    def node_scores(self, g, x):
        """NodeScores of mode SCORE_GAT for this RHS evaluation (x fp32)."""
        W, a, ws = self.folded(x, g.B)
        return ops.gat_scores(g, x, W, a, self.h, self.alpha, ws=ws)

    def forward(self, x, edge, y=None):
        """Returns (attention [B,E,h], None): the per-edge softmax attention of :135
        in COO order.  ``wx`` (:123) is not materialised (dead for mix_features=False)."""
        g = self.graph_for(x, edge)
        norm_idx = int(self.opt['attention_norm_idx'])
        if _needs_grad(x, self.W, self.a):
            return _GatEdgeAttention.apply(x, self.W, self.a, self, g, norm_idx), None
        ns = self.node_scores(g, x.float())
        m, rl = ops.softmax_stats(g, ns, norm_idx)
        return ops.edge_attention(g, ns, m, rl, norm_idx), None

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class ODEFuncAtt(ODEFunc):
    """src/function_GAT_attention.py:9-71."""

    def __init__(self, in_features, out_features, opt, device):
        super(ODEFuncAtt, self).__init__(opt, device)
        self.in_features = in_features
        self.out_features = out_features
        self.multihead_att_layer = SpGraphAttentionLayer(in_features, out_features, opt, device)
        if device is not None:
            self.multihead_att_layer = self.multihead_att_layer.to(device)
        self.attention_dim = opt.get('attention_dim', out_features)
        assert self.attention_dim % opt['heads'] == 0, "Number of heads must be a factor of the dimension size"
        self.d_k = self.attention_dim // opt['heads']
        self.y = None

    def multiply_attention(self, x, attention, wx=None):
        """A_mean x with attention [B,E,h] given explicitly (:40-47)."""
        g = self.graph_for(x)
        w = g.gather_weights(attention.detach().float())
        return ops.spmm_rhs(g, w, x, rhs=False)

    def rhs_stage(self, t, x, stage):
        """forward(t, x) with the solver's stage combination fused into the
        aggregation epilogue (gnpde.integrator, no-grad solvers)."""
        self._rhs(x, stage)

    def graph_capture_state(self, x):
        """What a captured fused step reads (gnpde.integrator._capture_state): the
        device CSR / CSC + plans, the layer's cached operands (W, a and the scratch
        U is folded into) and, with add_source, the stable x0 buffer."""
        g = self.graph_for(x)
        st = [g, self.multihead_att_layer.folded(x, g.B)]
        if self.opt.get('add_source', False):
            st.append(self.stable_x0(x))
        return st

    def supports_node_layout(self):
        """The user numbering is kept (the in-degree node layout is not wired for GAT)."""
        return False

    def supports_feature_padding(self):
        """The node scores read all C columns of the state: no padded columns."""
        return False

    def forward(self, t, x):  # t is needed when called by the integrator
        return self._rhs(x, None)

    def _rhs(self, x, stage):
        if self.nfe > self.opt["max_nfe"]:
            raise MaxNFEException
        self.nfe += 1
        g = self.graph_for(x)
        lay = self.multihead_att_layer
        if stage is None and _needs_grad(x, self.alpha_train, self.beta_train, lay.W, lay.a):
            return self._rhs_autograd(g, x)
        norm_idx = int(self.opt['attention_norm_idx'])
        add_source = bool(self.opt.get('add_source', False))
        if add_source and self.x0 is None:
            raise RuntimeError("ODEFuncAtt: add_source needs x0 (ODEblock.set_x0)")
        # fused stages (and their captured graphs) read a stable x0 buffer (ODEFunc.stable_x0)
        x0 = (self.stable_x0(x) if stage is not None else self.x0) if add_source else None
        if x0 is not None and x0.dtype != x.dtype:
            x0 = x0.to(x.dtype)
        kw = dict(x0=x0, alpha=self.alpha_train.detach(), beta=self.beta_train.detach(),
                  rhs=True, alpha_sigmoid=not self.opt.get('no_alpha_sigmoid', False), add_source=add_source,
                  stage=stage)
        # a bf16 state: scores from an fp32 copy, the weights pass and the bf16 K1 (ops.attn_rhs)
        ns = lay.node_scores(g, x.float() if x.dtype == torch.bfloat16 else x)
        # the fused K1 where it measured faster than the weights pass + K1 (ops.gat_fuse_default)
        return ops.attn_rhs(g, ns, None, None, norm_idx, x, fuse=ops.gat_fuse_default(lay.h, norm_idx), **kw)

    def _rhs_autograd(self, g, x):
        """Training forward: attention [B,E,h] through _GatEdgeAttention, then the
        Laplacian RHS autograd with those weights (head mean), so gradients reach x
        (both paths), alpha, beta, W and a."""
        from .function_laplacian_diffusion import _LaplacianRHS
        att, _ = self.multihead_att_layer(x, self.edge_index)
        add_source = bool(self.opt.get('add_source', False))
        if add_source and self.x0 is None:
            raise RuntimeError("ODEFuncAtt: add_source needs x0 (ODEblock.set_x0)")
        x0 = self.x0 if add_source else None
        if x0 is not None and x0.dtype != torch.float32:
            x0 = x0.float()
        ad = att.detach()
        return _LaplacianRHS.apply(x, self.alpha_train, self.beta_train, att, g, g.gather_weights(ad),
                                   lambda: g.gather_weights(ad, transpose=True), x0,
                                   not self.opt.get('no_alpha_sigmoid', False), add_source)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'
