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
read there; the parameter exists for state_dict compatibility and gets no gradient.
``multi_modal=True`` calls ``torch.nn.softmax``, which does not exist (:121), and
raises NotImplementedError.

``mix_features=True`` (the value projection, :29-38) runs when the option dict also
sets ``opt['gnpde_gat_mix_features'] = True`` (NotImplementedError without the key,
fp32 states only).  The reference aggregates the projected features per head and maps
them back, wx = mean_h(A_h (x W)), ax = wx Wout.  Every head's attention multiplies
the whole wx (not a per-head slice), so the head mean commutes with the product and

    f = a ((A_mean (x W)) Wout - x) + b x0

with the head-mean attention A_mean of steps 1-3.  One RHS is then: the node scores
and statistics as above (still from x U: wx is not needed for them), wx = x W
(gnpde_linear_f32), z = A_mean wx by the GAT-weight K1 at width attention_dim with no
epilogue, and gnpde_linear_rhs_f32: z Wout with the RHS epilogue fused.  The kernel also
fuses the fixed-grid Runge-Kutta stage combination (the same bits as f followed by
gnpde_stage_apply_f32); the solvers' stages take the two passes, which measured faster
(DESIGN.md §6.15), as the adaptive stages do.
W^T and Wout^T are cached per parameter version (stable buffers for captured graphs).

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
tensor is not the derivative of its forward).  Under mix_features the RHS autograd is
``_GatMixRHS`` instead of the Laplacian one: gradients also reach ``Wout``, and ``W``
through the value path (tests/golden/gat_mix/gatmixgrad_*.npz).
"""
import torch
from torch import nn

from . import ops
from .base_classes import ODEFunc, _tensor_key
from .utils import MaxNFEException


def _check_supported(opt):
    if opt.get('mix_features', False) and not opt.get('gnpde_gat_mix_features', False):
        raise NotImplementedError("gnpde: function 'GAT' with mix_features=True (the value projection, "
                                  "function_GAT_attention.py:29-38) is opt-in: set "
                                  "opt['gnpde_gat_mix_features'] = True to select it")
    if opt.get('multi_modal', False):
        raise NotImplementedError("gnpde: multi_modal is broken in the reference (torch.nn.softmax, "
                                  "function_GAT_attention.py:121) and out of scope for the GAT function "
                                  "(opt['gnpde_multi_modal'] serves function='laplacian' under block='constant' only)")


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


class _GatProject(torch.autograd.Function):
    """wx = x W (:123) on the matrix cores, with its backward (mix_features)."""

    @staticmethod
    def forward(ctx, x, W, Wt):
        ctx.save_for_backward(x, W)
        return ops.linear(x.detach(), Wt)[0].view(tuple(x.shape[:-1]) + (W.shape[1],))

    @staticmethod
    def backward(ctx, g_wx):
        x, W = ctx.saved_tensors
        g_wx = g_wx.contiguous()
        gx = ops.linear(g_wx, W.detach())[0].view(x.shape) if ctx.needs_input_grad[0] else None
        gW = ops.linear_wgrad(x.detach(), g_wx) if ctx.needs_input_grad[1] else None
        return gx, gW, None


class _GatMixRHS(torch.autograd.Function):
    """f = a ((A_mean (x W)) Wout - x) [+ b x0] as a function of (x, alpha, beta,
    attention, W, Wout): the forward kernels of the no-grad path, and a backward of
    existing passes.  With g = dL/df and gh = a g:
      gWout = z^T gh, g_z = gh Wout^T, g_wx = A_mean^T g_z (K1 over the CSC),
      g_att[e,h] = <g_z[src], wx[dst]> / H, gW = x^T g_wx, g_x = -gh + g_wx W^T,
      g_alpha, g_beta by fp64 dots (as the Laplacian RHS)."""

    @staticmethod
    def forward(ctx, x, alpha_train, beta_train, att, W, Wout, g, Wt, Wot, x0, alpha_sigmoid, add_source):
        xd, ad = x.detach(), att.detach()
        wx = ops.linear(xd, Wt)[0].view(g.B, g.N, W.shape[1])
        z = ops.spmm_rhs(g, g.gather_weights(ad), wx, rhs=False)
        f = ops.linear_rhs(z, Wot, xd, x0=x0, alpha=alpha_train.detach(), beta=beta_train.detach(), rhs=True,
                           alpha_sigmoid=alpha_sigmoid, add_source=add_source)
        ctx.save_for_backward(x, alpha_train, beta_train, att, W, Wout, wx, z)
        ctx.g, ctx.Wot, ctx.x0 = g, Wot, x0
        ctx.alpha_sigmoid, ctx.add_source = alpha_sigmoid, add_source
        return f

    @staticmethod
    def backward(ctx, gf):
        x, alpha_train, beta_train, att, W, Wout, wx, z = ctx.saved_tensors
        g = ctx.g
        gf = gf.contiguous()
        x, W, Wout, ad = x.detach(), W.detach(), Wout.detach(), att.detach()
        al = alpha_train.detach()
        a = torch.sigmoid(al) if ctx.alpha_sigmoid else al
        gh = (a.float() * gf).contiguous()
        need = ctx.needs_input_grad
        gx = ga = gb = gatt = gW = gWout = None
        if need[5]:
            gWout = ops.linear_wgrad(z, gh).to(Wout.dtype)                     # [att, C] = z^T gh
        if need[0] or need[3] or need[4]:
            g_z = ops.linear(gh, Wout)[0]                                      # [R, att] = gh Wout^T
            if need[3]:
                gatt = ops.sddmm(g, g_z, wx, heads=att.shape[2]).view(att.shape)
            if need[0] or need[4]:
                g_wx = ops.spmm_rhs(g, g.gather_weights(ad, transpose=True), g_z.view(wx.shape), rhs=False,
                                    transpose=True)
                if need[4]:
                    gW = ops.linear_wgrad(x, g_wx).to(W.dtype)                 # [C, att] = x^T g_wx
                if need[0]:
                    gx = ops.linear(g_wx, W)[0].view(x.shape) - gh             # g_wx W^T - gh
        if need[1]:
            one = torch.ones((), dtype=torch.float32, device=x.device)
            d = ops.linear_rhs(z, ctx.Wot, x, alpha=one, rhs=True, alpha_sigmoid=False)   # ax - x
            s = ops.dot(gf, d).to(alpha_train.dtype)  # fp64 accumulation, fixed order
            if ctx.alpha_sigmoid:
                sg = torch.sigmoid(al)
                s = s * sg * (1 - sg)
            ga = s.reshape(alpha_train.shape)
        if need[2]:
            if ctx.add_source:
                gb = ops.dot(gf, ctx.x0.float()).to(beta_train.dtype).reshape(beta_train.shape)
            else:
                gb = torch.zeros_like(beta_train)
        return gx, ga, gb, gatt, gW, gWout, None, None, None, None, None, None


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
        self.mix = bool(opt.get('mix_features', False))
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
        self._transposed = None  # (param versions, (W^T, Wout^T)): mix_features

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

    def transposed(self):
        """(W^T [att, C], Wout^T [C, att]) contiguous, cached per parameter version: the
        [Nout, K] operands of the two products of mix_features (stable buffers, so
        captured step graphs keep replaying)."""
        key = (_tensor_key(self.W), _tensor_key(self.Wout))
        if self._transposed is None or self._transposed[0] != key:
            self._transposed = (key, (self.W.detach().t().contiguous(), self.Wout.detach().t().contiguous()))
        return self._transposed[1]

    def project(self, x):
        """wx = x W (:123) [.., attention_dim] fp32 (mix_features)."""
        if x.dtype != torch.float32:
            raise NotImplementedError("gnpde: GAT mix_features runs on fp32 states only (got %s)" % x.dtype)
        Wt, _ = self.transposed()
        if _needs_grad(x, self.W):
            return _GatProject.apply(x, self.W, Wt)
        return ops.linear(x, Wt)[0].view(tuple(x.shape[:-1]) + (self.attention_dim,))

    def node_scores(self, g, x):
        """NodeScores of mode SCORE_GAT for this RHS evaluation (x fp32)."""
        W, a, ws = self.folded(x, g.B)
        return ops.gat_scores(g, x, W, a, self.h, self.alpha, ws=ws)

    def forward(self, x, edge, y=None):
        """Returns (attention [B,E,h], wx): the per-edge softmax attention of :135 in COO
        order, and wx = x W (:123) under mix_features — None otherwise (dead there, not
        materialised)."""
        g = self.graph_for(x, edge)
        norm_idx = int(self.opt['attention_norm_idx'])
        wx = self.project(x) if self.mix else None
        if _needs_grad(x, self.W, self.a):
            return _GatEdgeAttention.apply(x, self.W, self.a, self, g, norm_idx), wx
        ns = self.node_scores(g, x.float())
        m, rl = ops.softmax_stats(g, ns, norm_idx)
        return ops.edge_attention(g, ns, m, rl, norm_idx), wx

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
        """A_mean x with attention [B,E,h] given explicitly (:40-47); under mix_features
        (A_mean wx) Wout (:29-38), wx = x W when not given."""
        g = self.graph_for(x)
        w = g.gather_weights(attention.detach().float())
        lay = self.multihead_att_layer
        if not lay.mix:
            return ops.spmm_rhs(g, w, x, rhs=False)
        if wx is None:
            wx = lay.project(x)
        z = ops.spmm_rhs(g, w, wx.detach().float().view(g.B, g.N, lay.attention_dim), rhs=False)
        return ops.linear_rhs(z, lay.transposed()[1], x.detach(), rhs=False)

    def rhs_stage(self, t, x, stage):
        """forward(t, x) with the solver's stage combination fused into the
        aggregation epilogue (gnpde.integrator, no-grad solvers)."""
        self._rhs(x, stage)

    def graph_capture_state(self, x):
        """What a captured fused step reads (gnpde.integrator._capture_state): the
        device CSR / CSC + plans, the layer's cached operands (W, a and the scratch
        U is folded into) and, with add_source, the stable x0 buffer."""
        g = self.graph_for(x)
        lay = self.multihead_att_layer
        st = [g, lay.folded(x, g.B)]
        if lay.mix:
            st.append(lay.transposed())
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
        if lay.mix and x.dtype != torch.float32:
            raise NotImplementedError("gnpde: GAT mix_features runs on fp32 states only (got %s)" % x.dtype)
        if stage is None and _needs_grad(x, self.alpha_train, self.beta_train, lay.W, lay.a,
                                         lay.Wout if lay.mix else None):
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
        if lay.mix:
            # the value projection: z = A_mean (x W) by the GAT-weight K1 at width attention_dim
            # (no epilogue), then z Wout with the RHS / stage epilogue fused (ops.linear_rhs)
            Wt, Wot = lay.transposed()
            wx = ops.linear(x, Wt)[0].view(g.B, g.N, lay.attention_dim)
            z = ops.attn_rhs(g, ns, None, None, norm_idx, wx, rhs=False, fuse=ops.gat_fuse_default(lay.h, norm_idx))
            # a solver stage takes f + the stage pass: the same bits as the kernel's fused stage, and
            # faster on the benchmark graph (0.195-0.211 against 0.212-0.217 ms)
            return ops.linear_rhs(z, Wot, x, fuse=False, **kw)
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
        lay = self.multihead_att_layer
        if lay.mix:  # + Wout, and W through the value path as well (_GatMixRHS)
            Wt, Wot = lay.transposed()
            return _GatMixRHS.apply(x, self.alpha_train, self.beta_train, att, lay.W, lay.Wout, g, Wt, Wot, x0,
                                    not self.opt.get('no_alpha_sigmoid', False), add_source)
        return _LaplacianRHS.apply(x, self.alpha_train, self.beta_train, att, g, g.gather_weights(ad),
                                   lambda: g.gather_weights(ad, transpose=True), x0,
                                   not self.opt.get('no_alpha_sigmoid', False), add_source)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'
