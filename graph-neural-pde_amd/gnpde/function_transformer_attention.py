"""Drop-in ODEFuncTransformerAtt and SpGraphTransAttentionLayer
(reference src/function_transformer_attention.py:9-270).

Per RHS evaluation the reference projects Q/K/V, gathers q[src] and k[dst],
forms an [B,h,E,E] score matmul, runs utils.softmax and densifies the
head-mean attention into [B,N,N] for a dense matmul.  Here one RHS is:

1. node scores — reference ``scaled_dot`` (the fork's global key sum,
   :249 = ``q_src . (sum_e' k_dst(e')) / sqrt(dk)``) needs no
   per-edge work at all: an indegree-weighted column sum of x (fp64), a tiny
   key projection, and one fp64 GEMV per node (gnpde_ref_scores_f32).  The
   per-edge modes (``score_mode='per_edge'`` scaled_dot = upstream GRAND, and
   exp_kernel / cosine_sim / pearson, :246-259) project Q|K with the MFMA
   kernel (gnpde_linear_f32);
2. norm_idx 1: destination-grouped softmax statistics (max, 1/sum-exp)
   over the CSC (K2, gnpde_seg_softmax_f32);
3. head-mean softmax weights in aggregation-CSR order: for norm_idx 0 the
   edge-block segmented-softmax kernel K2 computes them straight from the
   scores (SDDMM + segmented max/sum-exp + head mean in one pass, no [E,h]
   tensor); for norm_idx 1 an edge-parallel pass over the statistics of
   step 2 (gnpde_attn_weights_f32); then the K1 gather-aggregate with the RHS /
   Runge-Kutta epilogue fused (gnpde_spmm_rhs_f32).  With the fork scaled_dot
   and norm_idx 0 every score of a source group is equal, so the weights are
   1/outdeg for any x: computed once per graph.

``square_plus`` (with the opt-in key ``gnpde_square_plus``; the reference's call at
:264 passes a 2-D slice and omits num_nodes) normalises the scores with
``utils.squareplus(prods, edge[:, norm_idx, :], None)`` instead of the softmax:
steps 2-3 become the global score maximum per batch element (gnpde_score_max_f32;
per-edge modes store their scores once), the group sums of p = squareplus(s - M_b)
(gnpde_squareplus_stats_f32; for the fork's scores p is per node) and the
head-mean weights — inside K1 for the fork's scores under norm_idx 1
(gnpde_attn_sp_rhs_f32: no transcendental per edge), else a weights pass
(gnpde_squareplus_weights_f32) + K1.  M, p and the stored scores live in buffers
cached on the layer (``squareplus_buffers``); nothing is read on the host.  The
uniform case keeps its cached 1/outdeg weights.  DESIGN.md §6.12.

V and Wout are dead when ``mix_features=False`` (:33-41) and are never
computed there; the parameters exist for state_dict compatibility.
``mix_features=True`` (the value projection, :23-32) runs when the option dict also sets
``opt['gnpde_mix_features'] = True``: the reference's call site hands
``multiply_attention`` the tuple ``(v, prods)`` (:50), so the option cannot run there, and
the key selects what its pieces compute when composed as intended
(``multiply_attention(x, attention, values[0])``):
  v = V(x) [B,N,att], head h owning columns h*dk .. h*dk+dk-1
  z[b,i,:] = (1/h) sum_{e: row(e) = i} sum_h att[b,e,h] v[b, col(e), h*dk : (h+1)*dk]   [B,N,dk]
  ax = Wout(z),  f = alpha (ax - x) [+ beta x0]
One RHS is then: the node scores and statistics as above, the per-head attention in
aggregation-CSR order [nnz, h] (the attention pass that serves every score mode, grouping
and normaliser, with a CSR-order output; cached for the uniform case), v on the matrix
cores (gnpde_linear_f32), the per-head aggregation (gnpde_head_aggregate_f32,
csrc/head_aggregate.hip: K1's plan items, per-head weights, the heads reduced across
lanes) and Wout with its bias and the RHS / stage epilogue fused
(gnpde_linear_rhs_bias_f32).  fp32 states, one GPU, the user's node numbering.
DESIGN.md §6.16.

The beltrami product kernel (``beltrami`` with ``attention_type='exp_kernel'``, :90-123 and
:164-216) runs when the option dict also sets ``opt['gnpde_beltrami_kernel'] = True``: the
reference slices the node axis where it means the feature axis (:166-167), and the key selects
what the branch means.  With C = hidden_dim, F = feat_hidden_dim, P = pos_enc_hidden_dim and the
state columns [features F | positions P | labels C-F-P]:
  p = x[..., F:F+P],  xf = cat(x[..., :F], x[..., F+P:])
  s[b,e,h] = ovx^2 exp(-|Qx(xf)_src,h - Kx(xf)_dst,h|^2 / (2 lsx^2)) ovp^2 exp(-|Qp(p)_src,h - Kp(p)_dst,h|^2 / (2 lsp^2))
Since the two exponents add to |q' - k'|^2 / 2 with q'_h = [qx_h / lsx | qp_h / lsp], the score is
exp_kernel with heads h, dk' = 2 dk, p0 = ovx ovp, p1 = 1 over ONE folded projection operand
W' [4 att, C] (``fold_beltrami``, cached per parameter version as ``wcat()`` is): every forward
pass above runs unchanged.  Backward (``_BeltramiAttention``): gnpde_score_grad_split_f32 gives
dL/dq', dL/dk' and the per-edge terms of the four scalars' gradients (summed in fp64), the
projection backward runs over W', and ``unfold_beltrami`` takes its result back to Qx / Kx / Qp /
Kp.  Vx, Vp and Wout are dead (v = None, :216).  DESIGN.md §6.22.

Settings the fork cannot execute (``mix_features`` without
``gnpde_mix_features``, ``square_plus`` :264 without ``gnpde_square_plus``, ``multi_modal`` :171/222,
beltrami+exp_kernel :164-167 without ``gnpde_beltrami_kernel``)
raise NotImplementedError.  ``reweight_attention`` is a no-op in the fork (the
layer's ``edge_weights`` is captured as None at construction, :15 / :261) and
is a no-op here.

Gradients: with autograd recording, the layer's forward
is ``_EdgeAttention`` — the same forward kernels, plus a backward made of graph
passes (backward.hip): edge-softmax backward per group, then for the fork's
scaled_dot the node-score / key-sum chain rule (segment sums, fp64 weighted
column sums, a few [att, C] products) and for the per-edge scaled_dot two K1
aggregations per head (q side over the CSR, k side over the CSC) and the
projection backward (MFMA projections for d/dx and d/dW, gnpde_linear_wgrad_f32).  The
transformer ODEFunc then composes it with the Laplacian RHS autograd
(function_laplacian_diffusion._LaplacianRHS), whose weight gradient is an
SDDMM.  exp_kernel / cosine_sim / pearson: one pass per side over the grouped
CSR / CSC turns dL/ds into dL/dq and dL/dk (gnpde_score_grad_f32, exp_kernel
also into dL/d output_var and dL/d lengthscale), then the same projection
backward.  Under squareplus the first pass is gnpde_squareplus_backward_f32 (the
group term and the derivative of the global maximum, which lands on the arg-max
position found in the forward); the score chain rules take its result unchanged.
Every gradient is pinned by fixtures of the reference's own fp64 autograd
(tests/golden/grad_*.npz, tests/test_gpu_grad_golden.py; squareplus:
tests/golden/squareplus/spgrad_*.npz, tests/test_gpu_squareplus.py).
"""
import torch
from torch import nn

from . import ops
from .base_classes import ODEFunc, _tensor_key
from .utils import MaxNFEException


def _check_supported(opt):
    if opt.get('mix_features', False) and not opt.get('gnpde_mix_features', False):
        raise NotImplementedError("gnpde: mix_features=True is broken in the reference "
                                  "(function_transformer_attention.py:29-31 uses a tuple as a tensor); set "
                                  "opt['gnpde_mix_features'] = True to run the intended call, "
                                  "multiply_attention(x, attention, values[0])")
    if opt.get('square_plus', False) and not opt.get('gnpde_square_plus', False):
        raise NotImplementedError("gnpde: square_plus is broken in the reference (utils.squareplus called "
                                  "with a 2-D slice and without num_nodes, :264); set opt['gnpde_square_plus'] = "
                                  "True to run the intended call, utils.squareplus(prods, edge[:, norm_idx, :], None)")
    if opt.get('multi_modal', False):
        raise NotImplementedError("gnpde: multi_modal is broken in the reference and out of scope for the "
                                  "transformer function (opt['gnpde_multi_modal'] serves function='laplacian' "
                                  "under block='constant' only)")
    if opt.get('beltrami', False) and opt.get('attention_type', 'scaled_dot') == 'exp_kernel':
        if not opt.get('gnpde_beltrami_kernel', False):
            raise NotImplementedError("gnpde: the beltrami exp_kernel branch slices nodes instead of features in the "
                                      "reference (:166-167); set opt['gnpde_beltrami_kernel'] = True to run the "
                                      "intended slices, p = x[..., F:F+P] and x[..., :F] | x[..., F+P:]")
        if opt.get('mix_features', False):
            raise NotImplementedError("gnpde: mix_features with the beltrami exp_kernel branch "
                                      "(gnpde_beltrami_kernel): the reference's branch returns v = None (:216), "
                                      "so there are no values to mix")


def beltrami_kernel(opt):
    """Whether ``opt`` selects the beltrami product kernel (:90-123, :164-216): ``beltrami``,
    ``attention_type='exp_kernel'`` and the opt-in key ``gnpde_beltrami_kernel`` (the key
    alone changes nothing)."""
    return bool(opt.get('beltrami', False) and opt.get('attention_type', 'scaled_dot') == 'exp_kernel' and
                opt.get('gnpde_beltrami_kernel', False))


def beltrami_widths(opt, in_features):
    """(C, F, P) of the state layout [features F | positions P | labels C - F - P]
    (GNN.py:23-40, base_classes.py:149-162), checked."""
    C = int(opt['hidden_dim'])
    if int(in_features) != C:
        raise ValueError("gnpde: gnpde_beltrami_kernel: in_features %d != opt['hidden_dim'] %d (augment): the "
                         "reference sizes Qx from opt['hidden_dim'], not from in_features" % (in_features, C))
    if 'feat_hidden_dim' not in opt or 'pos_enc_hidden_dim' not in opt:
        raise ValueError("gnpde: gnpde_beltrami_kernel needs opt['feat_hidden_dim'] and opt['pos_enc_hidden_dim']")
    F, P = int(opt['feat_hidden_dim']), int(opt['pos_enc_hidden_dim'])
    if F < 1 or P < 1 or F + P > C:
        raise ValueError("gnpde: gnpde_beltrami_kernel: feat_hidden_dim %d and pos_enc_hidden_dim %d must be >= 1 "
                         "and sum to at most hidden_dim %d" % (F, P, C))
    return C, F, P


def fold_beltrami(Wqx, bqx, Wkx, bkx, Wqp, bqp, Wkp, bkp, lsx, lsp, heads, F, P, C):
    """The folded projection (W' [4 att, C], b' [4 att]) of the product kernel: since
      |qx - kx|^2 / (2 lsx^2) + |qp - kp|^2 / (2 lsp^2) = |q' - k'|^2 / 2,  q'_h = [qx_h / lsx | qp_h / lsp],
    the score is exp_kernel at heads = h, dk' = 2 dk, p0 = ovx ovp, p1 = 1.  Rows: q' then k'
    (2 att each); in each, head h owns rows h 2dk ..: dk rows of Qx (Kx) / lsx in the feature and
    label columns [0,F) + [F+P,C), then dk rows of Qp (Kp) / lsp in the columns [F,F+P); zero
    elsewhere.  torch ops on the parameters' device, the lengthscales never read on the host."""
    att = Wqx.shape[0]
    dk = att // heads
    dev = Wqx.device
    xcols = torch.cat([torch.arange(0, F, device=dev), torch.arange(F + P, C, device=dev)])
    pcols = torch.arange(F, F + P, device=dev)
    W = torch.zeros(2, heads, 2, dk, C, dtype=Wqx.dtype, device=dev)
    b = torch.zeros(2, heads, 2, dk, dtype=Wqx.dtype, device=dev)
    for side, (Wx, bx, Wp, bp) in enumerate(((Wqx, bqx, Wqp, bqp), (Wkx, bkx, Wkp, bkp))):
        W[side, :, 0].index_copy_(2, xcols, (Wx / lsx).view(heads, dk, C - P))
        W[side, :, 1].index_copy_(2, pcols, (Wp / lsp).view(heads, dk, P))
        b[side, :, 0] = (bx / lsx).view(heads, dk)
        b[side, :, 1] = (bp / lsp).view(heads, dk)
    return W.view(4 * att, C), b.view(4 * att)


def unfold_beltrami(gW, gb, lsx, lsp, heads, F, P, C):
    """fold_beltrami's transpose: the gradients of (W', b') taken back to (Wqx, bqx, Wkx, bkx,
    Wqp, bqp, Wkp, bkp) at fixed lengthscales (their own gradients come per edge,
    ops.score_grad_split)."""
    att = gW.shape[0] // 4
    dk = att // heads
    dev = gW.device
    xcols = torch.cat([torch.arange(0, F, device=dev), torch.arange(F + P, C, device=dev)])
    pcols = torch.arange(F, F + P, device=dev)
    gW = gW.view(2, heads, 2, dk, C)
    gb = gb.view(2, heads, 2, dk)
    out = []
    for part, (cols, ls) in enumerate(((xcols, lsx), (pcols, lsp))):
        for side in (0, 1):
            out.append((gW[side, :, part].index_select(2, cols).reshape(att, cols.numel()) / ls,
                        gb[side, :, part].reshape(att) / ls))
    (gWqx, gbqx), (gWkx, gbkx), (gWqp, gbqp), (gWkp, gbkp) = out
    return gWqx, gbqx, gWkx, gbkx, gWqp, gbqp, gWkp, gbkp


def _needs_grad(*ts):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in ts)


class _EdgeAttention(torch.autograd.Function):
    """attention [B,E,h] (COO) = SpGraphTransAttentionLayer.forward's first
    output as a function of (x, Wq, bq, Wk, bk[, output_var, lengthscale]);
    backward in graph passes."""

    @staticmethod
    def forward(ctx, x, Wq, bq, Wk, bk, ov, ls, layer, g, norm_idx):
        ns, m, rl = layer.scores_and_stats(g, x.detach(), norm_idx, fresh=True)
        att = layer.edge_attention(g, ns, m, rl, norm_idx)
        ctx.save_for_backward(x, Wq, bq, Wk, bk, att)
        ctx.layer, ctx.g, ctx.norm_idx, ctx.ns = layer, g, norm_idx, ns
        # squareplus (m is then the SquareplusState): its backward reads rl and the arg-max positions
        ctx.sp = (rl, m.amax) if isinstance(m, ops.SquareplusState) else None
        ctx.p_shapes = (None if ov is None else (ov.shape, ov.dtype), None if ls is None else (ls.shape, ls.dtype))
        return att

    @staticmethod
    def backward(ctx, g_att):
        x, Wq, bq, Wk, bk, att = ctx.saved_tensors
        g, ns, norm_idx = ctx.g, ctx.ns, ctx.norm_idx
        grouped = g.csr if norm_idx == 0 else g.csc
        if ctx.sp is not None:
            # squareplus is not shift-invariant: dL/ds carries the term of the global maximum
            gs = ops.squareplus_backward(grouped, att, g_att.float(), *ctx.sp)
        else:
            gs = ops.softmax_backward(grouped, att, g_att.float())
        g_ov = g_ls = None
        if ns.mode == ops._lib.SCORE_UNIFORM:
            # every score of a softmax group is the same node score: the attention does not move
            grads = (torch.zeros_like(x), torch.zeros_like(Wq), torch.zeros_like(bq), torch.zeros_like(Wk),
                     torch.zeros_like(bk))
        elif ns.mode == ops._lib.SCORE_REFERENCE:
            grads = _reference_score_backward(g, ns, gs, x.detach(), Wq.detach(), bq.detach(), Wk.detach(),
                                              bk.detach())
        elif ns.mode == ops._lib.SCORE_DOT:
            grads = _dot_score_backward(g, ns, gs, x.detach(), Wq.detach(), Wk.detach())
        else:
            grads, gp = _edge_score_backward(g, ns, gs, x.detach(), Wq.detach(), Wk.detach())
            if gp is not None:
                (so, do), (sl, dl) = ctx.p_shapes
                g_ov, g_ls = gp[0].reshape(so).to(do), gp[1].reshape(sl).to(dl)
        return grads + (g_ov, g_ls, None, None, None)


class _BeltramiAttention(torch.autograd.Function):
    """attention [B,E,h] (COO) of the beltrami product kernel as a function of x, the eight
    Qx / Kx / Qp / Kp tensors and the four scalars.  Forward: the exp_kernel passes over the
    folded projection (fold_beltrami).  Backward: the normaliser's backward, then
    gnpde_score_grad_split_f32 per side (dL/dq', dL/dk' and, summed per edge in fp64,
      S0 = sum g_s 2 s / (ovx ovp),  S1 = sum g_s s |q'x - k'x|^2,  S2 = sum g_s s |q'p - k'p|^2,
    so g_ovx = ovp S0, g_ovp = ovx S0, g_lsx = S1 / lsx, g_lsp = S2 / lsp), the projection
    backward over W' and its unfolding."""

    @staticmethod
    def forward(ctx, x, Wqx, bqx, Wkx, bkx, Wqp, bqp, Wkp, bkp, ovx, lsx, ovp, lsp, layer, g, norm_idx):
        ns, m, rl = layer.scores_and_stats(g, x.detach(), norm_idx, fresh=True)
        att = layer.edge_attention(g, ns, m, rl, norm_idx)
        ctx.save_for_backward(x, ovx, lsx, ovp, lsp, att)
        ctx.layer, ctx.g, ctx.norm_idx, ctx.ns = layer, g, norm_idx, ns
        ctx.Wf = layer.wcat()[0]  # the folded operand these scores were projected with
        ctx.sp = (rl, m.amax) if isinstance(m, ops.SquareplusState) else None
        return att

    @staticmethod
    def backward(ctx, g_att):
        x, ovx, lsx, ovp, lsp, att = ctx.saved_tensors
        g, ns, norm_idx, lay = ctx.g, ctx.ns, ctx.norm_idx, ctx.layer
        grouped = g.csr if norm_idx == 0 else g.csc
        if ctx.sp is not None:
            gs = ops.squareplus_backward(grouped, att, g_att.float(), *ctx.sp)
        else:
            gs = ops.softmax_backward(grouped, att, g_att.float())
        gq, S0, S1, S2 = ops.score_grad_split(g.csr, 0, ns, gs, lay.d_k, with_params=True)
        gk = ops.score_grad_split(g.csc, 1, ns, gs, lay.d_k)
        gqk = torch.cat([gq, gk], 1)
        xd = x.detach()
        gx, _ = ops.linear(gqk, ctx.Wf.t().contiguous())       # gx = [g_q' | g_k'] W'
        gW = ops.linear_wgrad(gqk, xd.reshape(g.R, -1))         # [4 att, C] = gqk^T x
        gb = gqk.sum(0)
        ovx, lsx, ovp, lsp = ovx.detach(), lsx.detach(), ovp.detach(), lsp.detach()
        C, F, P = lay.beltrami_dims
        gws = unfold_beltrami(gW, gb, lsx, lsp, lay.h, F, P, C)
        scal = tuple((v.double() * s).to(v.dtype).reshape(v.shape) for v, s in
                     ((ovp, S0), (1.0 / lsx, S1), (ovx, S0), (1.0 / lsp, S2)))
        return (gx.view(x.shape),) + gws + scal + (None, None, None)


class _MixProject(torch.autograd.Function):
    """v = V(x) (:226) on the matrix cores, with its backward (mix_features)."""

    @staticmethod
    def forward(ctx, x, W, b):
        ctx.save_for_backward(x, W)
        return ops.linear(x.detach(), W.detach(), b.detach())[0].view(tuple(x.shape[:-1]) + (W.shape[0],))

    @staticmethod
    def backward(ctx, g_v):
        x, W = ctx.saved_tensors
        g_v = g_v.contiguous()
        gx = ops.linear(g_v, W.detach().t().contiguous())[0].view(x.shape) if ctx.needs_input_grad[0] else None
        gW = ops.linear_wgrad(g_v, x.detach()).to(W.dtype) if ctx.needs_input_grad[1] else None
        gb = g_v.reshape(-1, g_v.shape[-1]).sum(0).to(W.dtype) if ctx.needs_input_grad[2] else None
        return gx, gW, gb


class _MixRHS(torch.autograd.Function):
    """f = a (Wout(z) - x) [+ b x0], z = the per-head aggregation of v = V(x) with the
    attention [B,E,h], as a function of (x, alpha, beta, attention, V, Wout): the forward
    kernels of the no-grad path and a backward of existing passes, one launch per head
    where the head slices differ.  With g = dL/df and gh = a g:
      g_Wout = gh^T z, g_bout = sum_r gh, g_z = gh Wout,
      g_att[e,h] = <g_z[row(e)], v[col(e), head h]> / H            (an SDDMM per head),
      g_v[:, head h] = A_h^T g_z / H                               (K1 over the CSC per head),
      g_V = g_v^T x, g_bv = sum_r g_v, g_x = -gh + g_v V,
      g_alpha, g_beta by fp64 dots (as the Laplacian RHS)."""

    @staticmethod
    def forward(ctx, x, alpha_train, beta_train, att, Wv, bv, Wo, bo, g, x0, alpha_sigmoid, add_source):
        xd, ad = x.detach(), att.detach().float().contiguous()
        v = ops.linear(xd, Wv.detach(), bv.detach())[0]                        # [R, att]
        z = ops.head_aggregate(g, ad, v, coo=True)                             # [R, dk]
        f = ops.linear_rhs(z, Wo.detach(), xd, x0=x0, alpha=alpha_train.detach(), beta=beta_train.detach(), rhs=True,
                           alpha_sigmoid=alpha_sigmoid, add_source=add_source, bias=bo.detach())
        ctx.save_for_backward(x, alpha_train, beta_train, ad, Wv, Wo, bo, v, z)
        ctx.g, ctx.x0 = g, x0
        ctx.alpha_sigmoid, ctx.add_source = alpha_sigmoid, add_source
        return f

    @staticmethod
    def backward(ctx, gf):
        x, alpha_train, beta_train, ad, Wv, Wo, bo, v, z = ctx.saved_tensors
        g = ctx.g
        gf = gf.contiguous()
        x, Wv, Wo, bo = x.detach(), Wv.detach(), Wo.detach(), bo.detach()
        H = ad.shape[2]
        dk = z.shape[1]
        al = alpha_train.detach()
        a = torch.sigmoid(al) if ctx.alpha_sigmoid else al
        gh = (a.float() * gf).contiguous()
        ghr = gh.reshape(g.R, -1)
        need = ctx.needs_input_grad
        gx = ga = gb = gatt = gWv = gbv = gWo = gbo = None
        if need[6]:
            gWo = ops.linear_wgrad(ghr, z).to(Wo.dtype)                        # [C, dk] = gh^T z
        if need[7]:
            gbo = ghr.sum(0).to(bo.dtype)
        if need[0] or need[3] or need[4] or need[5]:
            g_z = ops.linear(ghr, Wo.t().contiguous())[0]                      # [R, dk] = gh Wout
            if need[3]:
                gatt = torch.empty_like(ad)
                for h in range(H):
                    vh = v[:, h * dk:(h + 1) * dk].contiguous()
                    gatt[:, :, h] = ops.sddmm(g, g_z, vh)
                gatt = gatt / H
            if need[0] or need[4] or need[5]:
                g_v = torch.empty_like(v)
                for h in range(H):
                    g_v[:, h * dk:(h + 1) * dk] = ops.spmm_rhs(g, ops.gather_head(g.csc, ad, h, 1.0 / H), g_z,
                                                               rhs=False, transpose=True)
                if need[4]:
                    gWv = ops.linear_wgrad(g_v, x.reshape(g.R, -1)).to(Wv.dtype)   # [att, C] = g_v^T x
                if need[5]:
                    gbv = g_v.sum(0).to(Wv.dtype)
                if need[0]:
                    gx = ops.linear(g_v, Wv.t().contiguous())[0].view(x.shape) - gh   # g_v V - gh
        if need[1]:
            one = torch.ones((), dtype=torch.float32, device=x.device)
            d = ops.linear_rhs(z, Wo, x, alpha=one, rhs=True, alpha_sigmoid=False, bias=bo)   # ax - x
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
        return gx, ga, gb, gatt, gWv, gbv, gWo, gbo, None, None, None, None


def _reference_score_backward(g, ns, gs, x, Wq, bq, Wk, bk):
    """Chain rule of the fork's scaled_dot (function_transformer_attention.py:249):
    s[e,h] = cs[src(e),h], cs[n,h] = q_{n,h} . S_h / sqrt(dk), q = Wq x + bq,
    S = Wk xbar + E bk, xbar = sum_n indeg(n) x_n.  Graph passes in HIP; the
    [att, C]-sized products in fp64 torch."""
    B, N, H, dk = g.B, g.N, ns.heads, ns.dk
    att_dim = H * dk
    C = x.shape[-1]
    inv = 1.0 / float(dk) ** 0.5
    gcs = ops.segment_sum(g.csr, gs)                           # [R,H]: edges gather the score of their source
    xbar = ops.wcolsum(x, B, N, g.indeg.double().view(-1, 1))[:, 0, :]    # [B,C+1]
    y = ops.wcolsum(x, B, N, gcs)                              # [B,H,C+1]
    Wq64, bq64, Wk64, bk64 = Wq.double(), bq.double(), Wk.double(), bk.double()
    S = xbar[:, :C] @ Wk64.t() + xbar[:, C:] * bk64            # [B,att]
    Sh = S.view(B, H, dk)
    Wqh = Wq64.view(H, dk, C)
    U = inv * torch.einsum('hdc,bhd->bch', Wqh, Sh)            # [B,C,H]
    gU = y[:, :, :C].transpose(1, 2)                           # [B,C,H]
    gv = y[:, :, C]                                            # [B,H]
    g_Wq = inv * torch.einsum('bhd,bch->hdc', Sh, gU).reshape(att_dim, C)
    g_bq = inv * torch.einsum('bhd,bh->hd', Sh, gv).reshape(att_dim)
    gS = inv * (torch.einsum('hdc,bch->bhd', Wqh, gU) + bq64.view(H, dk)[None] * gv[:, :, None])
    gS = gS.reshape(B, att_dim)
    g_Wk = gS.t() @ xbar[:, :C]
    g_bk = gS.t() @ xbar[:, C]
    gxbar = gS @ Wk64                                          # [B,C]
    gx = ops.score_input_grad(gcs, U, g.indeg, gxbar, B, N, C).view(x.shape)
    return (gx, g_Wq.to(Wq.dtype), g_bq.to(bq.dtype), g_Wk.to(Wk.dtype), g_bk.to(bk.dtype))


def _dot_score_backward(g, ns, gs, x, Wq, Wk):
    """Per-edge scaled_dot s[e,h] = q[src,h] . k[dst,h] / sqrt(dk): per head, g_q
    aggregates g_s k[dst] over the CSR and g_k aggregates g_s q[src] over the
    CSC (K1 with per-head weights), then the projection backward."""
    H, dk = ns.heads, ns.dk
    inv = 1.0 / float(dk) ** 0.5
    R = g.R
    xr = x.reshape(R, -1)
    gqk = torch.empty(R, 2 * H * dk, dtype=torch.float32, device=x.device)
    for h in range(H):
        cols = slice(h * dk, (h + 1) * dk)
        kh = ns.k[:, cols].contiguous()
        qh = ns.q[:, cols].contiguous()
        gqk[:, cols] = ops.spmm_rhs(g, ops.gather_head(g.csr, gs, h, inv), kh, rhs=False)
        gqk[:, H * dk + h * dk:H * dk + (h + 1) * dk] = ops.spmm_rhs(g, ops.gather_head(g.csc, gs, h, inv), qh,
                                                                     rhs=False, transpose=True)
    W = torch.cat([Wq, Wk], 0)                                 # [2att, C]
    gx, _ = ops.linear(gqk, W.t().contiguous())                # gx = [g_q | g_k] [Wq; Wk]
    gW = ops.linear_wgrad(gqk, xr)                             # [2att, C] = gqk^T x on the matrix cores
    gb = gqk.sum(0)
    att_dim = H * dk
    return (gx.view(x.shape), gW[:att_dim], gb[:att_dim], gW[att_dim:], gb[att_dim:])


def _edge_score_backward(g, ns, gs, x, Wq, Wk):
    """exp_kernel / cosine_sim / pearson (function_transformer_attention.py:246-259):
    dL/dq over the aggregation CSR (edges grouped by source) and dL/dk over the
    CSC (grouped by destination) in one pass each (gnpde_score_grad_f32), then
    the projection backward as for the per-edge scaled_dot.  exp_kernel also
    returns dL/d(output_var), dL/d(lengthscale)."""
    with_p = ns.mode == ops._lib.SCORE_EXP_KERNEL
    if with_p:
        gq, gov, gls = ops.score_grad(g.csr, 0, ns, gs, with_params=True)
    else:
        gq = ops.score_grad(g.csr, 0, ns, gs)
    gk = ops.score_grad(g.csc, 1, ns, gs)
    gqk = torch.cat([gq, gk], 1)
    xr = x.reshape(g.R, -1)
    W = torch.cat([Wq, Wk], 0)
    gx, _ = ops.linear(gqk, W.t().contiguous())                # gx = [g_q | g_k] [Wq; Wk]
    gW = ops.linear_wgrad(gqk, xr)
    gb = gqk.sum(0)
    att_dim = ns.heads * ns.dk
    grads = (gx.view(x.shape), gW[:att_dim], gb[:att_dim], gW[att_dim:], gb[att_dim:])
    return grads, ((gov, gls) if with_p else None)


class SpGraphTransAttentionLayer(nn.Module):
    """src/function_transformer_attention.py:65-270 (standard branch)."""

    def __init__(self, in_features, out_features, opt, device, concat=True, edge_weights=None):
        super(SpGraphTransAttentionLayer, self).__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.alpha = opt.get('leaky_relu_slope', 0.2)
        self.concat = concat
        self.device = device
        self.opt = opt
        self.h = int(opt['heads'])
        self.edge_weights = edge_weights
        self.attention_dim = opt.get('attention_dim', out_features)
        assert self.attention_dim % self.h == 0, \
            "Number of heads ({}) must be a factor of the dimension size ({})".format(self.h, self.attention_dim)
        self.d_k = self.attention_dim // self.h
        _check_supported(opt)
        self.mix = bool(opt.get('mix_features', False))
        self.beltrami_kernel = beltrami_kernel(opt)
        if self.beltrami_kernel:
            # the product kernel (:90-107): split projections of the feature (+ label) and the
            # positional columns, an amplitude and a lengthscale each; no Q, K or V
            C, F, P = self.beltrami_dims = beltrami_widths(opt, in_features)
            self.output_var_x = nn.Parameter(torch.ones(1))
            self.lengthscale_x = nn.Parameter(torch.ones(1))
            self.output_var_p = nn.Parameter(torch.ones(1))
            self.lengthscale_p = nn.Parameter(torch.ones(1))
            for name, width in (('Qx', C - P), ('Vx', C - P), ('Kx', C - P), ('Qp', P), ('Vp', P), ('Kp', P)):
                lin = nn.Linear(width, self.attention_dim)
                self.init_weights(lin)
                setattr(self, name, lin)
        else:
            if opt.get('attention_type', 'scaled_dot') == "exp_kernel":
                self.output_var = nn.Parameter(torch.ones(1))
                self.lengthscale = nn.Parameter(torch.ones(1))
            self.Q = nn.Linear(in_features, self.attention_dim)
            self.init_weights(self.Q)
            self.V = nn.Linear(in_features, self.attention_dim)
            self.init_weights(self.V)
            self.K = nn.Linear(in_features, self.attention_dim)
            self.init_weights(self.K)
        self.activation = nn.Sigmoid()
        self.Wout = nn.Linear(self.d_k, in_features)
        self.init_weights(self.Wout)
        self._graph = None
        self._graph_key = None
        self._uniform = None  # (graph, NodeScores, m, rl, csr weights) for the uniform fast path
        self._wcat = None     # (param versions, ([Wq;Wk], [bq;bk]))
        self._p0 = None       # (param versions, ovx * ovp): the beltrami product kernel's amplitude
        self._sp_bufs = None  # (state shape, ops.SquareplusState): the squareplus operands
        self._mixp = None     # (param versions, (Wv, bv, Wout, b_out)): mix_features
        self._uniform_heads = None  # (graph, per-head weights [nnz, h]) of the uniform case: mix_features

    def init_weights(self, m):
        """Constant 1e-5 init (:153-157)."""
        if type(m) == nn.Linear:
            nn.init.constant_(m.weight, 1e-5)

    @property
    def score_mode(self):
        return self.opt.get('attention_score_mode', 'reference')

    def score_parameters(self):
        """The parameters the scores depend on, in the order of the layer's autograd function
        (what the transformer function and the blocks test for requires_grad)."""
        if self.beltrami_kernel:
            return (self.Qx.weight, self.Qx.bias, self.Kx.weight, self.Kx.bias, self.Qp.weight, self.Qp.bias,
                    self.Kp.weight, self.Kp.bias, self.output_var_x, self.lengthscale_x, self.output_var_p,
                    self.lengthscale_p)
        ps = (self.Q.weight, self.Q.bias, self.K.weight, self.K.bias)
        if self.opt.get('attention_type', 'scaled_dot') == 'exp_kernel':
            ps += (self.output_var, self.lengthscale)
        return ps

    def _score_params(self):
        if self.beltrami_kernel:
            # the folded projection carries the lengthscales: p0 = ovx ovp, p1 = 1.  The two
            # amplitudes are read on the host once per parameter version (the eager step that
            # precedes a capture reads them; a capture must not synchronise)
            key = (_tensor_key(self.output_var_x), _tensor_key(self.output_var_p))
            if self._p0 is None or self._p0[0] != key:
                self._p0 = (key, float(self.output_var_x.detach()) * float(self.output_var_p.detach()))
            return self._p0[1], 1.0
        if self.opt.get('attention_type', 'scaled_dot') == 'exp_kernel':
            # p0 = output_var, p1 = lengthscale: read once per call (host sync of 2 scalars)
            return float(self.output_var.detach()), float(self.lengthscale.detach())
        return 1.0, 1.0

    def graph_for(self, x, edge):
        key = (_tensor_key(edge), int(x.shape[1]))
        if self._graph is None or key != self._graph_key:
            self._graph = ops.GraphCSR(edge, int(x.shape[1]), chunk=self.opt.get('gnpde_chunk'))
            self._graph_key = key
        return self._graph

    def is_uniform(self, norm_idx):
        """Fork scaled_dot + source-grouped softmax: all scores of a group are equal,
        so the attention is 1/outdeg whatever x — graph-only, cached."""
        return (self.score_mode == 'reference' and norm_idx == 0 and
                self.opt.get('attention_type', 'scaled_dot') == 'scaled_dot')

    @property
    def square_plus(self):
        """opt['square_plus'] (accepted with opt['gnpde_square_plus'], _check_supported)."""
        return bool(self.opt.get('square_plus', False))

    def squareplus_buffers(self, g, x):
        """The squareplus operands (ops.SquareplusState: M, the per-node p or the stored
        scores, the reduction scratch) cached per state shape and device — stable buffers,
        so captured step graphs keep replaying and the RHS reads nothing on the host."""
        mode = ops.SCORE_MODES[(self.opt.get('attention_type', 'scaled_dot'), self.score_mode)]
        key = (g.B, g.N, g.E, self.h, mode, str(x.device))
        if self._sp_bufs is None or self._sp_bufs[0] != key:
            self._sp_bufs = (key, ops.squareplus_buffers(g, mode, self.h, x.device))
        return self._sp_bufs[1]

    def scores_and_stats(self, g, x, norm_idx, fresh=False):
        """(NodeScores, m, rl) for this RHS evaluation; under squareplus m is the
        ops.SquareplusState (the global maxima M and what the later passes read) — in the
        layer's cached buffers, or new ones with fresh=True (autograd keeps them).
        Uniform scores keep the cached 1/outdeg statistics under either normaliser:
        att = p / (d p + 1e-16) is 1/outdeg to within 1e-16 / (d p)."""
        if self.is_uniform(norm_idx):
            if self._uniform is None or self._uniform[0] is not g:
                ns = ops.uniform_scores(self.h)
                m, rl = ops.softmax_stats(g, ns, 0)
                self._uniform = (g, ns, m, rl, ops.attn_weights(g, ns, m, rl, 0))
            return self._uniform[1:4]
        ns = self.node_scores(g, x)
        if self.square_plus:
            sq = ops.score_max(g, ns, None if fresh else self.squareplus_buffers(g, x))
            return ns, sq, ops.squareplus_stats(g, ns, sq, norm_idx)
        m, rl = ops.softmax_stats(g, ns, norm_idx)
        return ns, m, rl

    def edge_attention(self, g, ns, m, rl, norm_idx):
        """attention [B,E,h] (COO) from scores_and_stats' result, under the layer's normaliser."""
        if isinstance(m, ops.SquareplusState):
            return ops.squareplus_attention(g, ns, m, rl, norm_idx)
        return ops.edge_attention(g, ns, m, rl, norm_idx)

    def uniform_weights(self, g):
        self.scores_and_stats(g, None, 0)
        return self._uniform[4]

    def uniform_head_weights(self, g):
        """The uniform case's per-head weights [nnz, h] (aggregation-CSR order; 1/outdeg in
        every head), computed once per graph and cached beside ``_uniform`` (mix_features)."""
        if self._uniform_heads is None or self._uniform_heads[0] is not g:
            ns, m, rl = self.scores_and_stats(g, None, 0)
            self._uniform_heads = (g, ops.head_weights(g, ns, m, rl, 0))
        return self._uniform_heads[1]

    def mix_params(self):
        """(Wv [att, C], bv [att], Wout [C, dk], b_out [C]) contiguous, cached per parameter
        version: the operands of the two products of mix_features (stable buffers, so
        captured step graphs keep replaying)."""
        ps = (self.V.weight, self.V.bias, self.Wout.weight, self.Wout.bias)
        key = tuple(_tensor_key(t) for t in ps)
        if self._mixp is None or self._mixp[0] != key:
            self._mixp = (key, tuple(t.detach().contiguous() for t in ps))
        return self._mixp[1]

    def project(self, x):
        """v = V(x) (:226) [.., attention_dim] fp32, head h in columns h*dk .. (mix_features)."""
        if x.dtype != torch.float32:
            raise NotImplementedError("gnpde: transformer mix_features runs on fp32 states only (got %s)" % x.dtype)
        if _needs_grad(x, self.V.weight, self.V.bias):
            return _MixProject.apply(x, self.V.weight, self.V.bias)
        Wv, bv, _, _ = self.mix_params()
        return ops.linear(x, Wv, bv)[0].view(tuple(x.shape[:-1]) + (self.attention_dim,))

    def uses_wcat(self):
        """Per-edge score modes project Q|K with one fused MFMA GEMM over [Wq; Wk]."""
        return self.score_mode != 'reference' or self.opt.get('attention_type', 'scaled_dot') != 'scaled_dot'

    def wcat(self):
        """([Wq; Wk], [bq; bk]) cached per parameter version; the beltrami product kernel:
        the folded operand (fold_beltrami, [4 att, C]) over its eight tensors and two lengthscales."""
        if self.beltrami_kernel:
            ps = self.score_parameters()
            ps = ps[:8] + (ps[9], ps[11])
            key = tuple(_tensor_key(t) for t in ps)
            if self._wcat is None or self._wcat[0] != key:
                C, F, P = self.beltrami_dims
                with torch.no_grad():
                    W, b = fold_beltrami(*[t.detach() for t in ps], self.h, F, P, C)
                self._wcat = (key, (W.contiguous(), b.contiguous()))
            return self._wcat[1]
        key = tuple(_tensor_key(t) for t in (self.Q.weight, self.Q.bias, self.K.weight, self.K.bias))
        if self._wcat is None or self._wcat[0] != key:
            self._wcat = (key, (torch.cat([self.Q.weight.detach(), self.K.weight.detach()], 0).contiguous(),
                                torch.cat([self.Q.bias.detach(), self.K.bias.detach()], 0).contiguous()))
        return self._wcat[1]

    def node_scores(self, g, x):
        p0, p1 = self._score_params()
        if self.beltrami_kernel:
            # exp_kernel over the folded projection: heads h, dk' = 2 dk (fold_beltrami)
            return ops.node_scores(g, x, None, None, None, None, self.h, 'exp_kernel', self.score_mode, p0, p1,
                                   wcat=self.wcat())
        wcat = self.wcat() if self.uses_wcat() else None
        return ops.node_scores(g, x, self.Q.weight.detach(), self.Q.bias.detach(), self.K.weight.detach(),
                               self.K.bias.detach(), self.h, self.opt.get('attention_type', 'scaled_dot'),
                               self.score_mode, p0, p1, wcat=wcat)

    def forward(self, x, edge, y=None):
        """Returns (attention [B,E,h], (None, None)): the per-edge softmax
        attention of :265-266 in COO order.  ``values`` (V(x), prods) is not
        materialised (dead for mix_features=False).  Under mix_features:
        (attention, (v, None)), v = V(x) in the reference's layout [B,N,dk,h] (:226-234:
        a transposed view of the [B,N,h,dk] projection); ``prods`` stays unmaterialised."""
        att = self.attention(x, edge)
        if not self.mix:
            return att, (None, None)
        v = self.project(x)
        return att, (v.view(tuple(v.shape[:-1]) + (self.h, self.d_k)).transpose(-1, -2), None)

    def attention(self, x, edge):
        """attention [B,E,h] (COO): forward's first output."""
        g = self.graph_for(x, edge)
        norm_idx = int(self.opt['attention_norm_idx'])
        ov = getattr(self, 'output_var', None)
        ls = getattr(self, 'lengthscale', None)
        if _needs_grad(x, *self.score_parameters()):
            if self.beltrami_kernel:
                if x.dtype != torch.float32:
                    raise NotImplementedError("gnpde: gnpde_beltrami_kernel trains on fp32 states only (got %s)"
                                              % x.dtype)
                return _BeltramiAttention.apply(x, *self.score_parameters(), self, g, norm_idx)
            return _EdgeAttention.apply(x, self.Q.weight, self.Q.bias, self.K.weight, self.K.bias, ov, ls, self, g,
                                        norm_idx)
        ns, m, rl = self.scores_and_stats(g, x, norm_idx)
        return self.edge_attention(g, ns, m, rl, norm_idx)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'


class ODEFuncTransformerAtt(ODEFunc):
    """src/function_transformer_attention.py:9-62."""

    def __init__(self, in_features, out_features, opt, device):
        super(ODEFuncTransformerAtt, self).__init__(opt, device)
        self.in_features = in_features
        self.out_features = out_features
        self.multihead_att_layer = SpGraphTransAttentionLayer(in_features, out_features, opt, device,
                                                              edge_weights=self.edge_weight)
        if device is not None:
            self.multihead_att_layer = self.multihead_att_layer.to(device)
        self.y = None

    def multiply_attention(self, x, attention, v=None):
        """A_mean x with attention [B,E,h] given explicitly (:33-42); under mix_features
        Wout(z) (:23-32), z the per-head aggregation of ``v`` (the layer's [B,N,dk,h]
        values; V(x) when not given) with that attention."""
        g = self.graph_for(x)
        lay = self.multihead_att_layer
        if lay.mix:
            if x.dtype != torch.float32:
                raise NotImplementedError("gnpde: transformer mix_features runs on fp32 states only (got %s)"
                                          % x.dtype)
            if v is None:
                vr = lay.project(x.detach())
            else:  # [B,N,dk,h] -> [B,N,att] with head h in columns h*dk ..
                vr = v.detach().float().transpose(-1, -2).reshape(g.B, g.N, lay.attention_dim)
            z = ops.head_aggregate(g, attention.detach().float(), vr, coo=True)
            _, _, Wo, bo = lay.mix_params()
            return ops.linear_rhs(z, Wo, x.detach(), rhs=False, bias=bo)
        w = g.gather_weights(attention.detach().float())
        return ops.spmm_rhs(g, w, x, rhs=False)

    def rhs_stage(self, t, x, stage):
        """forward(t, x) with the solver's stage combination fused into the
        aggregation epilogue (gnpde.integrator, no-grad fixed-grid solvers)."""
        self._rhs(x, stage)

    def graph_capture_state(self, x):
        """What a captured fused step reads (gnpde.integrator._capture_state):
        the device CSR / CSC + plans, the layer's cached operands (the 1/outdeg
        weights of the uniform case, or the concatenated [Wq; Wk] projection)
        and, with add_source, the stable x0 buffer."""
        g = self.graph_for(x)
        lay = self.multihead_att_layer
        st = [g]
        if lay.mix:
            # the cached contiguous V / Wout operands, and the uniform case's per-head weights
            st.append(lay.mix_params())
            if lay.is_uniform(int(self.opt['attention_norm_idx'])):
                st.append(lay.uniform_head_weights(g))
        if lay.is_uniform(int(self.opt['attention_norm_idx'])):
            lay.uniform_weights(g)
            st.append(lay._uniform)
        elif lay.uses_wcat():
            st.append(lay.wcat())
        if lay.square_plus and not lay.is_uniform(int(self.opt['attention_norm_idx'])):
            # the squareplus operands (M, p / stored scores) and the statistics plan of the groups
            grouped = g.csr if int(self.opt['attention_norm_idx']) == 0 else g.csc
            st.extend([lay.squareplus_buffers(g, x), grouped.stats_plan, g.csr.rowidx])
        if self.opt.get('add_source', False):
            st.append(self.stable_x0(x))
        return st

    def supports_node_layout(self):
        """The graph's locality numbering (ops.NodeLayout) for fixed-grid solves: every
        operand of the scaled_dot RHS is per node (x, q, k, node scores) or per edge
        in COO order, and a renumbering relabels them consistently, so the scores,
        the softmax groups and the aggregation are the same.  Bit-identical for the
        weights that are row-local in the fused kernels (the fork's 1/outdeg weights
        under source-grouped softmax — BLEND — and the per-edge scores under
        source-grouped softmax: each row scores and sums its own edges in COO
        order); the key sum of the fork's scores (fp64, row-tile order) and the
        destination statistics (packed CSC edge blocks) are summed in another order,
        within fp64 / fp32 rounding (tests/test_gpu_layout.py).  Other attention
        types keep the user numbering, and so does mix_features."""
        lay = self.multihead_att_layer
        if lay.mix:
            return False
        return lay.is_uniform(int(self.opt['attention_norm_idx'])) or \
            self.opt.get('attention_type', 'scaled_dot') == 'scaled_dot'

    def supports_feature_padding(self):
        """With the fork's scaled_dot under source-grouped softmax the weights do
        not depend on x (1/outdeg), so columns are independent and the fused
        integrator may pad the state (integrator._padded_width); score modes
        read Q/K over all C columns and may not, nor does mix_features (V reads them)."""
        if self.multihead_att_layer.mix:
            return False
        return self.multihead_att_layer.is_uniform(int(self.opt['attention_norm_idx'])) and \
            not self.opt.get('add_source', False)

    def forward(self, t, x):  # t is needed when called by the integrator
        return self._rhs(x, None)

    def _rhs(self, x, stage):
        if self.nfe > self.opt["max_nfe"]:
            raise MaxNFEException
        self.nfe += 1
        g = self.graph_for(x)
        lay = self.multihead_att_layer
        if lay.mix and x.dtype != torch.float32:
            raise NotImplementedError("gnpde: transformer mix_features runs on fp32 states only (got %s)" % x.dtype)
        mixp = (lay.V.weight, lay.V.bias, lay.Wout.weight, lay.Wout.bias) if lay.mix else ()
        if stage is None and _needs_grad(x, self.alpha_train, self.beta_train, *lay.score_parameters(), *mixp):
            return self._rhs_autograd(g, x)
        norm_idx = int(self.opt['attention_norm_idx'])
        add_source = bool(self.opt.get('add_source', False))
        if add_source and self.x0 is None:
            raise RuntimeError("ODEFuncTransformerAtt: add_source needs x0 (ODEblock.set_x0)")
        # fused stages (and their captured graphs) read a stable x0 buffer (ODEFunc.stable_x0)
        x0 = (self.stable_x0(x) if stage is not None else self.x0) if add_source else None
        if x0 is not None and x0.dtype != x.dtype:
            x0 = x0.to(x.dtype)
        kw = dict(x0=x0, alpha=self.alpha_train.detach(), beta=self.beta_train.detach(),
                  rhs=True, alpha_sigmoid=not self.opt.get('no_alpha_sigmoid', False), add_source=add_source,
                  stage=stage)
        if lay.mix:
            # the value projection: per-head attention (cached for the uniform case), v = V(x),
            # z by the per-head aggregation, then Wout with its bias and the RHS epilogue fused
            if lay.is_uniform(norm_idx):
                wh = lay.uniform_head_weights(g)
            else:
                wh = ops.head_weights(g, *lay.scores_and_stats(g, x, norm_idx), norm_idx)
            Wv, bv, Wo, bo = lay.mix_params()
            v = ops.linear(x, Wv, bv)[0]
            z = ops.head_aggregate(g, wh, v)
            # a solver stage takes f + the stage pass (the same bits as the kernel's fused stage)
            return ops.linear_rhs(z, Wo, x, bias=bo, fuse=False, **kw)
        if lay.is_uniform(norm_idx):
            return ops.spmm_rhs(g, lay.uniform_weights(g), x, **kw)
        if lay.square_plus:
            # squareplus: score maximum, group statistics, then the fused K1 (reference scores,
            # norm_idx 1, fp32 state) or the weights pass + K1; operands in the layer's buffers.
            # A bf16 state: the reference scores from an fp32 copy, as below
            ref = lay.score_mode == 'reference' and self.opt.get('attention_type', 'scaled_dot') == 'scaled_dot'
            ns = lay.node_scores(g, x.float() if ref and x.dtype == torch.bfloat16 else x)
            return ops.squareplus_rhs(g, ns, norm_idx, x, bufs=lay.squareplus_buffers(g, x), **kw)
        if x.dtype == torch.bfloat16:
            # bf16 storage: the per-edge scores' projection reads the bf16 state itself
            # (gnpde_linear_bf16, the same bits as from an fp32 copy); the fork's reference
            # scores (fp64 key sum and node scores) from an fp32 copy; weights precomputed,
            # bf16 aggregation
            ref = lay.score_mode == 'reference' and self.opt.get('attention_type', 'scaled_dot') == 'scaled_dot'
            ns = lay.node_scores(g, x.float() if ref else x)
            m, rl = ops.softmax_stats(g, ns, 1) if norm_idx == 1 else (None, None)
            # per-edge scaled_dot under source-grouped softmax: the fused pass over the bf16
            # state (gnpde_attn_dot_rhs_bf16); otherwise K2 weights + the bf16 K1
            return ops.attn_rhs(g, ns, m, rl, norm_idx, x, fuse=not ref and norm_idx == 0, **kw)
        ns = lay.node_scores(g, x)
        # destination-grouped softmax needs its statistics over the CSC first
        # (attn_rhs computes them: packed records for the fork's two-head
        # scores); source-grouped weights come straight from the scores (K2)
        return ops.attn_rhs(g, ns, None, None, norm_idx, x, **kw)

    def _rhs_autograd(self, g, x):
        """Training forward: attention [B,E,h] through _EdgeAttention, then the
        Laplacian RHS autograd with those weights (head mean), so gradients
        reach x (both paths), alpha, beta and the Q/K parameters.  Under mix_features
        _MixRHS instead: x also through V, and V / Wout with their biases."""
        from .function_laplacian_diffusion import _LaplacianRHS
        lay = self.multihead_att_layer
        att = lay.attention(x, self.edge_index)
        add_source = bool(self.opt.get('add_source', False))
        if add_source and self.x0 is None:
            raise RuntimeError("ODEFuncTransformerAtt: add_source needs x0 (ODEblock.set_x0)")
        x0 = self.x0 if add_source else None
        if x0 is not None and x0.dtype != torch.float32:
            x0 = x0.float()
        if lay.mix:
            return _MixRHS.apply(x, self.alpha_train, self.beta_train, att, lay.V.weight, lay.V.bias, lay.Wout.weight,
                                 lay.Wout.bias, g, x0, not self.opt.get('no_alpha_sigmoid', False), add_source)
        ad = att.detach()
        return _LaplacianRHS.apply(x, self.alpha_train, self.beta_train, att, g, g.gather_weights(ad),
                                   lambda: g.gather_weights(ad, transpose=True), x0,
                                   not self.opt.get('no_alpha_sigmoid', False), add_source)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.in_features) + ' -> ' + str(self.out_features) + ')'
