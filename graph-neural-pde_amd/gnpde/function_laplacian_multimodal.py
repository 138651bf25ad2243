"""The multi_modal branch of LaplacianODEFunc (reference src/function_laplacian_diffusion.py
:29-37 and :61-63): the Laplacian RHS of a cross-attention of the node rows against the
tokens ``y`` [B, M, D2] of a second modality,

    q = Q2(x), k = K2(y), v = V2(y)
    x~ = softmax(q k^T / sqrt(C), dim=-1) v                    (dk = in_features = C)
    f  = a (A x~ - x~) [+ b x0],   a = sigmoid(alpha_train) unless no_alpha_sigmoid.

The reference cannot run the branch (``torch.nn.softmax`` is a module class, and the class
has no ``init_weights``), so it is opt-in: ``opt['gnpde_multi_modal'] = True`` selects the
lines as they are meant — ``torch.softmax(..., dim=-1)``, as the transformer layer's
multi_modal branch spells out (:171) — and ``model_configurations.set_function`` then
returns ``MultiModalLaplacianODEFunc`` for ``function='laplacian'``.  Q2 / K2 / V2 keep the
reference's state_dict names and take the fork's constant 1e-5 weight initialisation (the
transformer layer's ``init_weights``, function_transformer_attention.py:153-157).

Served: ``block='constant'``, fp32 states, one GPU, the user's node numbering.  The state
reaches f only through Q2, so this RHS is not affine in x: the class is not a
LaplacianODEFunc and offers none of the hooks the integrator keys its affine fast paths on.

One RHS without autograd: q on the matrix cores (gnpde_linear_f32), k / v projected ONCE
per (y, parameter version) and cached, the flash-style cross-attention
(gnpde_cross_attention_f32, csrc/cross_attention.hip: no [B, N, M] score buffer), K1 with
the RHS epilogue (gnpde_spmm_rhs_f32); a solver stage then takes the stage pass
(gnpde_stage_apply_f32) on the solver's state x — K1's own stage epilogue would read its
input x~.  Training composes the projection autograd (_MixProject), _CrossAttention (the
forward kernel with its log-sum-exp; a backward of existing passes over row chunks that
recomputes P from it) and _LaplacianRHS on x~.  DESIGN.md §6.20.
"""
import math

import torch
from torch import nn

from . import ops
from .base_classes import ODEFunc, _tensor_key
from .function_laplacian_diffusion import _LaplacianRHS
from .function_transformer_attention import _MixProject, _needs_grad
from .utils import MaxNFEException

# bytes of one [rows, M] scratch array of _CrossAttention.backward (it holds four: 64 MB in all)
BACKWARD_CHUNK_BYTES = 1 << 24
# keys per product of dq = dS k: gnpde_linear_f32 stages W^T over its whole K in LDS
_DQ_KEYS = 512


class _CrossAttention(torch.autograd.Function):
    """x~ = softmax(scale q k^T) v as a function of (q [B,N,C], k [B,M,C], v [B,M,C]).
    With g = dL/dx~, P = exp(scale q k^T - lse) and D = rowsum(g * x~):
      dP = g v^T, dS = P * (dP - D),
      g_q = scale dS k, g_k = scale dS^T q, g_v = P^T g,
    formed per batch element on chunks of rows whose [rows, M] scratch is bounded
    (BACKWARD_CHUNK_BYTES), the chunks summed in row order."""

    @staticmethod
    def forward(ctx, q, k, v, scale):
        out, lse = ops.cross_attention(q.detach(), k.detach(), v.detach(), scale, lse=True)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, g_out):
        q, k, v, out, lse = ctx.saved_tensors
        q, k, v = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        g_out = g_out.contiguous()
        B, N, C = q.shape
        M = k.shape[1]
        scale = ctx.scale
        need_q, need_k, need_v = ctx.needs_input_grad[:3]
        gq = torch.empty_like(q) if need_q else None
        gk = torch.zeros_like(k) if need_k else None
        gv = torch.zeros_like(v) if need_v else None
        rows = max(1, min(N, BACKWARD_CHUNK_BYTES // (4 * M)))
        for b in range(B):
            kT = k[b].t().contiguous() if need_q else None                 # [C, M]
            for r0 in range(0, N, rows):
                r1 = min(N, r0 + rows)
                qr, gr = q[b, r0:r1], g_out[b, r0:r1]
                S = ops.linear(qr, k[b])[0]                                # [rows, M] = q k^T
                P = torch.exp(S.mul_(scale).sub_(lse[b, r0:r1].unsqueeze(1)))
                if need_v:
                    gv[b] += ops.linear_wgrad(P, gr)                       # [M, C] = P^T g
                if not (need_q or need_k):
                    continue
                dP = ops.linear(gr, v[b])[0]                               # [rows, M] = g v^T
                D = (gr * out[b, r0:r1]).sum(dim=1, keepdim=True)
                dS = dP.sub_(D).mul_(P).mul_(scale)
                if need_k:
                    gk[b] += ops.linear_wgrad(dS, qr)                      # [M, C] = dS^T q
                if need_q:
                    acc = None
                    for m0 in range(0, M, _DQ_KEYS):
                        m1 = min(M, m0 + _DQ_KEYS)
                        part = ops.linear(dS[:, m0:m1].contiguous(), kT[:, m0:m1].contiguous())[0]
                        acc = part if acc is None else acc.add_(part)
                    gq[b, r0:r1] = acc                                     # [rows, C] = dS k
        return gq, gk, gv, None


class MultiModalLaplacianODEFunc(ODEFunc):
    """LaplacianODEFunc with ``multi_modal`` (src/function_laplacian_diffusion.py:15-77)."""

    # f depends on x through softmax(Q2(x) k^T): not affine, no dense-output folding
    affine = False
    fold_dense = False

    def __init__(self, in_features, out_features, opt, device):
        super(MultiModalLaplacianODEFunc, self).__init__(opt, device)
        if not (opt.get('multi_modal', False) and opt.get('gnpde_multi_modal', False)):
            raise ValueError("gnpde: MultiModalLaplacianODEFunc needs opt['multi_modal'] and "
                             "opt['gnpde_multi_modal'] (model_configurations.set_function selects it)")
        if opt.get('block', 'constant') != 'constant':
            raise NotImplementedError("gnpde: gnpde_multi_modal serves function='laplacian' under block='constant' "
                                      "only (got block=%r: the reference's attention blocks call their attention "
                                      "layer without y)" % (opt.get('block'),))
        if 'second_modality_dim' not in opt:
            raise ValueError("gnpde: multi_modal needs opt['second_modality_dim'] (the width of y)")
        self.in_features = in_features
        self.out_features = out_features
        # unused by the RHS; kept for state_dict compatibility (:24-27)
        self.w = nn.Parameter(torch.eye(opt['hidden_dim']))
        self.d = nn.Parameter(torch.zeros(opt['hidden_dim']) + 1)
        self.alpha_sc = nn.Parameter(torch.ones(1))
        self.beta_sc = nn.Parameter(torch.ones(1))
        self.y = None
        d2 = int(opt['second_modality_dim'])
        self.Q2 = nn.Linear(in_features, in_features)
        self.init_weights(self.Q2)
        self.V2 = nn.Linear(d2, in_features)
        self.init_weights(self.V2)
        self.K2 = nn.Linear(d2, in_features)
        self.init_weights(self.K2)
        self._qp = None  # (param versions, (Wq, bq)): the contiguous Q2 operands
        self._kv = None  # (y / param versions, (k, v) [B, M, C]): the projected second modality

    def init_weights(self, m):
        """Constant 1e-5 weight init: the fork's own (function_transformer_attention.py:153-157;
        the Laplacian class calls an init_weights it does not define)."""
        if type(m) == nn.Linear:
            nn.init.constant_(m.weight, 1e-5)

    @property
    def scale(self):
        return 1.0 / math.sqrt(self.in_features)  # dk = in_features (:62)

    def supports_feature_padding(self):
        """Q2 reads all C columns of a row: the state is never padded."""
        return False

    def supports_node_layout(self):
        """The user's node numbering only."""
        return False

    def _weights(self):
        if self.edge_weight is None:
            raise RuntimeError("MultiModalLaplacianODEFunc: edge_weight is not set (ODEblock.reset_graph_data)")
        return self.edge_weight

    def _checked_y(self, x):
        y = self.y
        if y is None:
            raise RuntimeError("MultiModalLaplacianODEFunc: y is not set (ODEblock.reset_graph_data(data, dtype, y) "
                               "hands the second modality over)")
        if x.dtype != torch.float32:
            raise NotImplementedError("gnpde: multi_modal runs on fp32 states only (got %s)" % x.dtype)
        if y.dim() != 3 or y.shape[-1] != self.K2.in_features:
            raise ValueError("multi_modal: y must be [B, M, second_modality_dim=%d], got %s"
                             % (self.K2.in_features, tuple(y.shape)))
        if y.shape[0] != x.shape[0]:
            raise ValueError("multi_modal: y holds %d batch elements, x %d" % (y.shape[0], x.shape[0]))
        if y.shape[1] == 0:
            raise ValueError("multi_modal: y has M = 0 tokens (a softmax over no keys)")
        if y.dtype != torch.float32:
            raise TypeError("gnpde: multi_modal: y must be torch.float32, got %s" % y.dtype)
        return y

    def q_params(self):
        """(Wq [C, C], bq [C]) contiguous, cached per parameter version (stable buffers, so
        captured step graphs keep replaying)."""
        ps = (self.Q2.weight, self.Q2.bias)
        key = tuple(_tensor_key(t) for t in ps)
        if self._qp is None or self._qp[0] != key:
            self._qp = (key, tuple(t.detach().contiguous() for t in ps))
        return self._qp[1]

    def kv(self, y):
        """(k, v) = (K2(y), V2(y)) [B, M, C]: projected once per (y, parameter version).  A
        new y of the same shape is projected INTO the cached buffers, so the captured step
        graphs that read them keep replaying (only the no-grad path reads this cache)."""
        ps = (y, self.K2.weight, self.K2.bias, self.V2.weight, self.V2.bias)
        key = tuple(_tensor_key(t) for t in ps)
        hit = self._kv
        if hit is not None and hit[0] == key:
            return hit[1]
        B, M = y.shape[0], y.shape[1]
        yd = y.detach()
        k = ops.linear(yd, self.K2.weight.detach(), self.K2.bias.detach())[0].view(B, M, -1)
        v = ops.linear(yd, self.V2.weight.detach(), self.V2.bias.detach())[0].view(B, M, -1)
        if hit is not None and hit[1][0].shape == k.shape and hit[1][0].device == k.device:
            hit[1][0].copy_(k)
            hit[1][1].copy_(v)
            k, v = hit[1]
        self._kv = (key, (k, v))
        return k, v

    def cross_attention(self, x):
        """x~ [B, N, C] of the current y, without autograd."""
        y = self._checked_y(x)
        Wq, bq = self.q_params()
        k, v = self.kv(y)
        q = ops.linear(x.detach(), Wq, bq)[0].view(x.shape)
        return ops.cross_attention(q, k, v, self.scale)

    def graph_capture_state(self, x):
        """What a captured fused step reads (gnpde.integrator._capture_state): the device
        CSR + plan, the CSR-order weights, the cached Q2 operands and k / v and, with
        add_source, the stable x0 buffer."""
        g = self.graph_for(x)
        k, v = self.kv(self._checked_y(x))
        Wq, bq = self.q_params()
        st = [g, self.csr_weights(g, self._weights(), 'w'), Wq, bq, k, v]
        if self.opt.get('add_source', False):
            st.append(self.stable_x0(x))
        return st

    def sparse_multiply(self, x):
        """A x (:39-58) — K1 without the epilogue."""
        g = self.graph_for(x)
        return ops.spmm_rhs(g, self.csr_weights(g, self._weights(), 'w'), x, rhs=False)

    def rhs_stage(self, t, x, stage):
        """forward(t, x), then the solver's stage combination as a pass of its own
        (gnpde.integrator, no-grad solvers): it reads the solver's state x, not x~."""
        self._rhs(x, stage)

    def forward(self, t, x):  # the t param is needed by the ODE solver.
        return self._rhs(x, None)

    def _rhs(self, x, stage):
        if self.nfe > self.opt["max_nfe"]:
            raise MaxNFEException
        self.nfe += 1
        y = self._checked_y(x)
        g = self.graph_for(x)
        w = self._weights()
        w_csr = self.csr_weights(g, w, 'w')
        add_source = bool(self.opt.get('add_source', False))
        if add_source and self.x0 is None:
            raise RuntimeError("MultiModalLaplacianODEFunc: add_source needs x0 (ODEblock.set_x0)")
        alpha_sigmoid = not self.opt.get('no_alpha_sigmoid', False)
        if stage is None and _needs_grad(x, self.alpha_train, self.beta_train, y, *self.Q2.parameters(),
                                         *self.K2.parameters(), *self.V2.parameters()):
            x0 = self.x0.float() if add_source else None
            q = _MixProject.apply(x, self.Q2.weight, self.Q2.bias)
            k = _MixProject.apply(y, self.K2.weight, self.K2.bias)
            v = _MixProject.apply(y, self.V2.weight, self.V2.bias)
            xt = _CrossAttention.apply(q, k, v, self.scale)
            return _LaplacianRHS.apply(xt, self.alpha_train, self.beta_train, w.detach(), g, w_csr,
                                       lambda: self.csr_weights(g, w, 'w', transpose=True), x0, alpha_sigmoid,
                                       add_source)
        # fused stages (and their captured graphs) read a stable x0 buffer (ODEFunc.stable_x0)
        x0 = (self.stable_x0(x) if stage is not None else self.x0.float()) if add_source else None
        xt = self.cross_attention(x)
        f = ops.spmm_rhs(g, w_csr, xt, x0=x0, alpha=self.alpha_train.detach(), beta=self.beta_train.detach(),
                         rhs=True, alpha_sigmoid=alpha_sigmoid, add_source=add_source)
        if stage is None:
            return f
        ops.stage_apply(stage, f, x, x)
        return None
