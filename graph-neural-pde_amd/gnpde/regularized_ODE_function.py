"""ODE regularisers (reference src/regularized_ODE_function.py, src/base_classes.py:11-30).

Opt-in: ``opt['gnpde_regularization'] = True``.  The reference's lines do not run as
written (``RegularizedODEfunc.forward`` indexes the state tuple with ``state[:, 0]``;
``directional_derivative`` ends in ``.view(x.size(0), x.size(1) -1)``), so they are read
as they are meant:

* state ``(x, r_1, ..., r_nreg)``: x [B,N,C] fp32, every r_j [B,N], zero at t[0];
* ``RegularizedODEfunc.forward(t, state) = (f, reg_fn_1(x, t, f, odefunc), ...)``, f = odefunc(t, x);
* ``quadratic_cost`` (key ``kinetic_energy``): e[b,n] = 1/(2C) sum_c f[b,n,c]^2 (as written);
* ``directional_derivative`` (key ``directional_penalty``): with v = (df/dx)^T f, the value of
  ``autograd.grad(dx, x, dx, create_graph=True)``, d[b,n] = 1/(2C) sum_c v[b,n,c]^2 — what the
  reference's ``total_derivative`` returns for f + 0*t.  For the Laplacian RHS f = a (A x - x)
  [+ b x0] the Jacobian does not depend on x: v = a (A^T f - f), one K1 launch over the CSC, a
  first-order autograd Function of its own (no double backward anywhere).  Any other ODE function
  raises: its Jacobian depends on x and the custom Functions have no double backward.

C is the state's true width (twice the hidden dimension under ``augment``), never a padded one.

``jacobian_norm2`` and ``total_deriv`` raise NotImplementedError naming the key: the
reference's ``total_derivative`` raises by itself for a time-independent f, and the Jacobian's
Frobenius term is a state-independent constant for the Laplacian.

The row sums and their backward are HIP passes (ops.row_energy, ops.row_axpy).
"""
import torch
from torch import nn

from . import ops

OPT_KEY = 'gnpde_regularization'


def not_opted_in(what):
    return NotImplementedError("gnpde: %s: ODE regularisation terms are opt-in: set opt['%s'] = True "
                               "(kinetic_energy and directional_penalty; gnpde.regularized_ODE_function)"
                               % (what, OPT_KEY))


def _check_state(f):
    if f.dtype != torch.float32:
        raise NotImplementedError("gnpde: ODE regularisers take an fp32 state (got %s)" % f.dtype)
    if f.dim() != 3:
        raise ValueError("gnpde: ODE regularisers take a [B,N,C] state")


class _RowEnergy(torch.autograd.Function):
    """e[b,n] = scale * sum_c f[b,n,c]^2 (ops.row_energy); backward g_f = 2 scale g_e (row-scale) f
    (ops.row_axpy)."""

    @staticmethod
    def forward(ctx, f, scale):
        f = f.contiguous()
        ctx.save_for_backward(f)
        ctx.scale = scale
        return ops.row_energy([f], [scale])

    @staticmethod
    def backward(ctx, ge):
        f, = ctx.saved_tensors
        return ops.row_axpy(None, [(2.0 * ctx.scale, ge.contiguous().float(), f)]), None


def quadratic_cost(x, t, dx, unused_context):
    """src/regularized_ODE_function.py:66-69: 0.5 * mean_c dx^2, for any ODE function."""
    del x, t, unused_context
    _check_state(dx)
    return _RowEnergy.apply(dx, 0.5 / dx.shape[-1])


class _LaplacianTransposedRHS(torch.autograd.Function):
    """v = a (A^T f - f), a = sigma(alpha_train) or alpha_train: the vector-Jacobian product of the
    Laplacian RHS with f itself (K1 over the CSC).  Backward: to f, a (A g - g) (K1 over the CSR);
    to alpha, a'(alpha) <g, (A^T - I) f>; to the weights, a <f[src(e)], g[dst(e)]> — the RHS
    backward's SDDMM with its operands swapped, since d v[dst(e)] / d w_e = a f[src(e)]."""

    @staticmethod
    def forward(ctx, f, alpha_train, w_src, g, w_csr, w_csc, alpha_sigmoid):
        f = f.contiguous()
        v = ops.spmm_rhs(g, w_csc, f, alpha=alpha_train.detach(), rhs=True, alpha_sigmoid=alpha_sigmoid,
                         transpose=True)
        ctx.save_for_backward(f, alpha_train)
        ctx.g, ctx.w_csr, ctx.w_csc, ctx.alpha_sigmoid = g, w_csr, w_csc, alpha_sigmoid
        ctx.w_heads = w_src.shape[2] if w_src.dim() == 3 else 1
        ctx.w_shape = w_src.shape
        return v

    @staticmethod
    def backward(ctx, gv):
        f, alpha_train = ctx.saved_tensors
        gv = gv.contiguous()
        g = ctx.g
        gf = ga = gw = None
        if ctx.needs_input_grad[0]:
            gf = ops.spmm_rhs(g, ctx.w_csr, gv, alpha=alpha_train.detach(), rhs=True, alpha_sigmoid=ctx.alpha_sigmoid)
        if ctx.needs_input_grad[1]:
            one = torch.ones((), dtype=torch.float32, device=f.device)
            d = ops.spmm_rhs(g, ctx.w_csc, f, alpha=one, rhs=True, alpha_sigmoid=False, transpose=True)
            s = ops.dot(gv, d).to(alpha_train.dtype)
            if ctx.alpha_sigmoid:
                sg = torch.sigmoid(alpha_train.detach())
                s = s * sg * (1 - sg)
            ga = s.reshape(alpha_train.shape)
        if ctx.needs_input_grad[2]:
            gw = ops.sddmm(g, f, gv, heads=ctx.w_heads, alpha=alpha_train.detach(),
                           alpha_sigmoid=ctx.alpha_sigmoid).view(ctx.w_shape)
        return gf, ga, gw, None, None, None, None


def laplacian_vjp(odefunc, f):
    """v = (df/dx)^T f of a LaplacianODEFunc, under autograd (f, alpha_train and the weights)."""
    g = odefunc.graph_for(f)
    w, tag = odefunc._weights_tensor()
    w_csr = odefunc.csr_weights(g, w, tag)
    w_csc = odefunc.csr_weights(g, w, tag, transpose=True)
    if not isinstance(w_csr, torch.Tensor) or not isinstance(w_csc, torch.Tensor):
        # the sampled graph's compacted weights (HardAttODEblock training) cover K1 alone
        full = lambda t: t.full if isinstance(t, ops.CompactWeights) else t  # noqa: E731
        w_csr, w_csc = full(w_csr), full(w_csc)
    w_src = w.detach() if odefunc.adjoint_const_weights else w
    return _LaplacianTransposedRHS.apply(f, odefunc.alpha_train, w_src, g, w_csr, w_csc,
                                         not odefunc.opt.get('no_alpha_sigmoid', False))


def directional_derivative(x, t, dx, odefunc):
    """src/regularized_ODE_function.py:57-63 as meant: 0.5 * mean_c ((df/dx)^T dx)^2."""
    del x, t
    from .function_laplacian_diffusion import LaplacianODEFunc
    if not isinstance(odefunc, LaplacianODEFunc):
        raise NotImplementedError("gnpde: directional_penalty is built for LaplacianODEFunc (a Jacobian that does "
                                  "not depend on x); %s would need a double backward of its custom autograd "
                                  "Functions" % odefunc.__class__.__name__)
    _check_state(dx)
    return _RowEnergy.apply(laplacian_vjp(odefunc, dx), 0.5 / dx.shape[-1])


# what the fused regularised solve (integrator._LaplacianRegFixedGridFn) carries by itself
quadratic_cost.gnpde_reg_kind = 'kinetic'
directional_derivative.gnpde_reg_kind = 'directional'

# src/base_classes.py:11-16, in its order
REGULARIZATION_FNS = (
    ("kinetic_energy", quadratic_cost),
    ("jacobian_norm2", None),
    ("total_deriv", None),
    ("directional_penalty", directional_derivative),
)
_OUT_OF_SCOPE = {
    "jacobian_norm2": "for the Laplacian RHS the Jacobian's Frobenius term is a state-independent constant, and "
                      "the other functions' would need a double backward",
    "total_deriv": "the reference's total_derivative raises by itself for a time-independent f (use "
                   "directional_penalty, the same value)",
}


def create_regularization_fns(args):
    """src/base_classes.py:19-30: (fns, coeffs) of the keys of ``args`` that are present and not
    None, in the reference's order."""
    fns, coeffs = [], []
    for key, fn in REGULARIZATION_FNS:
        if args.get(key) is None:
            continue
        if fn is None:
            raise NotImplementedError("gnpde: regulariser %r is out of scope: %s" % (key, _OUT_OF_SCOPE[key]))
        fns.append(fn)
        coeffs.append(args[key])
    return fns, coeffs


class RegularizedODEfunc(nn.Module):
    """src/regularized_ODE_function.py:8-33.  ``odefunc`` keeps the reference's attribute path
    (``reg_odefunc.odefunc``: the first copy an ODEblock builds, with its state_dict keys).
    ``rhs(odefunc, t, state)`` evaluates the regularised right-hand side of any copy: an ODEblock's
    training solve integrates the block's own ``odefunc`` — the copy evaluation integrates, whose
    graph, x0 and attention the block's forward has just set — where the reference would integrate
    ``reg_odefunc.odefunc``, which evaluation never reads."""

    def __init__(self, odefunc, regularization_fns):
        super(RegularizedODEfunc, self).__init__()
        self.odefunc = odefunc
        self.regularization_fns = regularization_fns

    def rhs(self, odefunc, t, state):
        opt = getattr(odefunc, 'opt', None)
        if not (isinstance(opt, dict) and opt.get(OPT_KEY)):
            raise not_opted_in("RegularizedODEfunc.forward")
        x = state[0]
        dx = odefunc(t, x)
        if len(state) > 1:
            return (dx,) + tuple(fn(x, t, dx, odefunc) for fn in self.regularization_fns)
        return dx

    def forward(self, t, state):
        return self.rhs(self.odefunc, t, state)

    def bound(self, odefunc):
        """The regularised RHS of ``odefunc`` as the solver's callable."""
        return _BoundRegRHS(self, odefunc)


class _BoundRegRHS(object):
    def __init__(self, reg, odefunc):
        self.reg, self.odefunc = reg, odefunc
        self.regularization_fns = reg.regularization_fns

    def __call__(self, t, state):
        return self.reg.rhs(self.odefunc, t, state)
