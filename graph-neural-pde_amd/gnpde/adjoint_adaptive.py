"""Fused adaptive adjoint of the Laplacian RHS.

Three of the reference's best_params train with an ADAPTIVE adjoint method
(src/best_params.py:3-5: Pubmed adaptive_heun — the reference's default
adjoint_method, src/run_GNN.py:334 —, CoauthorCS and Computers dopri5;
src/base_classes.py:45-49 and src/block_constant.py:34-44 pass adjoint_method,
adjoint_atol / adjoint_rtol from tol_scale_adjoint).  torchdiffeq's
odeint_adjoint (0.2.x OdeintAdjointMethod, not installed here: restated, parity
with it unpinned) integrates the augmented state [y | a | theta] from t[-1] back
to t[0] in s = -t with the same adaptive solver as the forward and the mixed norm
(the max over the components of their RMS norms).  For the Laplacian
f(y) = sigma(alpha)(A y - y) [+ beta x0] (src/function_laplacian_diffusion.py)
the augmented RHS is, with L = sigma(alpha)(A - I):

    dy/ds     = -f(y)                        K1 over the CSR with alpha -> -sigma(alpha), beta -> -beta
    da/ds     = L^T a                        K1 over the CSC
    dalpha/ds = (1 - sigma(alpha)) <L^T a, y>  the CSC launch's dot rows (ABI 7: beside its error rows)
    dbeta/ds  = <a, x0>                      (add_source) one fp64 dot per stage

and every other parameter's component has derivative 0 (so its value and error
stay 0).  integrator._OdeintAdjoint runs that as torchdiffeq does — a packed
[y | a | params] vector, torch stage combinations, per-component norms — at
~0.64 ms per augmented evaluation on G-arxiv, 0.45 of it solver glue.

This module runs the same loop (integrator._RKAdaptive: the tableau, the initial
step selection, the controller, the dense output) with the y and a halves kept in
one packed device state [2, B, N, C] and every stage combination in the K1
epilogues (solver_common._AdaptivePlan: launch i of a step evaluates both halves at
stage input X_i and writes X_{i+1} and the error rows of its half; the CSC launch
adds the alpha integrand's rows <L^T a_i, y_i>).  The scalar components (alpha,
beta) are integrated on the host in fp64 from the per-stage sums: one segment-sum
launch per step reduces the two halves' error rows and the stages' alpha rows, and
the host reads that record once per step (accept / reject and the next dt, as
torchdiffeq's loop).  Step arithmetic: fp32 state, fp64 error norms and scalar
components (the restated loop runs every component in fp32).
"""
import math

import numpy as np
import torch

from . import ops
from .solver_common import (_AdaptiveState, _adaptive_plan, _node_layout, _to_internal, _to_user, check_step,
                            dense_combo, dense_weights, laplacian_operands, next_dt, rotate)
from .utils import MaxNFEException


def _f32(v):
    return float(np.float32(v))


class AdaptiveAdjoint(object):
    """The backward of odeint_adjoint for a LaplacianODEFunc with an adaptive
    adjoint method: ``run(t_h, ans, grad_y)`` -> (grad of y0, alpha's gradient, beta's
    or None without add_source), the scalars as host floats."""

    def __init__(self, func, params, method, rtol, atol, options=None):
        self.func, self.params = func, tuple(params)
        self.method = method
        self.plan = _adaptive_plan(method)
        self.order = float(self.plan.order)
        self.rtol, self.atol = float(rtol), float(atol)
        opts = dict(options or {})
        self.first_step = opts.get('first_step')
        self.max_num_steps = opts.get('max_num_steps', 2 ** 31 - 1)
        self.safety, self.ifactor, self.dfactor = 0.9, 10.0, 0.2
        self.n_steps = 0
        self.add_source = bool(func.opt.get('add_source', False))

    # ------------------------------------------------------------------ setup
    def _setup(self, y_like):
        P, func = self.plan, self.func
        C = y_like.shape[-1]
        packed = torch.empty((2,) + tuple(y_like.shape), dtype=torch.float32, device=y_like.device)
        st = _AdaptiveState(P, packed, False)
        self.bufs = st.bufs
        self.scale = st.scale
        R = y_like.numel() // C
        self.R, self.C, self.ny = R, C, y_like.numel()
        ns = P.ns
        # row channels: 0 / 1 the y / a error rows, 2 + j the alpha rows of stage derivative j
        self.rows = torch.zeros((3 + ns, R), dtype=torch.float64, device=y_like.device)
        # the step's record: the segment sums (3 + ns), the beta stage dots (ns + 1), the initial
        # step's squared sums (4: y / a halves, two each)
        self.nrec = 3 + ns + (ns + 1) + 4
        self.rec = torch.zeros(self.nrec, dtype=torch.float64, device=y_like.device)
        self.rec_host = torch.empty(self.nrec, dtype=torch.float64, pin_memory=True)
        o = laplacian_operands(func, y_like, csr=True)
        self.g, self.w_csr, self.w_csc, self.x0 = o.g, o.w_csr, o.w_csc, o.x0
        alpha = o.alpha
        self.alpha = alpha.float().reshape(()).contiguous()
        # y-half: -f(y) = (-sigma(alpha))(A y - y) + (-beta) x0 from the same K1 (alpha taken as given)
        self.neg_sig = (-torch.sigmoid(alpha.float())).reshape(()).contiguous()
        self.neg_beta = (-o.beta.float()).reshape(()).contiguous()
        self.one_minus_sig = 1.0 - 1.0 / (1.0 + math.exp(-float(alpha)))

    def _read(self):
        self.rec_host.copy_(self.rec, non_blocking=True)
        torch.cuda.current_stream(self.rec.device).synchronize()
        return self.rec_host.tolist()

    # ------------------------------------------------------------------ RHS launches
    def _count(self, n=1):
        f = self.func
        if f.nfe > f.opt["max_nfe"]:
            raise MaxNFEException
        f.nfe += n

    def _rhs(self, x, stage_y, stage_a, dot_row, beta_slot):
        """One augmented evaluation at the packed stage input x: the y-half over the
        CSR, the a-half over the CSC with the alpha rows <L^T a, y> into rows[dot_row],
        and (add_source) <a, x0> into rec[beta_slot]."""
        self._count()
        ops.spmm_rhs(self.g, self.w_csr, x[0], x0=self.x0, alpha=self.neg_sig, beta=self.neg_beta, rhs=True,
                     alpha_sigmoid=False, add_source=self.add_source, stage=stage_y)
        stage_a.dot = (x[0], self.rows[dot_row], 1.0, False)
        ops.spmm_rhs(self.g, self.w_csc, x[1], alpha=self.alpha, rhs=True, alpha_sigmoid=True, transpose=True,
                     stage=stage_a)
        if self.add_source:
            ops.dot(x[1], self.x0, out=self.rec[beta_slot:beta_slot + 1])

    def _beta_slot(self, j):
        return 3 + self.plan.ns + j

    def _launch(self, i, mid):
        P, b = self.plan, self.bufs
        x = b['X%d' % i]
        j = i + 1
        stages = []
        for h in (0, 1):  # the plan's symbols resolved to half h of the packed buffers
            outs, err, err_y1, store = P.launch(i, mid, lambda s: (x if s == 'X' else b[s])[h])
            if err is not None:
                err = (self.rows[h], err, b['Y'][h], err_y1, self.atol, self.rtol)
            stages.append(ops.Stage(f_out=b['K%d' % j][h] if store else None, outs=outs, err=err, scale=self.scale))
        self._rhs(x, stages[0], stages[1], 2 + j, self._beta_slot(j))

    def _step(self, mid):
        """Enqueue one step: the first stage input X0 = Y + dt b00 K0 (one pass over the
        packed state), the ns launches of each half, one segment-sum launch."""
        P, b = self.plan, self.bufs
        ops.stage_apply(ops.Stage(outs=[(b['X0'], b['Y'], 1.0, 0.0, [(b['K0'], P.beta[0][0])])], scale=self.scale),
                        None, None, b['Y'])
        for i in range(P.ns):
            self._launch(i, mid)
        ops.segment_sums(self.rows, self.rec[:3 + P.ns])

    # ------------------------------------------------------------------ scalar components
    def _ratio(self, e2y, e2a, s0, s1, k, dt):
        """torchdiffeq's mixed error norm: max of the halves' RMS error ratios and the
        scalar components' |e| / tol; s1 = the scalars at the step's end."""
        P = self.plan
        r = max(math.sqrt(e2y / self.ny), math.sqrt(e2a / self.ny))
        for c in range(len(s0)):
            e = dt * sum(P.c_err[j] * k[c][j] for j in range(P.ns + 1) if P.c_err[j] != 0.0)
            tol = self.atol + self.rtol * max(abs(s0[c]), abs(s1[c]))
            r = max(r, abs(e) / tol)
        return r

    def _initial_step(self, s0, k0):
        """_select_initial_step over the mixed norm: the halves' squared sums on the
        device (gnpde_scaled_sq_sums_f32), the scalar components on the host; the probe
        z0 + h0 f0 is one stage pass and one augmented evaluation.  h0 and the result
        are rounded to fp32 as torch computes them on an fp32 state."""
        b, n = self.bufs, float(self.ny)
        off = 3 + self.plan.ns + self.plan.ns + 1
        ops.scaled_sq_sums(b['Y'][0], b['K0'][0], None, self.atol, self.rtol, self.rec[off:off + 2])
        ops.scaled_sq_sums(b['Y'][1], b['K0'][1], None, self.atol, self.rtol, self.rec[off + 2:off + 4])
        r = self._read()
        sc = [self.atol + abs(v) * self.rtol for v in s0]
        d0 = max([math.sqrt(r[off] / n), math.sqrt(r[off + 2] / n)] + [abs(v) / s for v, s in zip(s0, sc)])
        d1 = max([math.sqrt(r[off + 1] / n), math.sqrt(r[off + 3] / n)] + [abs(v) / s for v, s in zip(k0, sc)])
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else _f32(0.01 * d0 / d1)
        # probe f(z0 + h0 f0): stage input in X0, its derivative in Y1 (both free before the first step)
        self.scale.fill_(h0)
        ops.stage_apply(ops.Stage(outs=[(b['X0'], b['Y'], 1.0, 0.0, [(b['K0'], 1.0)])], scale=self.scale), None,
                        None, b['Y'])
        slot = 2 + self.plan.ns  # the last stage's alpha rows: free before the first step
        self._rhs(b['X0'], ops.Stage(f_out=b['Y1'][0]), ops.Stage(f_out=b['Y1'][1]), slot, self._beta_slot(self.plan.ns))
        ops.segment_sums(self.rows[slot:slot + 1], self.rec[slot:slot + 1])
        ops.scaled_sq_sums(b['Y'][0], b['K0'][0], b['Y1'][0], self.atol, self.rtol, self.rec[off:off + 2])
        ops.scaled_sq_sums(b['Y'][1], b['K0'][1], b['Y1'][1], self.atol, self.rtol, self.rec[off + 2:off + 4])
        r = self._read()
        k1 = [self.one_minus_sig * r[slot]]
        if self.add_source:
            k1.append(r[self._beta_slot(self.plan.ns)])
        d2 = max([math.sqrt(r[off] / n), math.sqrt(r[off + 2] / n)] +
                 [abs(a - c) / s for a, c, s in zip(k1, k0, sc)]) / h0
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(1e-6, h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1.0 / self.order)
        return _f32(min(100.0 * h0, h1))

    # ------------------------------------------------------------------ one interval
    def _interval(self, t0, t1, s0):
        """Integrate the packed state in bufs['Y'] (y | a) and the scalars s0 from
        s = t0 to t1 > t0; returns (the a-half at t1, the scalars at t1)."""
        P, b = self.plan, self.bufs
        ns = P.ns
        # f0 = f(z0): K0 and the scalars' derivatives
        self._rhs(b['Y'], ops.Stage(f_out=b['K0'][0]), ops.Stage(f_out=b['K0'][1]), 2, self._beta_slot(0))
        ops.segment_sums(self.rows[2:3], self.rec[2:3])
        if self.first_step is None:
            r = self._read()
            k0 = [self.one_minus_sig * r[2]] + ([r[self._beta_slot(0)]] if self.add_source else [])
            dt = self._initial_step(s0, k0)
        else:
            dt = float(self.first_step)
            r = self._read()
            k0 = [self.one_minus_sig * r[2]] + ([r[self._beta_slot(0)]] if self.add_source else [])
        t_cur = t0
        last = None
        while t1 > t_cur:
            check_step(t_cur, dt, self.n_steps, self.max_num_steps)
            mid = t_cur + dt >= t1
            self.scale.fill_(dt)
            self._step(mid)
            r = self._read()
            ks = [k0[0]] + [self.one_minus_sig * r[2 + j] for j in range(1, ns + 1)]
            kk = [ks]
            if self.add_source:
                kk.append([k0[1]] + [r[self._beta_slot(j)] for j in range(1, ns + 1)])
            s1 = [s0[c] + dt * sum(P.c_sol[j] * kk[c][j] for j in range(ns + 1) if P.c_sol[j] != 0.0)
                  for c in range(len(s0))]
            ratio = self._ratio(r[0], r[1], s0, s1, kk, dt)
            if ratio <= 1:
                last = (t_cur, dt, dict(b), list(s0), list(s1), [list(v) for v in kk])
                t_cur = t_cur + dt
                s0 = s1
                k0 = [v[ns] for v in kk]
                rotate(b, P)
            dt = next_dt(dt, ratio, self.order, self.safety, self.ifactor, self.dfactor)
            self.n_steps += 1
        if last is None or t1 == t_cur:
            return self.bufs['Y'][1], s0
        return self._interp(last, t1, t_cur)

    def _interp(self, last, t, t1):
        """torchdiffeq's 4th-order dense output of the last accepted step (integrator.
        _RKAdaptive._interp) for the a-half (one stage pass) and the scalars."""
        P = self.plan
        t0, dt, d, s0, s1, kk = last
        wts = cy0, cy1, cym, cf0, cf1 = dense_weights((t - t0) / (t1 - t0), dt)
        ns = P.ns
        h = 1
        y0, y1, f0, f1 = d['Y'][h], d['Y1'][h], d['K0'][h], d['K%d' % ns][h]
        # (every [h] is a fresh view: K0's c_mid term and f0's stay two entries, which the Stage merges by address)
        cb, cf_f1, terms = dense_combo(P, wts, dt, y1, f0, f1, lambda j: d['K%d' % j][h])
        out = torch.empty_like(y0)
        ops.stage_apply(ops.Stage(outs=[(out, y0, cb, cf_f1, terms)]), f1, y0, y0)
        sv = []
        for c in range(len(s0)):
            k = kk[c]
            ymid = s0[c] + dt * sum(P.c_mid[j] * k[j] for j in range(ns + 1))
            sv.append(cy0 * s0[c] + cy1 * s1[c] + cym * ymid + cf0 * k[0] + cf1 * k[ns])
        return out, sv

    # ------------------------------------------------------------------ the backward
    def run(self, t_h, ans, grad_y):
        func = self.func
        lay = _node_layout(func, ans[0])
        if lay is not None:
            func._layout = lay
        try:
            self._setup(ans[0])
            b = self.bufs
            _to_internal(grad_y[-1], lay, out=b['Y'][1])
            s = [0.0] + ([0.0] if self.add_source else [])
            for i in range(len(t_h) - 1, 0, -1):
                _to_internal(ans[i], lay, out=b['Y'][0])
                if i < len(t_h) - 1:
                    _to_internal(a_user, lay, out=b['Y'][1])
                a_end, s = self._interval(-t_h[i], -t_h[i - 1], s)
                a_user = torch.empty_like(grad_y[i - 1])
                _to_user(a_end, a_user, lay)
                a_user += grad_y[i - 1]
        finally:
            func._layout = None
        return a_user, s[0], (s[1] if self.add_source else None)
