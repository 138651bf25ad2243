"""Backprop through an adaptive solve of the Laplacian RHS as ONE autograd node.

The attention-block datasets that train WITHOUT the adjoint (src/best_params.py:1-2:
Cora, Citeseer — block attention, dopri5, adjoint False) differentiate straight through
torchdiffeq's adaptive loop: autograd records every stage combination and every RHS
(src/block_transformer_attention.py:40-52 calls odeint with the attention weights from an
autograd-tracked layer), and the step sizes are constants of the graph (torchdiffeq's
_select_initial_step and _optimal_step_size run under no_grad).  The gradient is the
discrete adjoint of the ACCEPTED steps (a rejected step's values are never used) and of
the dense output.  The restated loop (integrator._RKAdaptive) does exactly that through
per-RHS autograd nodes: ~175 us of host work per RHS on a Cora-sized graph.

Here (the Laplacian f(y) = L y + s, L = sigma(alpha)(A(w) - I), s = beta x0):

forward  — the tableau's stage plan (solver_common._AdaptivePlan) with every combination and
           the error rows in the K1 epilogues, each accepted step's stage inputs kept
           (Yin_i, i < ns), torchdiffeq's controller on the host (one read per step);
backward — per accepted step, last first, the transposed stages (gather form):
             Yin_bar_i = L^T kbar_{i+1} [+ ybar_1 on the FSAL last stage]   (K1 over the CSC)
             kbar_j    = dt sum_{m >= j} beta[m][j] Yin_bar_m [+ dt c_sol[j] ybar_1, non-FSAL]
             ybar_0    = sum_m Yin_bar_m [+ ybar_1, non-FSAL]
           launch i (input kbar_{i+1}) writes Yin_bar_i and kbar_i (launch 0: kbar_0 and
           ybar_0) from the rows it holds; kbar_0 is the previous step's f1 adjoint (FSAL,
           and torchdiffeq's k[-1] for the non-FSAL pairs);
parameters — alpha: (1 - sigma) sum <L^T kbar, Yin> (the CSC launches' dot rows, fp64);
           beta: <sum kbar, x0>; the weights: ONE SDDMM over the stacked pairs
           (kbar_{i+1}, Yin_i) of every stage of every step (features concatenated:
           sum_s <kbar_s[src], Yin_s[dst]> sigma / heads).

The dense output's adjoint seeds the last step's (y0, y1, k_j); an output at a step
boundary adds to that state's adjoint.  Parity: against the restated loop's autograd
(tests/test_gpu_adaptive_backprop.py).  User numbering (the small graphs this path
serves); no hipGraph capture.
"""
import math

import torch

from . import ops
from .solver_common import _adaptive_plan, alpha_grad, check_step, dense_weights, next_dt, rotate


class AdaptiveBackprop(object):
    """One solve: ``forward()`` -> solution; ``backward(grad_sol, operands, w)`` -> (ybar, alpha,
    beta, w grads), reading the module's state only as the LaplacianOperands snapshot the caller
    took in forward (integrator._LaplacianAdaptiveFn)."""

    def __init__(self, func, y0, t_h, method, rtol, atol, first_step=None, max_num_steps=2 ** 31 - 1):
        self.func, self.y0, self.t_h = func, y0.contiguous(), list(t_h)
        self.plan = _adaptive_plan(method)
        self.order = float(self.plan.order)
        self.rtol, self.atol = float(rtol), float(atol)
        self.first_step, self.max_num_steps = first_step, max_num_steps
        self.safety, self.ifactor, self.dfactor = 0.9, 10.0, 0.2
        self.n_steps = 0
        self.add_source = bool(func.opt.get('add_source', False))

    # ------------------------------------------------------------------ forward
    def _rhs(self, t, x, stage):
        # (rhs_stage counts the evaluation and raises MaxNFEException past opt['max_nfe'], as forward())
        self.func.rhs_stage(t, x, stage)

    def _select_initial_step(self, t0):
        """torchdiffeq's _select_initial_step on the device (gnpde_initial_step_f32: two
        fixed-order reductions; the probe y0 + h0 f0 one stage pass and one RHS); no_grad
        in torchdiffeq, a constant of the gradient here too."""
        y, k0 = self.y0, self.K0
        h = torch.zeros(3, dtype=torch.float64, device=y.device)
        hf = torch.zeros((), dtype=torch.float32, device=y.device)
        ops.initial_step(y, k0, None, self.atol, self.rtol, self.order, h, hf)
        probe, f1 = torch.empty_like(y), torch.empty_like(y)
        ops.stage_apply(ops.Stage(outs=[(probe, y, 1.0, 0.0, [(k0, 1.0)])], scale=hf), None, None, y)
        self._rhs(t0, probe, ops.Stage(f_out=f1))
        ops.initial_step(y, k0, f1, self.atol, self.rtol, self.order, h, None)
        return float(h[2])

    def _attempt(self, y, t_cur, dt):
        """One step from y with f0 in bufs['K0']: fresh stage-input buffers (kept when
        the step is accepted); returns (stage inputs [ns], y1, err2 device scalar)."""
        P, b = self.plan, self.bufs
        ns = P.ns
        X = [torch.empty_like(y) for _ in range(ns)]
        y1 = X[ns - 1] if P.fsal else torch.empty_like(y)
        b['Y'] = y
        for i in range(ns):
            b['X%d' % i] = X[i]
        b['Y1'] = y1
        ops.stage_apply(ops.Stage(outs=[(X[0], y, 1.0, 0.0, [(b['K0'], dt * P.beta[0][0])])]), None, None, y)
        for i in range(ns):
            ti = t_cur + dt if P.alpha[i] == 1. else t_cur + P.alpha[i] * dt
            # (the host's dt in the coefficients; every k_{i+1} is stored: the dense output's adjoint)
            outs, err, err_y1, _ = P.launch(i, True, lambda s: X[i] if s == 'X' else b[s], mult=dt)
            if err is not None:
                err = (self.rows, err, y, err_y1, self.atol, self.rtol)
            self._rhs(ti, X[i], ops.Stage(f_out=b['K%d' % (i + 1)], outs=outs, err=err))
        return X, y1, ops.sum_f64(self.rows)

    def _interp_into(self, out, step, t):
        """The dense output of an accepted step from the step's y0, y1 and the k's still in
        bufs, as one pass; returns the coefficients (on y0, y1, k_0..k_ns) its adjoint needs.
        The pass keeps every k_j as an operand in stage order (the adjoint's coefficient per
        k_j), not solver_common.dense_combo's merged form with f1 as the f input."""
        P, b = self.plan, self.bufs
        t0, dt, y0, y1 = step['t0'], step['dt'], step['y0'], step['y1']
        ns = P.ns
        cy0, cy1, cym, cf0, cf1 = dense_weights((t - t0) / dt, dt)
        ck =[cym * dt * P.c_mid[j] for j in range(ns + 1)]
        ck[0] += cf0
        ck[ns] += cf1
        terms = [(b['K%d' % j], ck[j]) for j in range(ns + 1) if ck[j] != 0.0]
        if len(terms) <= 5:
            ops.stage_apply(ops.Stage(outs=[(out, y0, cy0 + cym, 0.0, terms + [(y1, cy1)])]), None, None, y0)
        else:
            tmp = torch.empty_like(out)
            ops.stage_apply(ops.Stage(outs=[(tmp, y0, cy0 + cym, 0.0, terms[:5])]), None, None, y0)
            ops.stage_apply(ops.Stage(outs=[(out, tmp, 1.0, 0.0, terms[5:] + [(y1, cy1)])]), None, None, y0)
        return {'y0': cy0 + cym, 'y1': cy1, 'k': ck}

    def forward(self):
        """The adaptive loop (integrator._RKAdaptive.integrate) with fused stages; returns
        the solution [len(t), *y0.shape] and keeps what the backward needs."""
        P, func = self.plan, self.func
        y0 = self.y0
        ns = P.ns
        th = self.t_h
        R = y0.numel() // y0.shape[-1]
        self.rows = torch.empty(R, dtype=torch.float64, device=y0.device)
        self.bufs = b = {}
        for j in range(ns + 1):
            b['K%d' % j] = torch.empty_like(y0)
        if any(L['epart'] is not None for L in P.launches):
            b['E'] = torch.empty_like(y0)
        self.K0 = b['K0']
        sol = torch.empty((len(th),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
        sol[0].copy_(y0)
        self._rhs(th[0], y0, ops.Stage(f_out=b['K0']))
        dt = self._select_initial_step(th[0]) if self.first_step is None else float(self.first_step)
        self.steps = []           # accepted steps: t0, dt, y0, stage inputs, y1
        self.outputs = []         # (output index, 'exact', boundary index) | (output index, 'dense', step, coefs)
        y, t_cur = y0, th[0]
        for i_out in range(1, len(th)):
            next_t = th[i_out]
            while next_t > t_cur:
                check_step(t_cur, dt, self.n_steps, self.max_num_steps)
                X, y1, e2 = self._attempt(y, t_cur, dt)
                ratio = math.sqrt(float(e2) / y0.numel())  # the one host read of the step
                if ratio <= 1:
                    self.steps.append({'t0': t_cur, 'dt': dt, 'y0': y, 'yin': X, 'y1': y1})
                    t_cur = t_cur + dt
                    y = y1
                    rotate(b, P)  # the next f0: this step's last stage (FSAL or not); _attempt rebinds Y / Y1
                dt = next_dt(dt, ratio, self.order, self.safety, self.ifactor, self.dfactor)
                self.n_steps += 1
            if next_t == t_cur or not self.steps:
                sol[i_out].copy_(y)
                self.outputs.append((i_out, 'exact', len(self.steps)))
            else:
                # the k's of the last accepted step are in bufs (K0 / K_ns swapped back for the formula)
                rotate(b, P)
                coefs = self._interp_into(sol[i_out], self.steps[-1], next_t)
                rotate(b, P)
                self.outputs.append((i_out, 'dense', len(self.steps) - 1, coefs))
        self.func = None  # the backward reads the caller's snapshot, never the module
        return sol

    # ------------------------------------------------------------------ backward
    def backward(self, grad_sol, o, w):
        """The discrete adjoint of the accepted steps and the dense outputs.  ``o``: the
        LaplacianOperands taken in forward (snapshot mode); ``w``: the weights as autograd
        saved them."""
        P = self.plan
        ns, S = P.ns, len(self.steps)
        g, w_csc, alpha = o.g, o.w_csc, o.alpha
        R = self.y0.numel() // self.y0.shape[-1]
        drow = torch.zeros(R, dtype=torch.float64, device=self.y0.device)
        grad_sol = grad_sol.contiguous()
        z = torch.zeros_like(self.y0)

        def csc(x, stage):
            ops.spmm_rhs(g, w_csc, x, alpha=alpha, rhs=True, alpha_sigmoid=True, transpose=True, stage=stage)

        # output adjoints: per boundary (exact outputs) and per step (dense-output seeds)
        ybound = [None] * (S + 1)
        seeds = {}
        for ent in self.outputs:
            gs = grad_sol[ent[0]]
            if ent[1] == 'exact':
                n = ent[2]
                ybound[n] = gs.clone() if ybound[n] is None else ybound[n] + gs
            else:
                s, c = ent[2], ent[3]
                sd = seeds.setdefault(s, {'y0': None, 'y1': None, 'k': [None] * (ns + 1)})
                for key in ('y0', 'y1'):
                    sd[key] = c[key] * gs if sd[key] is None else sd[key] + c[key] * gs
                for j in range(ns + 1):
                    if c['k'][j] != 0.0:
                        sd['k'][j] = c['k'][j] * gs if sd['k'][j] is None else sd['k'][j] + c['k'][j] * gs
        pairs_k, pairs_y = [], []   # (kbar_{i+1}, Yin_i) of every stage: the weights' SDDMM
        ybar = ybound[S] if ybound[S] is not None else z.clone()
        fbar = None                 # the next step's kbar_0 = this step's f1 adjoint
        for s in range(S - 1, -1, -1):
            st = self.steps[s]
            dt, yin = st['dt'], st['yin']
            sd = seeds.get(s)
            ybar1 = ybar if sd is None or sd['y1'] is None else ybar + sd['y1']
            # kbar_ns: the f1 adjoint (+ dense seed; + dt c_sol[ns] ybar1 for the non-FSAL pairs)
            kb = [None] * (ns + 1)
            kns = fbar if fbar is not None else z.clone()
            if sd is not None and sd['k'][ns] is not None:
                kns = kns + sd['k'][ns]
            if not P.fsal and P.c_sol[ns] != 0.0:
                kns = kns + (dt * P.c_sol[ns]) * ybar1
            kb[ns] = kns
            ybin = [None] * ns
            y0bar = torch.empty_like(self.y0)
            for i in range(ns - 1, -1, -1):
                fsal_last = P.fsal and i == ns - 1
                # kbar_i = dt sum_{m >= i} beta[m][i] Yin_bar_m [+ dt c_sol[i] ybar1 non-FSAL]; Yin_bar_i = f [+ ybar1]
                terms = [(ybin[m], dt * P.beta[m][i]) for m in range(i + 1, ns) if P.beta[m][i] != 0.0]
                cf_i = dt * P.beta[i][i]
                if fsal_last:
                    terms.append((ybar1, cf_i))
                if not P.fsal and P.c_sol[i] != 0.0:
                    terms.append((ybar1, dt * P.c_sol[i]))
                kbi = torch.empty_like(self.y0)
                outs = [(kbi, None, 0.0, cf_i, terms)]
                if i > 0:
                    ybin[i] = torch.empty_like(self.y0)
                    outs.append((ybin[i], ybar1 if fsal_last else None, 1.0 if fsal_last else 0.0, 1.0, []))
                else:
                    # ybar_0 = sum_m Yin_bar_m [+ ybar1 non-FSAL]: Yin_bar_0 = f [+ ybar1 if ns == 1 and FSAL]
                    yterms = [(ybin[m], 1.0) for m in range(1, ns)]
                    if fsal_last or not P.fsal:
                        yterms.append((ybar1, 1.0))
                    outs.append((y0bar, None, 0.0, 1.0, yterms))
                stage = ops.Stage(outs=outs, dot=(yin[i], drow, 1.0, True))
                if len(stage._operands()) > 6:
                    raise RuntimeError("gnpde: adaptive backprop stage over 6 operands")
                csc(kb[i + 1], stage)
                pairs_k.append(kb[i + 1])
                pairs_y.append(yin[i])
                if sd is not None and sd['k'][i] is not None:
                    kbi = kbi + sd['k'][i]
                kb[i] = kbi
            if sd is not None and sd['y0'] is not None:
                y0bar = y0bar + sd['y0']
            if ybound[s] is not None:
                y0bar = y0bar + ybound[s]
            ybar, fbar = y0bar, kb[0]
        # the first step's k_0 = f(y0)
        y_init = self.y0
        if S > 0:
            out = torch.empty_like(self.y0)
            csc(fbar, ops.Stage(outs=[(out, ybar, 1.0, 1.0, [])], dot=(y_init, drow, 1.0, True)))
            pairs_k.append(fbar)
            pairs_y.append(y_init)
            ybar = out
        ybar = ybar + grad_sol[0]  # sol[0] = y0
        ga = alpha_grad(drow, alpha.double())
        gb = None
        if self.add_source and pairs_k:
            ksum = torch.stack(pairs_k, 0).sum(0)
            gb = ops.dot(ksum, o.x0)
        gw = None
        if w.requires_grad and pairs_k:
            C = self.y0.shape[-1]
            KB = torch.stack([k.reshape(R, C) for k in pairs_k], 1).reshape(self.y0.shape[:-1] + (-1,))
            YB = torch.stack([v.reshape(R, C) for v in pairs_y], 1).reshape(self.y0.shape[:-1] + (-1,))
            heads = w.shape[2] if w.dim() == 3 else 1
            gw = ops.sddmm(g, KB.contiguous(), YB.contiguous(), heads=heads, alpha=alpha,
                           alpha_sigmoid=True).view(w.shape)
        return ybar, ga, gb, gw
