"""The early-stop test integrator (src/early_stop_solver.py): ``EarlyStopInt``, what
``GNNEarly.__init__`` assigns to ``odeblock.test_integrator`` (src/GNN_early.py:24-33).

At test time the reference integrates over ``[0, earlystopxT * T]``, decodes the
state after every solver step with the model's output layer (``m2``), scores the
train / validation / test accuracies, and keeps those of the step with the best
validation accuracy and its time (``EarlyStopDopri5.advance`` :71-88,
``EarlyStopRK4.integrate`` :170-192).  Here the solve is gnpde.odeint's — the fused
adaptive step under the device controller, rk4 in replayed graphs — with one
added launch per scored state (gnpde_decode_score_f32, ops.decode_score), which
adds the three hit counts to slot k of a device record ``int32 [S, 3]``.  Nothing
is read between steps: the host reads the record once after the solve and forms
``best_*`` from it and the accepted step times it already holds.

Readings of the reference recorded here:

* ``evaluate`` / ``test`` index a 2-D weight with ``.shape[2]`` and call ``.max(2)``
  on a 2-D slice (:95, :114, :198, :214), so they cannot run in the reference
  fork.  The intended reading is implemented: the decoder's input width is
  ``Cd = m2_weight.shape[1]``; a wider state (``augment``) is scored on its first
  ``Cd`` columns; the prediction is the argmax over classes (the lowest class on a
  tie); a split's accuracy is its correct rows over its mask size, over all
  ``B * N`` masked rows (a per-node mask repeats over the batch elements).
* dopri5: the reference scores after every attempt, rejected ones included; a
  rejected attempt leaves ``rk_state.y1`` unchanged and the update is a strict
  ``>``, so scoring the accepted steps alone gives the same ``best_*``; that is what
  runs.  ``max_test_steps`` counts attempts, rejected ones included; when it is
  reached before the end time the solve returns the state at the last accepted
  ``t1`` (``y0`` when nothing was accepted) (:85-88).
* ``best_val`` and ``best_test`` start at 0 in every call (a new solver object per
  call, :309); ``best_train`` and ``best_time`` start at 0 here too (the reference
  leaves ``best_train`` undefined until the first improvement).
* The reference's callers run it under ``torch.no_grad()`` (run_GNN.py's ``test``);
  the solve here always does.
* The cross-entropy loss ``evaluate`` computes is used only by a commented-out
  print; it is not computed.

fp32 states only: a bf16 state raises NotImplementedError (the score kernel reads
fp32 rows).
"""
import torch

from . import ops
from .integrator import MULTISTEP_METHODS, _Combine, _host_grid, _host_times, odeint

SOLVERS = ('dopri5', 'rk4')


class EarlyStopSolver(object):
    """What ``EarlyStopInt.solver`` holds after a call: the reference solvers' result
    attributes (``best_train``, ``best_val``, ``best_test``, ``best_time``) and the per-step
    record they were formed from (``times``: the scored steps' t1; ``counts``: their
    [n, 3] correct-row counts; ``sizes``: the three mask sizes; ``preds``: the per-row
    predictions of every scored state when the integrator's ``record_pred`` is set)."""

    def __init__(self, method, opt):
        self.method, self.opt = method, opt
        self.max_test_steps = opt['max_test_steps']
        self.data = None
        self.m2_weight = None
        self.m2_bias = None
        self.best_train = 0
        self.best_val = 0
        self.best_test = 0
        self.best_time = 0
        self.times, self.counts, self.sizes, self.preds = [], None, None, None
        self.n_attempts, self.capped = 0, False

    def set_accs(self, train, val, test, time):
        self.best_train, self.best_val, self.best_test, self.best_time = train, val, test, float(time)

    def pick_best(self):
        """best_* from the record: the earliest step of the highest validation accuracy
        (strict >, from 0)."""
        acc = lambda c, n: (c / n) if n > 0 else 0.0  # noqa: E731
        for t1, (ctr, cva, cte) in zip(self.times, self.counts):
            val = acc(cva, self.sizes[1])
            if val > self.best_val:
                self.set_accs(acc(ctr, self.sizes[0]), val, acc(cte, self.sizes[2]), t1)


class EarlyStopInt(torch.nn.Module):
    """``EarlyStopInt(t, opt, device=None)``: a callable with torchdiffeq.odeint's
    signature that ignores the ``t`` and ``method`` it is passed (``self.t`` and
    ``opt['method']`` instead, as the reference), returns ``[2, *y0.shape]`` and leaves the
    result in ``self.solver``.  ``data``, ``m2_weight`` and ``m2_bias`` are assigned by the
    model (GNNEarly.set_solver_data / set_solver_m2).  ``scorer``: the function that scores
    a state, ops.decode_score's signature (default: it, the HIP kernel; the host tests
    inject ops.decode_score_torch)."""

    def __init__(self, t, opt, device=None, scorer=None):
        super(EarlyStopInt, self).__init__()
        if opt.get('beltrami', False) and opt.get('attention_type', 'scaled_dot') == 'exp_kernel' and \
                opt.get('gnpde_beltrami_kernel', False):
            raise NotImplementedError("gnpde.EarlyStopInt: the beltrami exp_kernel attention "
                                      "(gnpde_beltrami_kernel) is not covered by the early-stop integrator")
        self.device = device
        self.solver = None
        self.data = None
        self.max_test_steps = opt['max_test_steps']
        self.m2_weight = None
        self.m2_bias = None
        self.opt = opt
        self.t = torch.tensor([0, opt['earlystopxT'] * t], dtype=torch.float).to(self.device)
        self.scorer = scorer if scorer is not None else ops.decode_score
        self.record_pred = False  # tests / debugging: keep every scored state's predictions
        self._bufs = {}  # (slots, rows, device) -> (record, predictions or None): one allocation per shape

    def _record(self, S, R, dev):
        key = (S, R, str(dev), bool(self.record_pred))
        hit = self._bufs.get(key)
        if hit is None:
            if len(self._bufs) >= 4:
                self._bufs.clear()
            rec = torch.zeros((max(S, 1), 3), dtype=torch.int32, device=dev)
            preds = torch.empty((max(S, 1), R), dtype=torch.int32, device=dev) if self.record_pred else None
            hit = self._bufs[key] = (rec, preds)
        hit[0].zero_()
        return hit

    def __call__(self, func, y0, t, method=None, rtol=1e-7, atol=1e-9, adjoint_method="dopri5", adjoint_atol=1e-9,
                 adjoint_rtol=1e-7, options=None):
        method = self.opt['method']
        if method in MULTISTEP_METHODS:
            raise NotImplementedError("gnpde.EarlyStopInt: method %r: the early-stop integrator covers dopri5 and rk4 "
                                      "(as the reference), not the multistep solvers" % method)
        assert method in SOLVERS, "Only dopri5 and rk4 implemented with early stopping"
        if y0.dtype != torch.float32:
            raise NotImplementedError("gnpde.EarlyStopInt: %s state: the score kernel (gnpde_decode_score_f32) reads "
                                      "fp32 rows; early-stop solves of bf16 states are out of scope" % y0.dtype)
        options = dict(options or {})
        solver = EarlyStopSolver(method, self.opt)
        solver.data, solver.m2_weight, solver.m2_bias = self.data, self.m2_weight, self.m2_bias
        self.solver = solver
        dev = y0.device
        R = y0.numel() // y0.shape[-1]
        W = self.m2_weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        b = None if self.m2_bias is None else self.m2_bias.detach().to(device=dev, dtype=torch.float32).contiguous()
        if W.dim() != 2 or W.shape[1] > y0.shape[-1]:
            raise ValueError("gnpde.EarlyStopInt: m2_weight %s does not decode a state of width %d"
                             % (tuple(W.shape), y0.shape[-1]))
        split, label, solver.sizes = ops.pack_splits(self.data, R, dev)
        tt = self.t if self.t.device == dev else self.t.to(dev)
        if method == 'rk4':
            S = len(_host_grid(_host_times(tt), tt.dtype, options.get('step_size'))) - 1
        else:
            S = int(self.max_test_steps)
            options['gnpde_max_attempts'] = S
        rec, preds = self._record(S, R, dev)
        times = solver.times

        def hook(y, t1, lay):
            k = len(times)
            times.append(float(t1))
            self.scorer(y, W, b, split, label, rec[k], ld=y.shape[-1], rows=lay.order32 if lay is not None else None,
                        pred_out=preds[k] if preds is not None else None)

        options['gnpde_accept_hook'] = hook
        with torch.no_grad():
            # (a CPU state: the host tests' injected RHS and scorer; the product path is the device's)
            sol = odeint(func, y0, tt, rtol=rtol, atol=atol, method=method, options=options,
                         combine=None if y0.is_cuda else _Combine())
        n = len(times)
        if method != 'rk4':
            solver.n_attempts, solver.capped = odeint.last_n_steps, odeint.last_capped
        solver.counts = rec[:n].tolist()  # the one host read of the scores
        if preds is not None:
            solver.preds = preds[:n].clone()
        solver.pick_best()
        return sol
