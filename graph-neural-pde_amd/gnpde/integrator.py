"""Bundled ODE integrator with torchdiffeq's calling convention.

The reference integrates with ``torchdiffeq.odeint`` (src/block_constant.py:46-51,
src/block_transformer_attention.py:40-52); torchdiffeq (README.md:29 pins 0.2.1,
requirements.txt:20 0.1.1) is not installed in this image, so the solver loop
is restated here from its published algorithm (torchdiffeq 0.2.x):

* fixed grid (``euler``, ``midpoint``, ``rk4``): ``FixedGridODESolver`` with
  ``_grid_constructor_from_step_size`` (niters = ceil((t1-t0)/h + 1), the last
  grid point snapped to t1) and linear interpolation onto the requested times;
  rk4 is ``rk4_alt_step_func`` (the 3/8 rule);
* ``dopri5``, ``bosh3``, ``fehlberg2``, ``adaptive_heun``:
  ``RKAdaptiveStepsizeODESolver`` with the solver's embedded tableau,
  ``_select_initial_step``, the RMS error norm, the safety 0.9 / ifactor 10 /
  dfactor 0.2 controller and 4th-order dense output (``_interp_fit`` with the
  solver's mid-point coefficients) at the requested times.  adaptive_heun is the
  reference's default ``adjoint_method`` (src/run_GNN.py:334).

Stage combinations ``y0 + dt * sum_j b_j k_j`` are single fused HIP passes
(gnpde_rk_combine_f32).  The RHS calls are whatever ``func`` is (the gnpde
ODEFuncs run entirely in HIP).  Parity of integrated values is UNPINNED: the
reference's tests only check shapes.
"""
import collections
import itertools
import math
import os
import warnings
import weakref

import numpy as np
import torch

from . import _lib, adams_coefficients, ops
from ._cache import _tensor_key
from .adaptive_backprop import AdaptiveBackprop
from .adjoint_adaptive import AdaptiveAdjoint
from .solver_common import (_TABLEAUS, _AdaptivePlan, _AdaptiveState, _KrylovPlan, _adaptive_plan,  # noqa: F401
                            _entry_copy, _krylov_plan, _node_layout, _to_internal, _to_user, alpha_grad, check_step,
                            dense_combo, dense_weights, laplacian_adjoint_ok, laplacian_operands, next_dt,
                            param_grads, rotate)
from .utils import MaxNFEException

FIXED_METHODS = ('euler', 'midpoint', 'rk4')
ADAPTIVE_METHODS = ('dopri5', 'bosh3', 'fehlberg2', 'adaptive_heun')
# torchdiffeq's multistep solvers (fixed_adams.AdamsBashforthMoulton), opt-in: taken only with
# options['gnpde_adams'] true (adjoint_options['gnpde_adams'] for the adjoint solve)
MULTISTEP_METHODS = ('explicit_adams', 'implicit_adams')


class _CombineFn(torch.autograd.Function):
    """The fused HIP stage combination under autograd: forward one streaming pass
    (gnpde_rk_combine_f32) instead of a clone plus a multiply and an add per
    term; backward d/dy0 = g, d/dk_j = scale * c_j * g."""

    @staticmethod
    def forward(ctx, y0, scale, coefs, *ks):
        ctx.scale, ctx.coefs, ctx.has_y0 = scale, coefs, y0 is not None
        return ops.rk_combine(y0, list(ks), list(coefs), scale).view(ks[0].shape)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gk = [g * float(ctx.scale * c) for c in ctx.coefs]
        return (g if ctx.has_y0 else None, None, None) + tuple(gk)


class _Combine(object):
    """y0 + scale * sum_j c_j k_j on the device (fused HIP pass).  When autograd
    has to see the combination (grad enabled and an operand requires grad) it
    runs through _CombineFn so gradients flow through the solver (torch ops for
    CPU tensors: the host-logic tests' injected RHS)."""

    def __call__(self, y0, ks, coefs, scale):
        if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in [y0] + list(ks)):
            if ks[0].is_cuda and ks[0].dtype == torch.float32:
                return _CombineFn.apply(y0, float(scale), tuple(float(c) for c in coefs), *ks)
            return _torch_combine(y0, ks, coefs, scale)
        if ks[0].dtype == torch.bfloat16:
            # bf16 state outside the fused paths: the stage pass (gnpde_stage_apply_bf16: fp32
            # arithmetic, one rounding to bf16 per output) — VERDICT r3 weak 7
            nz = [(k, c) for k, c in zip(ks, coefs) if c != 0]  # the tableaus' zero entries (dopri5 b2)
            ops_ok = ks[0].is_cuda and 0 < len(nz) <= _lib.STAGE_MAX_K and all(
                k.is_contiguous() and k.shape == ks[0].shape for k in ks) and (
                y0 is None or (y0.is_contiguous() and y0.shape == ks[0].shape and y0.dtype == ks[0].dtype))
            if ops_ok:
                out = torch.empty_like(ks[0])
                ops.stage_apply(ops.Stage(outs=[(out, y0, 1.0, 0.0, [(k, float(scale * c)) for k, c in nz])]),
                                None, None, out)
                return out
            acc = _torch_combine(None if y0 is None else y0.float(), [k.float() for k in ks], coefs, scale)
            return acc.to(torch.bfloat16)
        return ops.rk_combine(y0, ks, coefs, scale).view(ks[0].shape)


def _torch_combine(y0, ks, coefs, scale):
    """Host-logic testing aid only (tests inject it for CPU oracle funcs)."""
    acc = torch.zeros_like(ks[0]) if y0 is None else y0.clone()
    for k, c in zip(ks, coefs):
        acc = acc + (scale * c) * k
    return acc


def _rms_norm(t):
    return t.abs().pow(2).mean().sqrt()


def fixed_grid(t, step_size):
    """torchdiffeq ``_grid_constructor_from_step_size`` (dtype of t)."""
    start_time, end_time = t[0], t[-1]
    niters = torch.ceil((end_time - start_time) / step_size + 1).item()
    t_infer = torch.arange(0, niters, dtype=t.dtype, device=t.device) * step_size + start_time
    t_infer[-1] = t[-1]
    return t_infer


def _linear_interp(t0, t1, y0, y1, t):
    if t == t0:
        return y0
    if t == t1:
        return y1
    slope = (t - t0) / (t1 - t0)
    return y0 + slope * (y1 - y0)


def _fixed_step(method, func, t0, dt, t1, y0, combine):
    """Returns y1 = y0 + dy (one grid step)."""
    if method == 'euler':
        f0 = func(t0, y0)
        return combine(y0, [f0], [1.0], dt)
    if method == 'midpoint':
        f0 = func(t0, y0)
        y_mid = combine(y0, [f0], [0.5], dt)
        f_mid = func(t0 + 0.5 * dt, y_mid)
        return combine(y0, [f_mid], [1.0], dt)
    if method == 'rk4':  # rk4_alt_step_func (3/8 rule)
        k1 = func(t0, y0)
        k2 = func(t0 + dt / 3.0, combine(y0, [k1], [1.0 / 3.0], dt))
        k3 = func(t0 + dt * 2.0 / 3.0, combine(y0, [k1, k2], [-1.0 / 3.0, 1.0], dt))
        k4 = func(t1, combine(y0, [k1, k2, k3], [1.0, -1.0, 1.0], dt))
        return combine(y0, [k1, k2, k3, k4], [0.125, 0.375, 0.375, 0.125], dt)
    raise ValueError(method)


def _fusable(func, y0, combine):
    """The RHS can emit the stage combinations itself (gnpde ODEFuncs, no autograd).
    A host-side RHS object with ``host_stages`` (tests/dist_workers.py: the gloo
    tests of gnpde.dist) takes the same path on CPU tensors."""
    if not (isinstance(combine, _Combine) and hasattr(func, 'rhs_stage')) or torch.is_grad_enabled():
        return False
    return y0.dtype in ops.STATE_DTYPES if y0.is_cuda else bool(getattr(func, 'host_stages', False))


RHS_PER_STEP = {'euler': 1, 'midpoint': 2, 'rk4': 4}


def _fused_step(method, func, t0, dt, t1, y0, ws, out=None, out_rows=None, inplace=False, frozen=None):
    """One grid step with the stage combinations fused into the RHS epilogues
    (gnpde_stage_epilogue_t): same arithmetic as _fixed_step, ~7 fewer passes
    over the state per rk4 step and no separate combine launches.  ``out``:
    the buffer that receives y1 (default: a new tensor); ``out_rows`` (int32
    [R]): y1's row r is stored at row out_rows[r] of ``out`` (the last step of
    a solve run in a node renumbering writes the caller's numbering).
    ``inplace`` (rk4): the step in three live buffers — y1 overwrites y0 when no
    ``out`` is given, and y0 is left alone otherwise; the same bits either way.
    ``frozen`` (the in-place rk4 step, _frozen_rows): (ops.FrozenRows, None) leaves the
    graph's frozen rows out of the step; (ops.FrozenRows, n), the solve's last step, also
    takes them from y0 through the solve's n steps at once; the same bits again."""
    y0 = y0.contiguous()
    if method == 'euler':
        y1 = torch.empty_like(y0) if out is None else out
        func.rhs_stage(t0, y0, ops.Stage(outs=[(y1, y0, 1.0, dt, [])], out_rows=out_rows))
        return y1
    if method == 'midpoint':
        ym = ws.get('a', y0)
        y1 = torch.empty_like(y0) if out is None else out
        func.rhs_stage(t0, y0, ops.Stage(outs=[(ym, y0, 1.0, 0.5 * dt, [])]))
        func.rhs_stage(t0 + 0.5 * dt, ym, ops.Stage(outs=[(y1, y0, 1.0, dt, [])], out_rows=out_rows))
        return y1
    if method == 'rk4':
        # rk4_alt_step_func (3/8 rule).  With x2 = y + dt k1/3 the stage inputs
        # and the result are affine in rows the epilogue already holds (its own
        # input row comes for free), so no k_i is ever stored:
        #   x3 = y + dt (k2 - k1/3)      = 2 y  - x2 + dt k2
        #   x4 = y + dt (k1 - k2 + k3)   = 2 x2 - x3 + dt k3
        #   y1 = y + dt/8 (k1 + 3k2 + 3k3 + k4) = (6 x3 + 3 x4 - y + dt k4) / 8
        # 8 state passes per step besides the gathers (one write per stage,
        # reads of y, x2, y + x3), where storing k's and an accumulator takes 15.
        if inplace:
            # The step never needs more than three live buffers (y, a, b: 260 MB on G-arxiv
            # against 433 MB for five, beside a 256 MiB Infinity Cache): x4 is written over x2
            # and y1 over y — each read only as the own-row operand of the row being written,
            # by the lane that writes it, before its store (ops.Stage: an output may alias an
            # operand).  Same combinations, same operand order: the same bits.
            a, b = ws.get('a', y0), ws.get('b', y0)
            y1 = y0 if out is None else out
            # Frozen rows (f = 0, gathered by no other row): their x2, x3, x4 equal y bit for bit,
            # y1 depends on nothing but y, and nothing reads them before the solve's end.  Every
            # launch leaves them out (their rows of y, a and b stay as they are) but the last of
            # the solve, which takes them from y0 through all its ``steps`` steps in registers
            # and stores them through out_rows.
            fr, fsteps = frozen if frozen is not None else (None, None)
            skip = {} if fr is None else {'frozen': (fr, None, 0)}
            last = skip if fsteps is None else {'frozen': (fr, y0, fsteps)}
            func.rhs_stage(t0, y0, ops.Stage(outs=[(a, y0, 1.0, dt / 3.0, [])]), **skip)
            func.rhs_stage(t0 + dt / 3.0, a, ops.Stage(outs=[(b, a, -1.0, dt, [(y0, 2.0)])]), **skip)
            func.rhs_stage(t0 + dt * 2.0 / 3.0, b, ops.Stage(outs=[(a, b, -1.0, dt, [(a, 2.0)])]), **skip)
            func.rhs_stage(t1, a, ops.Stage(outs=[(y1, a, 0.375, dt * 0.125, [(b, 0.75), (y0, -0.125)])],
                                            out_rows=out_rows), **last)
            return y1
        if frozen is not None:
            raise ValueError("frozen rows are left out of the in-place rk4 step only")
        x2, x3, x4 = ws.get('a', y0), ws.get('b', y0), ws.get('c', y0)
        y1 = torch.empty_like(y0) if out is None else out
        func.rhs_stage(t0, y0, ops.Stage(outs=[(x2, y0, 1.0, dt / 3.0, [])]))
        func.rhs_stage(t0 + dt / 3.0, x2, ops.Stage(outs=[(x3, x2, -1.0, dt, [(y0, 2.0)])]))
        func.rhs_stage(t0 + dt * 2.0 / 3.0, x3, ops.Stage(outs=[(x4, x3, -1.0, dt, [(x2, 2.0)])]))
        func.rhs_stage(t1, x4, ops.Stage(outs=[(y1, x4, 0.375, dt * 0.125, [(x3, 0.75), (y0, -0.125)])],
                                         out_rows=out_rows))
        return y1
    raise ValueError(method)


class _Workspace(dict):
    """Stage-input buffers of the fused steps.  A RHS object may place the state
    itself (``alloc_state(like)``: dist.RowShardedLaplacian hands out row blocks of
    its gathered buffers, so the all-gather before each RHS is in place)."""

    def __init__(self, alloc=None):
        dict.__init__(self)
        self.alloc = alloc

    def get(self, name, like):
        t = dict.get(self, name)
        if t is None or t.shape != like.shape or t.device != like.device:
            t = _new_state(like, self.alloc)
            self[name] = t
        return t


def _new_state(like, alloc=None):
    return alloc(like) if alloc is not None else torch.empty_like(like, memory_format=torch.contiguous_format)


# Graph replay of fixed-grid steps (hipGraph through torch.cuda.CUDAGraph): a run
# of k equal steps is replayed as the binary decomposition of k into captured
# blocks of 2^i steps (at most GRAPH_BLOCK each), so a solve costs a handful of
# graph launches whatever its length (each launch leaves the GPU idle ~18 us
# between replays: profiles/r03a trace).  Capture itself costs host time, so a
# solve shorter than GRAPH_MIN_STEPS runs eagerly.
GRAPH_MIN_STEPS = 6
# Largest block graph, in steps (a power of two; GNPDE_GRAPH_BLOCK overrides).
GRAPH_BLOCK = int(os.environ.get('GNPDE_GRAPH_BLOCK', '64'))
# Set to a list to receive (start_event, end_event, n_rhs) per graph replay
# (bench.py's per-launch roofline timing); None in normal use.
replay_events = None
# The no-grad fixed-grid rk4 solve keeps its state in one buffer and steps in place
# (_fused_step(inplace=True): three live buffers instead of five) for modules that do not
# place their own state (alloc_state: the row-sharded classes keep the ping-pong scheme).
# GNPDE_RK4_INPLACE=0 keeps the ping-pong scheme everywhere; results do not depend on it.
RK4_INPLACE = os.environ.get('GNPDE_RK4_INPLACE', '1') != '0'


def _steps_inplace(method, func, y):
    return RK4_INPLACE and method == 'rk4' and y.is_cuda and getattr(func, 'alloc_state', None) is None


# A graph's frozen rows — one edge, their own self loop of weight exactly 1.0, gathered by no
# other row: f = 0, and a step changes the row by the rounding of its last combination alone —
# are left out of every launch of an in-place rk4 solve with a single output time but the
# solve's last, which takes them through all the steps at once and stores them in the caller's
# numbering (ops.FrozenRows): nothing reads the state's frozen rows in
# between.  Results do not depend on it.  GNPDE_FROZEN_ROWS=0 runs every row through every launch.
FROZEN_ROWS = os.environ.get('GNPDE_FROZEN_ROWS', '1') != '0'
# how many solves left frozen rows out (tests assert the path was taken, not silently dropped)
frozen_stats = {'solves': 0}


def _frozen_rows(func, method, y, inplace, t_h, step_hook):
    """The ops.FrozenRows this solve leaves out of its launches, or None.  Called with the
    solve's NodeLayout active and outside any capture (the module may read the host once)."""
    fn = getattr(func, 'frozen_rows', None)
    if not (FROZEN_ROWS and fn is not None and inplace and method == 'rk4' and len(t_h) == 2 and step_hook is None):
        return None
    return fn(y)


def _pow2_blocks(k, cap):
    """k as a sum of powers of two <= cap, largest first (odd sizes last)."""
    out = []
    b = 1
    while b * 2 <= max(cap, 1):
        b *= 2
    while k > 0:
        while b > k:
            b //= 2
        out.append(b)
        k -= b
    return out


class _StatePool(object):
    """The two ping-pong state buffers and the stage-input workspace of a
    module's fused fixed-grid solves of one state shape (kept across calls, so
    the captured graphs that read them stay valid and a solve needs no
    allocation)."""

    def __init__(self, like, alloc=None):
        self.bufs = [_new_state(like, alloc) for _ in range(2)]
        self.ws = _Workspace(alloc)


_POOLS = weakref.WeakKeyDictionary()  # module -> {(shape, dtype, device): _StatePool}


def _state_pool(func, y):
    # keyed by stream too: two concurrent solves of one module on two streams
    # must not share ping-pong buffers or stage workspaces
    sid = torch.cuda.current_stream(y.device).cuda_stream if y.is_cuda else None
    key = (tuple(y.shape), y.dtype, str(y.device), sid)
    d = _POOLS.get(func)
    if d is None:
        d = {}
        _POOLS[func] = d
    pool = d.get(key)
    if pool is None:
        if len(d) >= 4:
            d.clear()
        pool = _StatePool(y, getattr(func, 'alloc_state', None))
        d[key] = pool
    return pool


class _StepGraphs(object):
    """Captured blocks of fixed-dt grid steps over a _StatePool: graph (s, p)
    runs s steps starting from bufs[p] (ping-ponging, so it ends in bufs[p ^ (s & 1)];
    ``inplace``: in bufs[p] itself); captured on first use.  The launches are those of the eager fused step (same
    kernels, same arguments, same bits).  ``warm`` is False until one eager step
    of this entry has run: every per-graph structure (CSR, plans, cached weights,
    scratch) is built by an eager call before anything is captured, so nothing
    synchronises inside a capture."""

    def __init__(self, method, func, dt, pool, inplace=False, frozen=None):
        self.method, self.dt, self.pool, self.inplace = method, dt, pool, inplace
        self.frozen = frozen  # the ops.FrozenRows the captured steps leave out, or None
        self.n_rhs = RHS_PER_STEP[method]
        self.graphs = {}
        self.mempool = None
        self.warm = False

    def graph(self, func, s, p):
        g = self.graphs.get((s, p))
        if g is None:
            nfe = getattr(func, 'nfe', None)
            bufs, ws = self.pool.bufs, self.pool.ws
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.mempool):
                for k in range(s):
                    if self.inplace:
                        _fused_step(self.method, func, 0.0, self.dt, self.dt, bufs[p], ws, inplace=True,
                                    frozen=(self.frozen, None) if self.frozen is not None else None)
                        continue
                    i = p ^ (k & 1)
                    _fused_step(self.method, func, 0.0, self.dt, self.dt, bufs[i], ws, out=bufs[1 - i])
            if self.mempool is None:
                self.mempool = g.pool()
            if nfe is not None:
                func.nfe = nfe  # capture records launches, it evaluates nothing
            self.graphs[(s, p)] = g
        return g

    def end(self, s, p):
        """The parity the state is in after s steps from bufs[p]."""
        return p if self.inplace else p ^ (s & 1)

    def replay(self, func, s, p):
        """Replay s steps from bufs[p]; counts the RHS evaluations like the eager
        calls; returns the parity the state ends in."""
        g = self.graph(func, s, p)
        if hasattr(func, 'nfe'):
            func.nfe += s * self.n_rhs
        if replay_events is not None:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            g.replay()
            ev1.record()
            replay_events.append((ev0, ev1, s * self.n_rhs))
        else:
            g.replay()
        return self.end(s, p)


# Captured step graphs kept per RHS module between odeint calls (one entry per
# module, replaced when its key changes), so repeated solves — every forward
# of a GRAND model in eval — replay without re-capturing.  A weak key: the
# entry goes with the module.
_GRAPH_CACHE = weakref.WeakKeyDictionary()


def _capture_state(func, y):
    """The derived device objects a captured step reads (device CSR and plans,
    CSR-order weights, the stable x0 buffer, cached projection weights ...),
    refreshed in place from the module's current tensors by
    ``func.graph_capture_state(y)``; None when the module offers no such hook
    (its graphs are then captured per call and never cached)."""
    fn = getattr(func, 'graph_capture_state', None)
    return None if fn is None else tuple(fn(y))


def _graph_cache_key(func, method, y, state):
    """Everything a captured step reads besides its own buffers: the module's
    parameters and buffers (identity + version: in-place updates recapture,
    host-read scalars such as exp_kernel's lengthscale are baked into the
    launches), its options, the state's shape and layout, and the IDENTITY of
    every derived object in ``state``.  The cache entry holds ``state``
    itself, so the buffers a replay reads stay alive however the module
    rebuilds its own caches (a solve on another graph replaces func._graph;
    the replayed step then finds a different object and recaptures instead of
    reading freed memory).  Source tensors (edge_index, edge_weight,
    attention_weights, x0) are NOT in the key: what the launches read is the
    derived buffers, refreshed in place when only the values change."""
    if state is None:
        return None
    if hasattr(func, 'parameters'):
        tens = [_tensor_key(t) for t in itertools.chain(func.parameters(), func.buffers())]
    else:  # a plain RHS object (gnpde.dist shards): the scalars it reads by pointer
        tens = [_tensor_key(t) for t in getattr(func, 'capture_key_tensors', lambda: ())()]
    opt = getattr(func, 'opt', None)
    okey = _opt_key(opt) if isinstance(opt, dict) else None
    return (method, tuple(y.shape), tuple(y.stride()), y.dtype, str(y.device), okey, tuple(tens),
            tuple(id(o) for o in state))


_OPT_KEYS = {}  # id(opt dict) -> (its items when keyed, key string)


def _opt_key(opt):
    """The options part of a graph cache key: the sorted repr of the dict, recomputed only
    when its items changed (an in-place edit of the module's opt changes them)."""
    items = tuple(opt.items())
    hit = _OPT_KEYS.get(id(opt))
    try:
        if hit is not None and hit[0] == items:
            return hit[1]
    except (TypeError, ValueError):  # values without a plain equality (arrays): no cache
        return repr(sorted(opt.items(), key=lambda kv: str(kv[0])))
    key = repr(sorted(opt.items(), key=lambda kv: str(kv[0])))
    if len(_OPT_KEYS) > 256:
        _OPT_KEYS.clear()
    _OPT_KEYS[id(opt)] = (items, key)
    return key


def _replayable(func):
    """Steps of ``func`` may be captured and replayed as hipGraphs: no collective per RHS
    (graph_capturable) and f(t, x) independent of t (autonomous) — a replay passes the
    stage times recorded at capture."""
    return getattr(func, 'graph_capturable', True) and getattr(func, 'autonomous', False)


def _nfe_headroom(func, n):
    """True when n more RHS calls cannot trip the MaxNFEException guard (the
    eager path raises at the exact call, as the reference does)."""
    opt = getattr(func, 'opt', None)
    if not hasattr(func, 'nfe') or not isinstance(opt, dict) or 'max_nfe' not in opt:
        return True
    return func.nfe + n - 1 <= opt['max_nfe']


# Experiment knob: byte multiple bf16 rows are padded to (default 16).  Whole
# 128-byte lines for BLEND's bf16 rows (162 -> 192 columns instead of 168) measured
# 0.391 against 0.315 ms per rk4 step: the wider row leaves the three-rows-per-
# wavefront geometry (tools/pad_ab.sh).
PAD_ALIGN_BF16 = int(os.environ.get('GNPDE_PAD_ALIGN_BF16', '16'))


def _padded_width(func, y0):
    """Feature width the fused path pads the state to, or None.  Rows whose byte
    length is not a multiple of 16 (C = 162 in fp32 or bf16, BLEND) cannot take
    16-byte vector gathers; a RHS whose arithmetic is column-independent
    (func.supports_feature_padding) integrates a zero-padded copy instead — the
    padding columns stay exactly 0 (A 0 - 0 = 0) — and the result is cut back."""
    per16 = 16 // y0.element_size()
    C = y0.shape[-1]
    if C % per16 == 0 or y0.dim() != 3:
        return None
    ok = getattr(func, 'supports_feature_padding', None)
    if ok is None or not ok():
        return None
    align = max(16, PAD_ALIGN_BF16 if y0.element_size() == 2 else 16) // y0.element_size()
    return (C + align - 1) // align * align


# --------------------------------------------------------------------------- training path
# Fixed-grid solves of the (linear) Laplacian RHS under autograd: the discrete
# adjoint of the whole solve as ONE autograd node.  GNPDE_FUSED_BACKWARD=0 falls
# back to autograd through every RHS and stage combination.
FUSED_BACKWARD = os.environ.get('GNPDE_FUSED_BACKWARD', '1') != '0'


def _fused_backward_ok(func, y0, combine, grid_h, t_h):
    if not (FUSED_BACKWARD and torch.is_grad_enabled() and isinstance(combine, _Combine) and y0.is_cuda and
            y0.dtype == torch.float32 and y0.dim() == 3):
        return False
    fn = getattr(func, 'fixed_grid_backward_ok', None)
    if fn is None or not fn():
        return False
    params = [y0, func.alpha_train, func.beta_train]
    if not any(p.requires_grad for p in params):
        return False
    gs = set(grid_h)
    return all(v in gs for v in t_h)  # every output time is a grid point (no interpolation)


class _LaplacianFixedGridFn(torch.autograd.Function):
    """The discrete adjoint of a fixed-grid solve (euler, midpoint, rk4 3/8) of
    f(x) = a (A x - x) [+ b x0], a = sigma(alpha_train) (or alpha_train),
    b = beta_train: exactly the gradient of the stepped computation, like
    backprop through every RHS call, but formed with the fused kernels.

    Forward: the fused steps (stage combinations in the K1 epilogues), the state
    at every step start and the stage inputs kept (3 states per rk4 step).
    Backward, step by step from the last, for rk4
        gk4 = dt/8 g              u4 = (A^T - I) gk4
        gk3 = 3dt/8 g + dt a u4   u3 = (A^T - I) gk3
        gk2 = 3dt/8 g - dt a u4 + dt a u3                       ...
        gk1 = dt/8 g + dt a u4 - dt/3 a u3 + dt/3 a u2
        g  <- g + a (u4 + u3 + u2 + u1)
    (formed as gk2 = gk3 + dt a u3 - 2 dt a u4, gk1 = gk2/3 + dt a (u2 + 4 u4 - 2 u3)/3
    and a running sum that carries g, so that each launch reads as few rows as it can)
        d alpha += a'(alpha) sum_i <u_i, x_i>,  d beta += sum_i <gk_i, x0>
    (K1 over the CSC for (A^T - I), each gk line and the running sum formed in
    the epilogue of the launch before it (gnpde_stage_epilogue_t), and the
    d alpha terms <u_i, x_i> added per row in fp64 by the same epilogues
    (dot_rows), summed once at the end): four transpose launches per rk4 step
    instead of autograd's ~40 elementwise kernels and a second K1 per RHS for
    d alpha."""

    @staticmethod
    def forward(ctx, y0, alpha_train, beta_train, func, method, steps, t_h):
        # everything the backward reads is taken NOW: a second forward with
        # another graph, x0 or alpha before this backward must not change its gradient.
        # The solve and its adjoint run in the graph's in-degree numbering when the module
        # offers one (as the no-grad solves, ops.NodeLayout); the solution and the input
        # gradient are in the caller's numbering.
        lay = _node_layout(func, y0)
        y0d = y0.detach().contiguous()
        sol = torch.empty((len(t_h),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
        if lay is not None:  # sol[0] = y0 and the solve's copy in one pass
            y = torch.empty_like(y0d)
            _entry_copy(y0d, y, sol[0], lay.order)
            func._layout = lay
        else:
            sol[0].copy_(y0d)
            y = y0d
        try:
            starts, stage_inputs = [], []
            j = 1
            for n_step, (ta, tb) in enumerate(steps):
                starts.append(y)
                ws = _Workspace()  # a fresh one per step: its stage inputs are kept for the backward
                if n_step == len(steps) - 1 and j == len(t_h) - 1 and t_h[j] == tb:
                    # the last step writes the result in the caller's numbering (no exit pass;
                    # the backward never reads the last step's output)
                    _fused_step(method, func, ta, tb - ta, tb, y, ws, out=sol[j],
                                out_rows=lay.order32 if lay is not None else None)
                    stage_inputs.append([ws[k] for k in ('a', 'b', 'c') if k in ws])
                    j += 1
                    break
                y = _fused_step(method, func, ta, tb - ta, tb, y, ws)
                stage_inputs.append([ws[k] for k in ('a', 'b', 'c') if k in ws])
                while j < len(t_h) and tb >= t_h[j]:
                    _to_user(y, sol[j], lay)
                    j += 1
            # The backward's own copies, taken after the forward launches are queued (the GPU
            # starts on the solve while the host does this; still before this call returns):
            # alpha (rk4's adjoint scales its a-dependent coefficients by a on the device, the
            # stage epilogue's coef_scale; the other methods' combinations need a on the host,
            # copied behind an event so the backward does not drain the queue to read it), and a
            # private CSC-order copy of the weights (grad mode is off inside a
            # Function's forward, so the module's cached buffer counts as no_grad-made and a
            # later no_grad call with new weights would refresh it in place under this node's
            # pending backward).
            ctx.o = o = laplacian_operands(func, y0, private_csc=True, snapshot=True)
            ctx.a_dev = torch.sigmoid(o.alpha) if o.sig else o.alpha
            ctx.a_scale = ctx.a_dev.reshape(()).float().contiguous()
            ctx.a_host = _host_scalar(ctx.a_dev) if method != 'rk4' else None
        finally:
            func._layout = None
        ctx.func, ctx.method, ctx.steps, ctx.t_h, ctx.lay = func, method, steps, t_h, lay
        ctx.starts, ctx.stage_inputs = starts, stage_inputs
        return sol

    @staticmethod
    def backward(ctx, g_sol):
        func, method, steps, t_h = ctx.func, ctx.method, ctx.steps, ctx.t_h
        g_sol = g_sol.contiguous()
        lay = ctx.lay
        with torch.no_grad():
            gr, w_csc, sig, add_source, x0 = ctx.o.g, ctx.o.w_csc, ctx.o.sig, ctx.o.add_source, ctx.o.x0
            one = _device_one(g_sol.device)
            a_dev = ctx.a_dev
            a = ctx.a_host() if ctx.a_host is not None else None  # euler / midpoint combinations
            asc = ctx.a_scale  # rk4: coef_scale of every adjoint launch (cb unscaled, cf and c_j times a)

            def u_of(v):  # (A^T - I) v
                return ops.spmm_rhs(gr, w_csc, v, alpha=one, rhs=True, alpha_sigmoid=False, transpose=True)

            comb = ops.rk_combine
            # the output-time gradients join the running gradient at their grid points
            out_at = {}
            j = 1
            for n, (ta, tb) in enumerate(steps):
                while j < len(t_h) and tb >= t_h[j]:
                    out_at.setdefault(n, []).append(j)
                    j += 1
            s0 = ctx.starts[0]
            g = None  # the running gradient (None: still zero)
            nfe = getattr(func, 'nfe', None)
            # d alpha, d beta and (rk4) the alpha gradient's per-row terms <u_i, x_i>, which
            # accumulate in the transpose launches' epilogues (gnpde_stage_epilogue_t dot_rows)
            # and are summed once at the end: one zero-filled fp64 buffer for the three
            n_drow = s0.numel() // s0.shape[-1] if method == 'rk4' else 0
            acc64 = torch.zeros(2 + n_drow, dtype=torch.float64, device=s0.device)
            ga, gb = acc64[0], acc64[1]
            drow = acc64[2:] if method == 'rk4' else None
            # rk4 in a renumbered solve: the first step's last launch stores the input gradient
            # straight into the caller's numbering (its out_rows), as the forward's last step
            # stores the solution — no exit pass
            user_rows = lay.order32 if (lay is not None and method == 'rk4' and not out_at.get(-1)) else None
            def g_at(jj):  # an output time's gradient in the solve's numbering (one gnpde_rows_copy pass)
                if lay is None:
                    return g_sol[jj]
                return _to_internal(g_sol[jj], lay)

            for n in range(len(steps) - 1, -1, -1):
                for jj in out_at.get(n, []):
                    g = g_at(jj) if g is None else g + g_at(jj)
                if g is None:
                    g = torch.zeros_like(s0)
                ta, tb = steps[n]
                dt = tb - ta
                y = ctx.starts[n]
                if method == 'rk4':
                    # the adjoint stage combinations ride in the transpose launches' epilogues
                    # (v = (A^T - I) g, so u4 = dt/8 v by linearity)
                    x2, x3, x4 = ctx.stage_inputs[n]
                    e = lambda: torch.empty_like(g)  # noqa: E731
                    v, gk3, u3, gk2, gk1, acc, g_new = (e() for _ in range(7))
                    c8 = dt / 8.0
                    T = dict(alpha=one, rhs=True, alpha_sigmoid=False, transpose=True)
                    # d alpha += a'(alpha) (dt/8 <v, x4> + <u3, x3> + <u2, x2> + <u1, y>): the epilogue of
                    # each launch adds its row terms; u2 and u1 are used only inside their own launch
                    # Each gk line is written against the launch's own input where it can (that row is
                    # in registers already): gk2 = gk3 + ad u3 - 2 ad c8 v, gk1 = gk2/3 + ad/3 u2 +
                    # 4/3 ad c8 v - 2/3 ad u3, and the running sum carries g (acc = g + a(c8 v + u3 + u2)),
                    # so g is read by the third launch only: 20 state passes per step, not 23
                    # (coefficients written without a: the epilogue multiplies cf and every c_j by *asc)
                    ops.spmm_rhs(gr, w_csc, g, stage=ops.Stage(f_out=v, outs=[(gk3, g, 3 * c8, dt * c8, [])],
                                                               dot=(x4, drow, c8, True), scale=asc), **T)
                    ops.spmm_rhs(gr, w_csc, gk3, stage=ops.Stage(f_out=u3, outs=[(gk2, gk3, 1.0, dt,
                                                                                  [(v, -2.0 * dt * c8)])],
                                                                 dot=(x3, drow, 1.0, True), scale=asc), **T)
                    ops.spmm_rhs(gr, w_csc, gk2, stage=ops.Stage(outs=[
                        (gk1, gk2, 1.0 / 3.0, dt / 3.0, [(v, 4.0 * dt * c8 / 3.0), (u3, -2.0 * dt / 3.0)]),
                        (acc, g, 1.0, 1.0, [(v, c8), (u3, 1.0)])], dot=(x2, drow, 1.0, True), scale=asc), **T)
                    last = n == 0 and user_rows is not None
                    ops.spmm_rhs(gr, w_csc, gk1, stage=ops.Stage(outs=[(g_new, acc, 1.0, 1.0, [])],
                                                                 out_rows=user_rows if last else None,
                                                                 dot=(y, drow, 1.0, True), scale=asc), **T)
                    if add_source:
                        gb = gb + c8 * ops.dot(g, x0) + ops.dot(gk3, x0) + ops.dot(gk2, x0) + ops.dot(gk1, x0)
                    g = g_new
                    if last:
                        lay = None  # g is in the caller's numbering now
                    continue
                if method == 'euler':
                    gk = [comb(None, [g], [dt], 1.0)]
                    xs = [y]
                    us = [u_of(gk[0])]
                else:  # midpoint
                    ym = ctx.stage_inputs[n][0]
                    gk2 = comb(None, [g], [dt], 1.0)
                    u2 = u_of(gk2)
                    gk1 = comb(None, [u2], [0.5 * dt * a], 1.0)
                    u1 = u_of(gk1)
                    gk, xs, us = [gk2, gk1], [ym, y], [u2, u1]
                for u, xv in zip(us, xs):
                    ga = ga + ops.dot(u, xv)
                if add_source:
                    for gkv in gk:
                        gb = gb + ops.dot(gkv, x0)
                g = comb(g, us, [a] * len(us), 1.0).view(g.shape)
            if nfe is not None:
                func.nfe = nfe  # the recomputed stages are not new RHS evaluations
            if drow is not None:
                ga = ops.sum_f64(drow, out=ga, accumulate=True)
            if g is None:
                g = torch.zeros_like(s0)
            for jj in out_at.get(-1, []):
                g = g + g_at(jj)
            if lay is not None:
                gu = torch.empty_like(g)
                _to_user(g, gu, lay)
                g = gu
            g = g + g_sol[0] if g._base is g_sol else g.add_(g_sol[0])  # (never g_sol itself in place)
            if sig:
                ga = ga * (a_dev * (1 - a_dev)).double()
        gy = g if ctx.needs_input_grad[0] else None
        galpha = ga.to(func.alpha_train.dtype).reshape(func.alpha_train.shape) if ctx.needs_input_grad[1] else None
        # without add_source beta_train is not on the path: no gradient, as autograd through
        # the reference's RHS leaves it (src/function_laplacian_diffusion.py:74-77)
        gbeta = gb.to(func.beta_train.dtype).reshape(func.beta_train.shape) \
            if ctx.needs_input_grad[2] and add_source else None
        return gy, galpha, gbeta, None, None, None, None


# --------------------------------------------------------------------------- regularised training path
# the methods' weights beta_i: a regulariser state advances by dt * sum_i beta_i e(k_i) per step
_REG_BETA = {'euler': (1.0,), 'midpoint': (0.0, 1.0), 'rk4': (0.125, 0.375, 0.375, 0.125)}


def _reg_kinds(func):
    """(kinds in the user's order) of a bound regularised RHS when every regulariser is one the
    fused solve carries ('kinetic', 'directional', each at most once), else None."""
    kinds = [getattr(fn, 'gnpde_reg_kind', None) for fn in getattr(func, 'regularization_fns', ())]
    if not kinds or None in kinds or len(set(kinds)) != len(kinds):
        return None
    return tuple(kinds)


def _reg_fused_ok(func, state, combine, grid_h, t_h, method):
    """The fused regularised solve (_LaplacianRegFixedGridFn): the plain fused backward's
    conditions on the integrated LaplacianODEFunc, euler or rk4, one output time (the block's
    t = [0, T]), regularisers among quadratic_cost / directional_derivative, rows the row passes take."""
    odefunc = getattr(func, 'odefunc', None)
    ok = getattr(odefunc, 'fixed_grid_reg_ok', None)
    if ok is None or not ok() or method not in ('euler', 'rk4') or len(t_h) != 2:
        return False
    if _reg_kinds(func) is None or state[0].dim() != 3 or state[0].shape[-1] > ops.ROW_MAX_COLS:
        return False
    if any(r.requires_grad or r.shape != state[0].shape[:-1] or r.dtype != torch.float32 for r in state[1:]):
        return False
    return _fused_backward_ok(odefunc, state[0], combine, grid_h, t_h)


class _LaplacianRegFixedGridFn(torch.autograd.Function):
    """_LaplacianFixedGridFn with the regulariser states r_j' = e_j(f) carried along (euler, rk4
    3/8; one output time; the caller's node numbering):

        kinetic      e(f) = 1/(2C) sum_c f^2
        directional  d(f) = 1/(2C) sum_c v^2,  v = J^T f = a (A^T f - f),  J = a (A - I)

    r' does not depend on r, so r_j(T) = sum_steps dt sum_i beta_i e_j(k_i) with the method's
    weights beta and the stage derivatives k_i: what torchdiffeq computes on the tuple state.

    Forward: the fused stage launches also store k_i (Stage.f_out); with the directional term one
    transposed K1 launch per stage gives v_i; one ops.row_energy pass per step and regulariser reads
    the step's k_i (v_i) once into an fp64 row accumulator, rounded to fp32 once at the end.  k_i
    and v_i are kept for the backward beside the stage inputs.

    Backward: the discrete adjoint of _LaplacianFixedGridFn with, for rho_j = dL/dr_j(T) [B,N],
        gk_i += q_i,  q_i = (dt beta_i / C) (rho_1 (row-scale) k_i + J (rho_2 (row-scale) v_i))
    (ops.row_axpy in place, and a K1 launch over the CSR whose epilogue adds J(.) in place), and
        d alpha += a'(alpha) (2 / a) <rho_2, r_2(T)>        (0 when a = 0: then v = 0)
    the explicit derivative of v = a (A^T - I) k with respect to a, summed over the stages; the
    terms <u_i, x_i> and <gk_i, x0> follow from the enlarged gk_i.  rk4 writes gk_4 = dt/8 h with
    h = g + q_4 / (dt/8) so that u_4 = dt/8 (A^T - I) h rides in the launches' epilogues as in the
    unregularised adjoint; the other gk_i are formed against g (their q_i is added after the
    epilogue that forms them)."""

    @staticmethod
    def forward(ctx, y0, alpha_train, beta_train, func, method, steps, kinds, *r0):
        y = y0.detach().contiguous()
        B, N, C = y.shape
        R = B * N
        o = laplacian_operands(func, y0, private_csc=True, snapshot=True)
        directional = 'directional' in kinds
        if directional:  # the CSR-order weights of J (.) in the backward: this node's own gather
            o.w_csr = o.g.gather_weights(o.w.detach().float() if o.w.dtype != torch.float32 else o.w.detach())
        acc = torch.zeros(len(kinds), R, dtype=torch.float64, device=y.device)
        beta = _REG_BETA[method]
        starts, stage_inputs, ks_all, vs_all = [], [], [], []
        sol = torch.empty((2,) + tuple(y.shape), dtype=y.dtype, device=y.device)
        sol[0].copy_(y)
        for n_step, (ta, tb) in enumerate(steps):
            dt = tb - ta
            starts.append(y)
            ks = [torch.empty_like(y) for _ in beta]
            y1 = sol[1] if n_step == len(steps) - 1 else torch.empty_like(y)
            if method == 'euler':
                func.rhs_stage(ta, y, ops.Stage(f_out=ks[0], outs=[(y1, y, 1.0, dt, [])]))
                stage_inputs.append([])
            else:  # rk4 3/8 rule, the stage inputs as _fused_step forms them
                x2, x3, x4 = (torch.empty_like(y) for _ in range(3))
                func.rhs_stage(ta, y, ops.Stage(f_out=ks[0], outs=[(x2, y, 1.0, dt / 3.0, [])]))
                func.rhs_stage(ta + dt / 3.0, x2, ops.Stage(f_out=ks[1], outs=[(x3, x2, -1.0, dt, [(y, 2.0)])]))
                func.rhs_stage(ta + dt * 2.0 / 3.0, x3,
                               ops.Stage(f_out=ks[2], outs=[(x4, x3, -1.0, dt, [(x2, 2.0)])]))
                func.rhs_stage(tb, x4, ops.Stage(f_out=ks[3], outs=[(y1, x4, 0.375, dt * 0.125,
                                                                      [(x3, 0.75), (y, -0.125)])]))
                stage_inputs.append([x2, x3, x4])
            coefs = [dt * b / (2.0 * C) for b in beta]
            vs = None
            if directional:
                vs = [ops.spmm_rhs(o.g, o.w_csc, k, alpha=o.alpha, rhs=True, alpha_sigmoid=o.sig, transpose=True)
                      for k in ks]
            for j, kind in enumerate(kinds):
                ops.row_energy(ks if kind == 'kinetic' else vs, coefs, acc=acc[j], accumulate=True)
            ks_all.append(ks)
            vs_all.append(vs)
            y = y1
        regs = tuple(torch.stack([r.detach(), r.detach() + acc[j].float().view(B, N)], 0) for j, r in enumerate(r0))
        ctx.o, ctx.acc, ctx.kinds = o, acc, kinds
        ctx.a_dev = torch.sigmoid(o.alpha) if o.sig else o.alpha
        ctx.a_scale = ctx.a_dev.reshape(()).float().contiguous()
        ctx.a_host = _host_scalar(ctx.a_dev)
        ctx.func, ctx.method, ctx.steps = func, method, steps
        ctx.starts, ctx.stage_inputs, ctx.ks, ctx.vs = starts, stage_inputs, ks_all, vs_all
        return (sol,) + regs

    @staticmethod
    def backward(ctx, g_sol, *g_regs):
        func, method, steps, kinds = ctx.func, ctx.method, ctx.steps, ctx.kinds
        o = ctx.o
        with torch.no_grad():
            gr, w_csc, sig, add_source, x0 = o.g, o.w_csc, o.sig, o.add_source, o.x0
            g_sol = g_sol.contiguous()
            one = _device_one(g_sol.device)
            a_dev, asc = ctx.a_dev, ctx.a_scale
            B, N, C = ctx.starts[0].shape
            rho = {kind: g_regs[j][1].contiguous().float() for j, kind in enumerate(kinds) if g_regs[j] is not None}
            rho1, rho2 = rho.get('kinetic'), rho.get('directional')
            beta = _REG_BETA[method]
            acc64 = torch.zeros(2 + B * N, dtype=torch.float64, device=g_sol.device)
            ga, gb, drow = acc64[0], acc64[1], acc64[2:]
            T = dict(alpha=one, rhs=True, alpha_sigmoid=False, transpose=True)
            e = lambda: torch.empty_like(g)  # noqa: E731

            def add_q(gk, n, i, scale, base=None):
                """gk = (base or gk) + scale * q_i of step n."""
                dt = steps[n][1] - steps[n][0]
                coef = scale * dt * beta[i] / C
                if rho1 is not None:
                    ops.row_axpy(gk if base is None else base, [(coef, rho1, ctx.ks[n][i])], out=gk)
                elif base is not None:
                    gk.copy_(base)
                if rho2 is not None:
                    tmp = ops.row_axpy(None, [(coef, rho2, ctx.vs[n][i])])
                    ops.spmm_rhs(gr, o.w_csr, tmp, alpha=o.alpha, rhs=True, alpha_sigmoid=sig,
                                 stage=ops.Stage(outs=[(gk, gk, 1.0, 1.0, [])]))

            g = g_sol[1].clone()
            a = ctx.a_host() if method != 'rk4' else None
            for n in range(len(steps) - 1, -1, -1):
                dt = steps[n][1] - steps[n][0]
                y = ctx.starts[n]
                if method == 'euler':
                    gk = ops.rk_combine(None, [g], [dt], 1.0)
                    add_q(gk, n, 0, 1.0)
                    g_new = e()
                    ops.spmm_rhs(gr, w_csc, gk, stage=ops.Stage(outs=[(g_new, g, 1.0, a, [])],
                                                                dot=(y, drow, 1.0, True)), **T)
                    if add_source:
                        gb = gb + ops.dot(gk, x0)
                    g = g_new
                    continue
                x2, x3, x4 = ctx.stage_inputs[n]
                c8 = dt / 8.0
                h, v, gk3, u3, gk2, gk1, acc, g_new = (e() for _ in range(8))
                add_q(h, n, 3, 1.0 / c8, base=g)  # gk4 = c8 h
                ops.spmm_rhs(gr, w_csc, h, stage=ops.Stage(f_out=v, outs=[(gk3, g, 3 * c8, dt * c8, [])],
                                                           dot=(x4, drow, c8, True), scale=asc), **T)
                add_q(gk3, n, 2, 1.0)
                ops.spmm_rhs(gr, w_csc, gk3, stage=ops.Stage(f_out=u3, outs=[(gk2, g, 3 * c8, dt, [(v, -dt * c8)])],
                                                             dot=(x3, drow, 1.0, True), scale=asc), **T)
                add_q(gk2, n, 1, 1.0)
                ops.spmm_rhs(gr, w_csc, gk2, stage=ops.Stage(outs=[
                    (gk1, g, c8, dt / 3.0, [(v, dt * c8), (u3, -dt / 3.0)]),
                    (acc, g, 1.0, 1.0, [(v, c8), (u3, 1.0)])], dot=(x2, drow, 1.0, True), scale=asc), **T)
                add_q(gk1, n, 0, 1.0)
                ops.spmm_rhs(gr, w_csc, gk1, stage=ops.Stage(outs=[(g_new, acc, 1.0, 1.0, [])],
                                                             dot=(y, drow, 1.0, True), scale=asc), **T)
                if add_source:
                    gb = gb + c8 * ops.dot(h, x0) + ops.dot(gk3, x0) + ops.dot(gk2, x0) + ops.dot(gk1, x0)
                g = g_new
            ga = ops.sum_f64(drow, out=ga, accumulate=True)
            if rho2 is not None:
                # the explicit derivative of v = a (A^T - I) k to a: (2 / a) <rho_2, r_2(T)>, fp64
                ex = ops.sum_f64(rho2.double().view(-1) * ctx.acc[kinds.index('directional')])
                ad = a_dev.double()
                ga = ga + torch.where(ad != 0, 2.0 * ex / torch.where(ad != 0, ad, torch.ones_like(ad)),
                                      torch.zeros_like(ex))
            g = g.add_(g_sol[0])
            if sig:
                ga = ga * (a_dev * (1 - a_dev)).double()
        gy = g if ctx.needs_input_grad[0] else None
        galpha = ga.to(func.alpha_train.dtype).reshape(func.alpha_train.shape) if ctx.needs_input_grad[1] else None
        gbeta = gb.to(func.beta_train.dtype).reshape(func.beta_train.shape) \
            if ctx.needs_input_grad[2] and add_source else None
        return (gy, galpha, gbeta, None, None, None, None) + (None,) * len(kinds)


class _TupleCombine(object):
    """A stage combination applied to every component of a tuple state."""

    def __init__(self, combine):
        self.combine = combine

    def __call__(self, y0, ks, coefs, scale):
        return tuple(self.combine(y0[i], [k[i] for k in ks], coefs, scale) for i in range(len(y0)))


def _odeint_tuple(func, state, t, method, options, combine):
    """odeint over a tuple state (the regularised RHS: (x, r_1, ...)), torchdiffeq's convention: a
    tuple of [len(t), ...] tensors.  Fixed-grid methods only: the fused regularised solve when it
    applies (_reg_fused_ok), else autograd through every RHS call and stage combination."""
    if method in ADAPTIVE_METHODS:
        raise NotImplementedError("gnpde.odeint: a tuple state (ODE regularisers) under the adaptive method %r "
                                  "is out of scope; use one of %s" % (method, ', '.join(FIXED_METHODS)))
    if method in MULTISTEP_METHODS:
        raise NotImplementedError("gnpde.odeint: a tuple state (ODE regularisers) under the multistep method %r "
                                  "is out of scope; use one of %s" % (method, ', '.join(FIXED_METHODS)))
    if method not in FIXED_METHODS:
        raise NotImplementedError("gnpde.odeint: method %r not supported" % method)
    if len(state) < 1 or not all(isinstance(s, torch.Tensor) for s in state):
        raise ValueError("gnpde.odeint: a tuple state holds tensors")
    if any(s.dtype == torch.bfloat16 for s in state):
        raise NotImplementedError("gnpde.odeint: a tuple state (ODE regularisers) with a bf16 state is out of "
                                  "scope: the regulariser passes are fp32")
    if combine is None:
        if not state[0].is_cuda:
            raise RuntimeError("gnpde.odeint: y0 must be a ROCm device tensor (stage combinations run in HIP)")
        combine = _Combine()
    t_h = _host_times(t)
    grid_h = _host_grid(t_h, t.dtype, options.get('step_size'))
    if not (grid_h[0] == t_h[0] and grid_h[-1] == t_h[-1]):
        raise AssertionError("time grid does not cover t")
    steps = list(zip(grid_h[:-1], grid_h[1:]))
    if _reg_fused_ok(func, state, combine, grid_h, t_h, method) and \
            _nfe_headroom(func.odefunc, len(steps) * RHS_PER_STEP[method]):
        odeint.last_reg_path = 'fused'
        f = func.odefunc
        return _LaplacianRegFixedGridFn.apply(state[0], f.alpha_train, f.beta_train, f, method, steps,
                                              _reg_kinds(func), *state[1:])
    odeint.last_reg_path = 'restated'
    tc = _TupleCombine(combine)
    solution = [state]
    j = 1
    yc = state
    for ta, tb in steps:
        y1 = _fixed_step(method, func, ta, tb - ta, tb, yc, tc)
        while j < len(t_h) and tb >= t_h[j]:
            solution.append(tuple(_linear_interp(ta, tb, a, b, t_h[j]) for a, b in zip(yc, y1)))
            j += 1
        yc = y1
    while j < len(t_h):
        solution.append(yc)
        j += 1
    return tuple(torch.stack([s[i] for s in solution], 0) for i in range(len(state)))


def _host_scalar(v):
    """A device scalar's value for the host later: an asynchronous copy into pinned
    memory behind an event; the returned callable waits for that event only (not
    for the work queued after it) and returns the float."""
    if not v.is_cuda:
        val = float(v)
        return lambda: val
    h = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
    h.copy_(v, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()

    def get():
        ev.synchronize()
        return float(h)
    return get


_ONES = {}


def _device_one(device):
    """A read-only fp32 1.0 on `device` (the adjoint launches' alpha operand), made once
    per device rather than filled per backward."""
    one = _ONES.get(device)
    if one is None:
        one = torch.ones((), dtype=torch.float32, device=device)
        if not torch.cuda.is_current_stream_capturing():  # a captured fill runs only on replay
            _ONES[device] = one
    return one


# Host copies of time grids.  A solve needs t on the host (the loop is there); a
# device t costs a device->host copy, i.e. a wait for everything queued before it.
# The values of a device t are kept per tensor object (and version), so a model
# that integrates over the same ``self.t`` every forward (ODEblock) reads it once.
_T_HOST = {}
_GRIDS = {}


def _host_times(t):
    if not t.is_cuda:
        return [float(v) for v in t.tolist()]
    hit = _T_HOST.get(id(t))
    if hit is not None and hit[0]() is t and hit[1] == t._version and hit[2] == t.data_ptr():
        return hit[3]
    vals = [float(v) for v in t.tolist()]
    if len(_T_HOST) >= 64:
        _T_HOST.clear()
    _T_HOST[id(t)] = (weakref.ref(t), t._version, t.data_ptr(), vals)
    return vals


def _host_grid(t_h, dtype, step_size):
    """torchdiffeq's grid for the host times t_h (built with CPU torch ops in t's
    dtype: IEEE on the host as on the device, the same values), cached."""
    if step_size is None:
        return list(t_h)
    key = (tuple(t_h), dtype, float(step_size))
    g = _GRIDS.get(key)
    if g is None:
        g = [float(v) for v in fixed_grid(torch.tensor(t_h, dtype=dtype), step_size).tolist()]
        if len(_GRIDS) >= 256:
            _GRIDS.clear()
        _GRIDS[key] = g
    return g


def odeint_fixed(func, y0, t, method, step_size=None, combine=None, graph=None, step_hook=None):
    """``step_hook(y1, t1, layout)`` (the early-stop integrator's score): called after every grid
    step with the state it produced, in the numbering ``layout`` (None: the caller's); the
    steps are then driven one at a time — the same launches and replayed one-step graphs,
    the same bits, nothing read by the host in between.  None: the plain solve."""
    combine = combine or _Combine()
    t_h = _host_times(t)
    grid_h = _host_grid(t_h, t.dtype, step_size)
    if not (grid_h[0] == t_h[0] and grid_h[-1] == t_h[-1]):
        raise AssertionError("time grid does not cover t")
    steps = list(zip(grid_h[:-1], grid_h[1:]))
    if _fusable(func, y0, combine):
        cp = _padded_width(func, y0)
        if cp is not None:
            C = y0.shape[-1]
            yp = torch.zeros(*y0.shape[:-1], cp, dtype=y0.dtype, device=y0.device)
            yp[..., :C] = y0
            out = _solve_fused(func, yp, t_h, steps, method, graph, step_hook)
            return out[..., :C].contiguous()
        return _solve_fused(func, y0, t_h, steps, method, graph, step_hook)
    if step_hook is None and _fused_backward_ok(func, y0, combine, grid_h, t_h) and _nfe_headroom(func, len(steps) * RHS_PER_STEP[method]):
        return _LaplacianFixedGridFn.apply(y0, func.alpha_train, func.beta_train, func, method, steps, t_h)
    solution = [y0]
    j = 1
    yc = y0
    for ta, tb in steps:
        y1 = _fixed_step(method, func, ta, tb - ta, tb, yc, combine)
        if step_hook is not None:
            step_hook(y1, tb, None)
        while j < len(t_h) and tb >= t_h[j]:
            solution.append(_linear_interp(ta, tb, yc, y1, t_h[j]))
            j += 1
        yc = y1
    while j < len(t_h):  # a degenerate grid (t0 == t1): the state itself
        solution.append(yc)
        j += 1
    return torch.stack(solution, 0)


def _solve_fused(func, y0, t_h, steps, method, graph, step_hook=None):
    """A fixed-grid solve whose RHS emits the stage combinations itself (gnpde
    ODEFuncs, no autograd), in the graph's node numbering when the module offers
    one (ops.NodeLayout: bit-identical results).

    The solution tensor is allocated once; the entry pass writes its t0 slice
    and the working state (renumbered) in one read of y0; runs of equal steps
    replay captured block graphs over two ping-pong buffers; when the last
    requested time is the last grid point, the last step's epilogue writes the
    result straight into the solution in the caller's numbering (out_rows), so
    there is no exit pass.  Other output times are copied out (or linearly
    interpolated, as torchdiffeq) when their step has run."""
    lay = _node_layout(func, y0)
    n = len(steps)
    if graph is None:
        # a RHS with a collective inside (dist.RowShardedLaplacian) opts out of capture
        graph = n >= GRAPH_MIN_STEPS and _replayable(func)
    sol = torch.empty((len(t_h),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
    pool = _state_pool(func, y0)
    bufs, ws = pool.bufs, pool.ws
    inplace = _steps_inplace(method, func, y0)
    _entry_copy(y0.contiguous(), bufs[0], sol[0], lay.order if lay is not None else None)
    if lay is not None:
        func._layout = lay
    try:
        fz = None
        if lay is not None and n >= 1 and steps[-1][1] == t_h[-1] and (n == 1 or steps[-2][1] < t_h[-1]):
            fz = _frozen_rows(func, method, bufs[0], inplace, t_h, step_hook)
        if fz is not None:
            frozen_stats['solves'] += 1
        sg = None
        if graph and n >= 2:
            # the first step's dt; the captured graphs replay only runs of exactly this dt
            state = _capture_state(func, bufs[0])
            key = _graph_cache_key(func, method, bufs[0], state)
            dt0 = steps[0][1] - steps[0][0]
            hit = _GRAPH_CACHE.get(func) if key is not None else None
            if (hit is not None and hit[0] == key and hit[1].dt == dt0 and hit[1].pool is pool
                    and hit[1].inplace == inplace and hit[1].frozen is fz):
                sg = hit[1]
            else:
                sg = _StepGraphs(method, func, dt0, pool, inplace, fz)
                if key is not None:
                    _GRAPH_CACHE[func] = (key, sg, state)
        p = 0      # the state is in bufs[p]
        i = 0      # next step to run
        j = 1      # next output time
        if step_hook is not None:
            _hooked_steps(func, method, steps, t_h, sol, lay, pool, sg, inplace, step_hook)
            j = len(t_h)
        while j < len(t_h):
            if i >= n:  # a degenerate grid (t0 == t1): the state itself
                _to_user(bufs[p], sol[j], lay)
                j += 1
                continue
            m = i
            while m < n - 1 and steps[m][1] < t_h[j]:
                m += 1
            p = _advance(func, method, steps, i, m, p, pool, sg, inplace, fz)
            ta, tb = steps[m]
            if m == n - 1 and j == len(t_h) - 1 and t_h[j] == tb:
                # the last step writes the result in the caller's numbering
                _fused_step(method, func, ta, tb - ta, tb, bufs[p], ws, out=sol[j],
                            out_rows=lay.order32 if lay is not None else None, inplace=inplace,
                            frozen=(fz, n) if fz is not None else None)
                j += 1
                break
            # an output time inside the step is interpolated from the state before it: that
            # step keeps its input (the ping-pong form)
            assert fz is None  # (a solve that leaves frozen rows out reads its state at its last step only)
            p = _advance(func, method, steps, m, m + 1, p, pool, sg, inplace and t_h[j] == tb)
            ya, yb = bufs[1 - p], bufs[p]
            while j < len(t_h) and tb >= t_h[j]:
                if t_h[j] == tb:
                    _to_user(yb, sol[j], lay)
                else:
                    _to_user(_linear_interp(ta, tb, ya, yb, t_h[j]), sol[j], lay)
                j += 1
            i = m + 1
    finally:
        func._layout = None
    return sol


def _hooked_steps(func, method, steps, t_h, sol, lay, pool, sg, inplace, step_hook):
    """_solve_fused's loop with ``step_hook`` after every grid step: one _advance per step (a
    replayed one-step graph once warm), the hook's launch behind it on the stream.  The
    last step stores the result in the caller's numbering as the plain solve does, and the
    hook sees that slice (layout None)."""
    bufs, ws = pool.bufs, pool.ws
    n = len(steps)
    p, j = 0, 1
    for m, (ta, tb) in enumerate(steps):
        if m == n - 1 and j == len(t_h) - 1 and t_h[j] == tb:
            _fused_step(method, func, ta, tb - ta, tb, bufs[p], ws, out=sol[j],
                        out_rows=lay.order32 if lay is not None else None, inplace=inplace)
            step_hook(sol[j], tb, None)
            return
        inside = j < len(t_h) and tb >= t_h[j] and t_h[j] != tb  # interpolated from the step's input
        p = _advance(func, method, steps, m, m + 1, p, pool, sg, inplace and not inside)
        step_hook(bufs[p], tb, lay)
        while j < len(t_h) and tb >= t_h[j]:
            if t_h[j] == tb:
                _to_user(bufs[p], sol[j], lay)
            else:
                _to_user(_linear_interp(ta, tb, bufs[1 - p], bufs[p], t_h[j]), sol[j], lay)
            j += 1
    while j < len(t_h):  # a degenerate grid (t0 == t1): the state itself
        _to_user(bufs[p], sol[j], lay)
        j += 1


def _advance(func, method, steps, i, m, p, pool, sg, inplace=False, frozen=None):
    """Run steps i .. m-1 from bufs[p] (``inplace``: in bufs[p]; ``frozen``: leaving the graph's
    frozen rows out, _frozen_rows); returns the parity the state ends in.
    Steps of the captured dt go through block graphs (binary decomposition),
    others — and every step while the module is not warm or too close to its
    max_nfe — run eagerly (a MaxNFEException is then raised at the exact call)."""
    bufs, ws = pool.bufs, pool.ws
    first = sg is not None and not sg.warm and i == 0 and p == 0
    while i < m:
        ta, tb = steps[i]
        dt = tb - ta
        if first and i == 1 and sg.warm:
            # the first solve of a new entry ran step 0 eagerly; the next solves will replay
            # steps 0 .. m-1 from bufs[0]: capture that decomposition now too (capture only
            # records launches), so a later solve of the same length captures nothing
            k = 1
            while k < m and steps[k][1] - steps[k][0] == sg.dt:
                k += 1
            q = 0
            for s in _pow2_blocks(k, GRAPH_BLOCK):
                sg.graph(func, s, q)
                q = sg.end(s, q)
        if sg is not None and sg.warm and dt == sg.dt and sg.inplace == inplace and sg.frozen is frozen:
            k = 1
            while i + k < m and steps[i + k][1] - steps[i + k][0] == dt:
                k += 1
            if _nfe_headroom(func, k * sg.n_rhs):
                for s in _pow2_blocks(k, GRAPH_BLOCK):
                    p = sg.replay(func, s, p)
                i += k
                continue
        if inplace:
            _fused_step(method, func, ta, dt, tb, bufs[p], ws, inplace=True,
                        frozen=(frozen, None) if frozen is not None else None)
        else:
            _fused_step(method, func, ta, dt, tb, bufs[p], ws, out=bufs[1 - p])
            p = 1 - p
        if sg is not None and dt == sg.dt:
            sg.warm = True
        i += 1
    return p


# --------------------------------------------------------------------------- multistep (Adams)
def _combine_chunks(combine, base, ks, coefs, scale, width=_lib.STAGE_MAX_K):
    """base + scale * sum_j coefs[j] ks[j] for more operands than one combine pass takes
    (gnpde_rk_combine_f32: 8, the bf16 stage pass: 6): passes of ``width``, each on the last."""
    acc = base
    for i in range(0, len(ks), width):
        acc = combine(acc, list(ks[i:i + width]), list(coefs[i:i + width]), scale)
    return acc


class _AdamsBashforthMoulton(object):
    """torchdiffeq 0.2.x fixed_adams.AdamsBashforthMoulton restated (explicit_adams: the
    Adams-Bashforth predictor alone; implicit_adams: with the Adams-Moulton corrector run as a
    fixed-point iteration), on torchdiffeq's fixed grid with linear interpolation onto the
    requested times.

    Per step from (t0, y0) to t1 = t0 + dt: f0 = func(t0, y0) joins the front of ``prev_f`` (at
    most max_order - 1 values, the oldest falls off); order = min(len(prev_f), max_order - 1).
    order < 3: the step is one rk4 (3/8 rule) step with k1 = f0, nothing else.  Otherwise
    dy = dt sum_j AB[order][j] prev_f[j]; implicit: with m = AM[order + 1] and delta = dt sum_j
    m[j + 1] prev_f[j], up to max_iters times  dy <- dt m[0] func(t1, y0 + dy) + delta  until
    max |dy_old - dy| / (atol + rtol max(|dy_old|, |dy|)) < 1 (a NaN is not converged); a step
    that never converged warns (once per solve) and drops the oldest entry of prev_f.
    y1 = y0 + dy.

    Two loops run this: ``_solve_fused`` (no autograd, device fp32 state, a RHS with
    rhs_stage: f0 and the corrector's f stored by the RHS epilogue, the history in a ring of
    buffers, the predictor / corrector passes of csrc/adams.hip, the convergence test on the
    device) and ``_solve_restated`` (anything else: torch tensors through ``combine``, one host
    decision per corrector iteration as torchdiffeq; autograd flows through it).

    After a solve: ``iterations`` (corrector iterations of every step; 0 for rk4 and explicit
    steps), ``converged`` (per step), ``ratios`` (the restated loop: every iteration's ratio;
    the fused loop: the last ratio of each corrector step) and ``path``."""

    def __init__(self, func, y0, rtol, atol, combine, implicit, max_order=None, max_iters=None):
        max_order = adams_coefficients.MAX_ORDER if max_order is None else int(max_order)
        if max_order > adams_coefficients.MAX_ORDER:
            raise ValueError("gnpde.odeint: max_order=%d: the Adams tables end at order %d"
                             % (max_order, adams_coefficients.MAX_ORDER))
        if max_order < 4:
            warnings.warn("gnpde.odeint: max_order=%d < 4: every step of the Adams solver is an rk4 step" % max_order)
        self.func, self.y0, self.combine, self.implicit = func, y0, combine, implicit
        self.rtol, self.atol = float(rtol), float(atol)
        self.hist_len = max(max_order - 1, 0)
        self.max_iters = 4 if max_iters is None else int(max_iters)
        self.iterations, self.converged, self.ratios, self.path = [], [], [], None
        self._warned = False

    def _not_converged(self, t1):
        if not self._warned:
            warnings.warn("gnpde.odeint: implicit_adams: the corrector did not converge in %d iterations at t = %g; "
                          "consider increasing max_iters or reducing step_size" % (self.max_iters, t1))
            self._warned = True

    def integrate(self, t, step_size):
        t_h = _host_times(t)
        grid_h = _host_grid(t_h, t.dtype, step_size)
        if not (grid_h[0] == t_h[0] and grid_h[-1] == t_h[-1]):
            raise AssertionError("time grid does not cover t")
        steps = list(zip(grid_h[:-1], grid_h[1:]))
        func, y0 = self.func, self.y0
        if type(func).__module__ == dist_module_name():
            raise NotImplementedError("gnpde.odeint: explicit_adams / implicit_adams do not cover the sharded RHS "
                                      "classes of gnpde.dist (the history ring is not sharded); use rk4 or an "
                                      "adaptive method")
        if _fusable(func, y0, self.combine) and y0.is_cuda and y0.dtype == torch.float32:
            self.path = 'fused'
            return self._solve_fused(t_h, steps)
        self.path = 'restated'
        return self._solve_restated(t_h, steps)

    # ---- torch tensors through ``combine``
    def _solve_restated(self, t_h, steps):
        func, combine = self.func, self.combine
        prev_f = collections.deque(maxlen=self.hist_len)
        solution = [self.y0]
        j = 1
        yc = self.y0
        for ta, tb in steps:
            dt = tb - ta
            f0 = func(ta, yc)
            prev_f.appendleft(f0)
            order = min(len(prev_f), self.hist_len)
            its, conv = 0, True
            if order < 3:  # rk4_alt_step_func with k1 = f0
                k2 = func(ta + dt / 3.0, combine(yc, [f0], [1.0 / 3.0], dt))
                k3 = func(ta + dt * 2.0 / 3.0, combine(yc, [f0, k2], [-1.0 / 3.0, 1.0], dt))
                k4 = func(tb, combine(yc, [f0, k2, k3], [1.0, -1.0, 1.0], dt))
                y1 = combine(yc, [f0, k2, k3, k4], [0.125, 0.375, 0.375, 0.125], dt)
            else:
                hist = list(prev_f)[:order]
                dy = _combine_chunks(combine, None, hist, adams_coefficients.ADAMS_BASHFORTH[order], dt)
                if self.implicit:
                    m = adams_coefficients.ADAMS_MOULTON[order + 1]
                    delta = _combine_chunks(combine, None, hist, m[1:], dt)
                    conv = False
                    for _ in range(self.max_iters):
                        dy_old = dy
                        f = func(tb, yc + dy)
                        dy = combine(delta, [f], [m[0]], dt)
                        with torch.no_grad():
                            tol = self.atol + self.rtol * torch.maximum(dy_old.abs(), dy.abs())
                            ratio = float(((dy_old - dy).abs() / tol).max())
                        its += 1
                        self.ratios.append(ratio)
                        if ratio < 1.0:  # (a NaN compares false)
                            conv = True
                            break
                    if not conv:
                        self._not_converged(tb)
                        prev_f.pop()
                y1 = yc + dy
            self.iterations.append(its)
            self.converged.append(conv)
            while j < len(t_h) and tb >= t_h[j]:
                solution.append(_linear_interp(ta, tb, yc, y1, t_h[j]))
                j += 1
            yc = y1
        while j < len(t_h):  # a degenerate grid (t0 == t1): the state itself
            solution.append(yc)
            j += 1
        return torch.stack(solution, 0)

    # ---- the HIP passes
    def _solve_fused(self, t_h, steps):
        func = self.func
        y0 = self.y0.contiguous()
        sol = torch.empty((len(t_h),) + tuple(y0.shape), dtype=y0.dtype, device=y0.device)
        sol[0].copy_(y0)
        ws = _state_pool(func, y0).ws
        # the state and its successor (swapped after every step), the rk4 stage inputs, the
        # increment, the corrector's constant part and its RHS value, and the history ring
        y, x = ws.get('adams_y', y0), ws.get('adams_x', y0)
        dy, delta, f = ws.get('adams_dy', y0), ws.get('adams_delta', y0), ws.get('adams_f', y0)
        free = [ws.get('adams_h%d' % k, y0) for k in range(max(self.hist_len, 1))]
        status = dict.get(ws, 'adams_status')
        if status is None or status.device != y0.device:
            status = ws['adams_status'] = ops.adams_workspace(y0.device)
        prev_f = collections.deque()
        y.copy_(y0)
        chunk = 1  # corrector iterations enqueued before the first status read of a step
        j = 1
        for ta, tb in steps:
            dt = tb - ta
            # f0 into a ring buffer: the one the oldest entry leaves, or a free one
            if self.hist_len == 0:
                slot = free[0]
            elif len(prev_f) == self.hist_len:
                slot = prev_f.pop()
            else:
                slot = free.pop()
            order = min(len(prev_f) + 1, self.hist_len)
            its, conv = 0, True
            if order < 3:
                # rk4_alt_step_func with k1 = f0: _fused_step's ping-pong form, the first launch
                # storing f0 as well
                a, b, c = ws.get('a', y0), ws.get('b', y0), ws.get('c', y0)
                func.rhs_stage(ta, y, ops.Stage(f_out=slot, outs=[(a, y, 1.0, dt / 3.0, [])]))
                if self.hist_len:
                    prev_f.appendleft(slot)
                func.rhs_stage(ta + dt / 3.0, a, ops.Stage(outs=[(b, a, -1.0, dt, [(y, 2.0)])]))
                func.rhs_stage(ta + dt * 2.0 / 3.0, b, ops.Stage(outs=[(c, b, -1.0, dt, [(a, 2.0)])]))
                func.rhs_stage(tb, c, ops.Stage(outs=[(x, c, 0.375, dt * 0.125, [(b, 0.75), (y, -0.125)])]))
            else:
                func.rhs_stage(ta, y, ops.Stage(f_out=slot))
                prev_f.appendleft(slot)
                hist = list(prev_f)[:order]
                cdy = [dt * v for v in adams_coefficients.ADAMS_BASHFORTH[order]]
                if not self.implicit:
                    ops.adams_predict(y, hist, cdy, dy, x)
                else:
                    m = adams_coefficients.ADAMS_MOULTON[order + 1]
                    ops.adams_predict(y, hist, cdy, dy, x, cdelta=[dt * v for v in m[1:]], delta=delta)
                    ops.adams_status_reset(status)
                    conv, ratio = False, float('nan')
                    while not conv and its < self.max_iters:
                        n = max(1, min(chunk if its == 0 else 1, self.max_iters - its))
                        if n > 1 and not _nfe_headroom(func, n):
                            n = 1  # near max_nfe: one at a time, the guard raises at the exact call
                        nfe = getattr(func, 'nfe', None)
                        for _ in range(n):
                            func.rhs_stage(tb, x, ops.Stage(f_out=f))
                            ops.adams_correct(f, delta, y, dy, x, dt * m[0], self.rtol, self.atol, status)
                        conv, done, ratio = ops.adams_status(status)  # the one host read of the chunk
                        if nfe is not None:
                            func.nfe = nfe + (done - its)  # launches behind the converged one were gated off
                        its = done
                    if its:
                        self.ratios.append(ratio)
                    chunk = max(1, its)
                    if not conv:
                        self._not_converged(tb)
                        free.append(prev_f.pop())
            self.iterations.append(its)
            self.converged.append(conv)
            while j < len(t_h) and tb >= t_h[j]:
                if t_h[j] == tb:
                    sol[j].copy_(x)
                else:
                    sol[j].copy_(_linear_interp(ta, tb, y, x, t_h[j]))
                j += 1
            y, x = x, y
        while j < len(t_h):  # a degenerate grid (t0 == t1): the state itself
            sol[j].copy_(y)
            j += 1
        return sol


def dist_module_name():
    return __name__.rsplit('.', 1)[0] + '.dist'


def odeint_adams(func, y0, t, method, rtol, atol, options, combine):
    """explicit_adams / implicit_adams (options: step_size, max_order <= 12, max_iters)."""
    if options.get('gnpde_accept_hook') is not None or options.get('gnpde_max_attempts') is not None:
        raise NotImplementedError("gnpde.odeint: the early-stop hooks cover rk4 and the adaptive methods, not %s"
                                  % method)
    solver = _AdamsBashforthMoulton(func, y0, rtol, atol, combine, method == 'implicit_adams',
                                    max_order=options.get('max_order'), max_iters=options.get('max_iters'))
    out = solver.integrate(t, options.get('step_size'))
    odeint.last_path = 'adams_' + solver.path
    odeint.last_n_steps = len(solver.iterations)
    odeint.last_adams = {'iterations': solver.iterations, 'converged': solver.converged, 'ratios': solver.ratios}
    return out


class _RKAdaptive(object):
    """torchdiffeq RKAdaptiveStepsizeODESolver (0.2.x rk_common.py) restated for an
    explicit embedded tableau (dopri5, bosh3, fehlberg2, adaptive_heun)."""

    def __init__(self, func, y0, rtol, atol, combine, method='dopri5', first_step=None, safety=0.9, ifactor=10.0,
                 dfactor=0.2, max_num_steps=2 ** 31 - 1, norm=_rms_norm, accept_hook=None, max_attempts=None):
        (self.order, self.alpha, self.beta, self.c_sol, self.c_error, self.c_mid) = _TABLEAUS[method]
        # FSAL tableaus (dopri5, bosh3): c_sol == beta[-1] and c_sol[-1] == 0, so y1 is the last stage input
        self.fsal = self.c_sol[-1] == 0 and list(self.c_sol[:-1]) == list(self.beta[-1])
        dtype = torch.promote_types(torch.float64, y0.dtype)
        dev = y0.device
        self.func, self.y0, self.combine, self.norm = func, y0, combine, norm
        self.dtype = dtype
        # the controller's scalars as given; their device tensors (the torch restatement's
        # arithmetic) are made on first use, so the fused solver (host floats) moves none
        self._scalars = {'rtol': rtol, 'atol': atol, 'safety': safety, 'ifactor': ifactor, 'dfactor': dfactor,
                         'first_step': first_step}
        self._tensors = {}
        self._dev = dev
        self.max_num_steps = max_num_steps
        self.n_steps = 0
        # The early-stop integrator's additions (inert when None).  accept_hook(y1, t1, layout):
        # called after every accepted step with the buffer that holds y1.  max_attempts: the
        # solve stops after that many attempts, rejected ones included (src/early_stop_solver.py:
        # 77-88), and returns the state at the last accepted t1 (y0 if none) for every output
        # time not reached — where max_num_steps raises.
        self.accept_hook, self.max_attempts = accept_hook, max_attempts
        self.capped = False

    def _scalar_tensor(self, name):
        v = self._tensors.get(name)
        if v is None:
            raw = self._scalars[name]
            v = None if raw is None else torch.as_tensor(raw, dtype=self.dtype, device=self._dev)
            self._tensors[name] = v
        return v

    rtol = property(lambda self: self._scalar_tensor('rtol'))
    atol = property(lambda self: self._scalar_tensor('atol'))
    safety = property(lambda self: self._scalar_tensor('safety'))
    ifactor = property(lambda self: self._scalar_tensor('ifactor'))
    dfactor = property(lambda self: self._scalar_tensor('dfactor'))
    first_step = property(lambda self: self._scalar_tensor('first_step'))

    def _select_initial_step(self, t0, f0):
        y0, rtol, atol, norm, func = self.y0, self.rtol, self.atol, self.norm, self.func
        dtype, dev = y0.dtype, y0.device
        t_dtype = t0.dtype
        scale = atol + torch.abs(y0) * rtol
        d0 = norm(y0 / scale).abs()
        d1 = norm(f0 / scale).abs()
        if d0 < 1e-5 or d1 < 1e-5:
            h0 = torch.tensor(1e-6, dtype=dtype, device=dev)
        else:
            h0 = 0.01 * d0 / d1
        h0 = h0.abs()
        y1 = y0 + h0 * f0
        f1 = func(t0.to(dtype) + h0, y1)
        d2 = torch.abs(norm((f1 - f0) / scale) / h0)
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = torch.max(torch.tensor(1e-6, dtype=dtype, device=dev), h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1. / float(self.order))
        h1 = h1.abs()
        return torch.min(100 * h0, h1).to(t_dtype)

    def _optimal_step_size(self, last_step, error_ratio):
        if error_ratio == 0:
            return last_step * self.ifactor
        dfactor = self.dfactor
        if error_ratio < 1:
            dfactor = torch.ones((), dtype=last_step.dtype, device=last_step.device)
        error_ratio = error_ratio.type_as(last_step)
        exponent = torch.tensor(self.order, dtype=last_step.dtype, device=last_step.device).reciprocal()
        factor = torch.min(self.ifactor, torch.max(self.safety / error_ratio ** exponent, dfactor))
        return last_step * factor

    def _step(self, y0, f0, t0, dt):
        dtf = float(dt.detach()) if isinstance(dt, torch.Tensor) else float(dt)
        t0f = float(t0.detach()) if isinstance(t0, torch.Tensor) else float(t0)
        k = [f0]
        yi = y0
        for i, (a_i, beta_i) in enumerate(zip(self.alpha, self.beta)):
            ti = t0f + dtf if a_i == 1. else t0f + a_i * dtf
            yi = self.combine(y0, k, beta_i, dtf)
            k.append(self.func(ti, yi))
        # non-FSAL tableaus (adaptive_heun, fehlberg2): y1 from c_sol, while the next
        # step's f0 is still the last stage k[-1], exactly as torchdiffeq does
        y1 = yi if self.fsal else self.combine(y0, k, self.c_sol, dtf)
        f1 = k[-1]
        y1_error = self.combine(None, k, self.c_error, dtf)
        return y1, f1, y1_error, k

    def _interp(self, y0, y1, k, dt, t0, t1, t):
        dtf = float(dt.detach()) if isinstance(dt, torch.Tensor) else float(dt)
        y_mid = self.combine(y0, k, self.c_mid, dtf)
        f0, f1 = k[0], k[-1]
        a = 2 * dtf * (f1 - f0) - 8 * (y1 + y0) + 16 * y_mid
        b = dtf * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * y_mid
        c = dtf * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * y_mid
        d = dtf * f0
        e = y0
        x = (t - t0) / (t1 - t0)
        x = float(x.detach()) if isinstance(x, torch.Tensor) else float(x)
        total = e + x * d
        xp = x
        for coeff in (c, b, a):
            xp = xp * x
            total = total + xp * coeff
        return total

    def integrate(self, t):
        t = t.to(self.dtype)
        solution = [self.y0]
        t0 = t[0]
        f0 = self.func(t0, self.y0)
        dt = self._select_initial_step(t0, f0) if self.first_step is None else self.first_step
        y, f = self.y0, f0
        t_prev, t_cur = t0, t0
        last = None  # (y_prev, y_cur, k, dt) of the last accepted step
        for i in range(1, len(t)):
            next_t = t[i]
            while next_t > t_cur:
                if self.max_attempts is not None and self.n_steps >= self.max_attempts:
                    self.capped = True
                    break
                check_step(t_cur, dt, self.n_steps, self.max_num_steps)
                y1, f1, y1_err, k = self._step(y, f, t_cur, dt)
                error_tol = self.atol + self.rtol * torch.max(y.abs(), y1.abs())
                error_ratio = self.norm(y1_err / error_tol).abs()
                if error_ratio <= 1:
                    last = (y, y1, k, dt)
                    t_prev, t_cur = t_cur, t_cur + dt
                    y, f = y1, f1
                    if self.accept_hook is not None:
                        self.accept_hook(y, float(t_cur), None)
                dt = self._optimal_step_size(dt, error_ratio)
                self.n_steps += 1
            if self.capped or last is None or next_t == t_cur:
                solution.append(y)
            else:
                y_prev, y_cur, k, dts = last
                solution.append(self._interp(y_prev, y_cur, k, dts, t_prev, t_cur, next_t))
        return torch.stack(solution, 0)


KRYLOV_STEP = os.environ.get('GNPDE_KRYLOV_STEP', '1') != '0'
# The dense output of a one-output-time Krylov solve folded into its steps' last launch
# (ABI 8 Stage.dense; GNPDE_DENSE_FOLD=0: the separate pass of _interp_into)
DENSE_FOLD = os.environ.get('GNPDE_DENSE_FOLD', '1') != '0'
# The initial-step selection of an affine RHS from row sums the f0 and probe launches form
# (ABI 8 scale_rows, err_y1 = -2, gnpde_initial_step_rows; GNPDE_INIT_ROWS=0: the passes of
# gnpde_initial_step_f32 over y0, f0 and f1 = f(y0 + h0 f0), in torch's fp32 arithmetic).
# Off by default: the wide epilogue the two launches then take costs more than the passes
# it saves (G-arxiv: f0 launch 80 -> 124 us, probe 76 -> 109 us)
INIT_ROWS = os.environ.get('GNPDE_INIT_ROWS', '0') == '1'
# The initial-step probe of an affine Krylov solve as v = L f0 (gnpde_initial_step_lin_*: d2 =
# rms(v / scale)), run beside the phase-0 reduction on a second stream; v is the first step's
# u_1 / dt, so that step scales it in place instead of launching K1 (GNPDE_LIN_INIT=0: the probe
# f0 + h0 L f0 after phase 0 and a first step like the others)
LIN_INIT = os.environ.get('GNPDE_LIN_INIT', '1') != '0'
# The f0 launch and the lin_init initial step replayed as one captured graph once warm
# (GNPDE_PROLOGUE_GRAPH=1).  Off by default: measured no faster (G-arxiv 2.705 against 2.698 ms
# per solve) — once the first launch runs, the host stays ahead of the device anyway.
PROLOGUE_GRAPH = os.environ.get('GNPDE_PROLOGUE_GRAPH', '0') == '1'


def _fused_adaptive_ok(func, y0, combine, options):
    """The fused adaptive step applies: a gnpde RHS (rhs_stage) without autograd, a
    device state (or a host-stage test RHS on CPU), torchdiffeq's RMS norm (or a
    sharded RHS's global one, reduced through func.reduce_error_sq)."""
    if not (isinstance(combine, _Combine) and hasattr(func, 'rhs_stage')) or torch.is_grad_enabled():
        return False
    if not getattr(func, 'fused_adaptive', True) or os.environ.get('GNPDE_FUSED_ADAPTIVE', '1') == '0':
        return False
    norm = options.get('norm')
    if norm is not None and not (getattr(norm, '__self__', None) is func and hasattr(func, 'reduce_error_sq')):
        return False
    if y0.is_cuda:
        return y0.dtype in ops.STATE_DTYPES
    return bool(getattr(func, 'host_stages', False)) and hasattr(func, 'host_stage_apply')


# Backprop through adaptive solves of the Laplacian (gnpde.adaptive_backprop; GNPDE_ADAPTIVE_BACKPROP=0: the
# restated loop with autograd through every RHS and stage combination)
ADAPTIVE_BACKPROP = os.environ.get('GNPDE_ADAPTIVE_BACKPROP', '1') != '0'


def _adaptive_backprop_ok(func, y0, combine, options):
    """An adaptive solve under autograd of a gnpde LaplacianODEFunc on a device fp32
    state with torchdiffeq's RMS norm, the sigmoid alpha and something to differentiate."""
    if not (ADAPTIVE_BACKPROP and torch.is_grad_enabled() and isinstance(combine, _Combine)):
        return False
    if not (hasattr(func, '_weights_tensor') and hasattr(func, 'rhs_stage')) or 'norm' in options:
        return False
    if not (y0.is_cuda and y0.dtype == torch.float32 and y0.dim() == 3) or getattr(func, '_layout', None) is not None:
        return False
    if func.opt.get('no_alpha_sigmoid', False):
        return False
    w, _ = func._weights_tensor()
    return any(v.requires_grad for v in (y0, func.alpha_train, func.beta_train, w))


class _LaplacianAdaptiveFn(torch.autograd.Function):
    """An adaptive solve of f(y) = sigma(alpha)(A(w) y - y) [+ beta x0] with its discrete
    adjoint (gnpde.adaptive_backprop): gradients to y0, alpha_train, beta_train and the
    weights (the attention an AttODEblock hands the Laplacian)."""

    @staticmethod
    def forward(ctx, y0, alpha_train, beta_train, w, func, t_h, method, rtol, atol, first_step, max_num_steps):
        with torch.no_grad():
            solver = AdaptiveBackprop(func, y0.detach(), t_h, method, rtol, atol, first_step, max_num_steps)
            sol = solver.forward()
            # everything the backward reads is taken NOW, after the forward launches are queued (as
            # _LaplacianFixedGridFn.forward): another forward, a new graph, weights or x0, or a no_grad
            # solve refreshing the module's cached buffers before this backward must not change its gradient
            ctx.o = laplacian_operands(func, solver.y0, snapshot=True)
        odeint.last_n_steps = solver.n_steps
        ctx.solver = solver
        ctx.save_for_backward(w, alpha_train, beta_train)  # an in-place edit before the backward is autograd's error
        return sol

    @staticmethod
    def backward(ctx, g):
        if ctx.solver is None:
            raise RuntimeError("gnpde: the adaptive backprop node's buffers (every accepted step's stage inputs) "
                               "were released after its first backward; run the forward again")
        w, alpha_train, beta_train = ctx.saved_tensors
        with torch.no_grad():
            ybar, ga, gb, gw = ctx.solver.backward(g, ctx.o, w)
        ctx.solver = ctx.o = None  # frees every stored stage input
        need = ctx.needs_input_grad
        gy = ybar.view(g.shape[1:]) if need[0] else None
        gal, gbe = (param_grads([p], [(alpha_train, ga), (beta_train, gb)])[0] if n else None
                    for p, n in zip((alpha_train, beta_train), need[1:3]))
        gwo = gw if need[3] else None
        return (gy, gal, gbe, gwo) + (None,) * 7


class _HostRecord(object):
    """A pinned host copy of a step's device record that its step graph writes."""
    __slots__ = ('buf',)

    def __init__(self, buf):
        self.buf = buf


# The replayed step graph copies the controller's record to pinned memory itself
# (GNPDE_GRAPH_RECORD_COPY=0: a copy enqueued behind each replay)
GRAPH_RECORD_COPY = os.environ.get('GNPDE_GRAPH_RECORD_COPY', '1') != '0'


# Captured adaptive steps (hipGraph): one graph per (buffer binding, dense-output
# variant) replays a whole step — the stage-input pass, the RHS launches and the
# error reduction — whatever dt (the coefficients scale by a device scalar), so a
# step costs one graph launch and one host read.  GNPDE_ADAPTIVE_GRAPH=0 runs
# every step eagerly.
ADAPTIVE_GRAPH = os.environ.get('GNPDE_ADAPTIVE_GRAPH', '1') != '0'
AFFINE_STAGE = os.environ.get('GNPDE_AFFINE_STAGE', '1') != '0'
ADAPTIVE_SPEC = os.environ.get('GNPDE_ADAPTIVE_SPEC', '1') != '0'  # steps enqueued ahead (_integrate)
_ADAPTIVE_CACHE = weakref.WeakKeyDictionary()  # module -> (key, _AdaptiveState)


class _RKAdaptiveFused(_RKAdaptive):
    """_RKAdaptive with the step formed by the RHS epilogues (_AdaptivePlan): the same
    controller (torchdiffeq's, in host float64 arithmetic), the same accepted /
    rejected sequence, dense output from the stored stage derivatives.  Per step:
    one stage-input pass, len(alpha) RHS launches carrying the combinations and the
    error rows, one fixed-order fp64 reduction and one host read of it; the step
    replayed from a captured hipGraph once the module's structures are built."""

    def __init__(self, func, y0, rtol, atol, combine, method='dopri5', options=None, **kw):
        super(_RKAdaptiveFused, self).__init__(func, y0, rtol, atol, combine, method=method, **kw)
        self.options = dict(options or {})
        self.plan = _adaptive_plan(method)
        self.host = not y0.is_cuda
        self.rtol_f, self.atol_f = float(rtol), float(atol)
        # f(y) = L y + s (func.affine): the step's first stage derivative is k0 + dt b00 L k0 from
        # a launch over k0 (Stage.f_lin) — no X0 = y0 + dt b00 k0 pass.  Needs k0 = f(y0): the FSAL
        # pairs (dopri5, bosh3); torchdiffeq's non-FSAL pairs carry k0 = the last stage of the previous
        # step instead.  GNPDE_AFFINE_STAGE=0 disables it.
        self.affine = bool(getattr(func, 'affine', False)) and AFFINE_STAGE and self.plan.fsal
        # the affine step in the Krylov basis (_KrylovPlan): ns launches, no stage operands
        # before the last; its u_1 .. u_{ns-1} live in the K1 .. K{ns-1} buffers
        P = self.plan
        self.krylov = None
        if self.affine and KRYLOV_STEP and P.ns <= _lib.STAGE_MAX_K and \
                set(range(1, P.ns + 1)) <= (P.store | P.store_mid):
            self.krylov = _krylov_plan(P)
        sc = self._scalars
        self.safety_f, self.ifactor_f, self.dfactor_f = float(sc['safety']), float(sc['ifactor']), float(sc['dfactor'])
        self.fold = False  # this solve's dense output folded into the Krylov steps (_integrate)
        self.init_rows = False  # its initial step from the f0 / probe launches' row sums (_integrate)
        self.lin_init = False   # its probe v = L f0, reused as the first step's u_1 (_integrate)
        self._first = False     # the next step is the first attempt after a lin_init probe
        self.lay = None

    # ---- device primitives (host-stage RHS objects supply CPU versions: tests only)
    def _apply(self, stage, f, x, like):
        if self.host:
            self.func.host_stage_apply(stage, f, x, like)
        else:
            ops.stage_apply(stage, f, x, like)

    def _err_sum(self, rows):
        """The step's squared error sum (0-d fp64 tensor) and its element count."""
        v = rows.sum() if self.host else ops.sum_f64(rows)
        n = float(rows.numel() * self.C)
        red = getattr(self.func, 'reduce_error_sq', None)
        if red is not None and 'norm' in self.options:
            pair = torch.stack([v.reshape(()), torch.tensor(n, dtype=torch.float64, device=rows.device)])
            red(pair)
            return pair
        return v

    def _launch(self, i, st, x, t, mid):
        P = self.plan
        bufs = st.bufs
        lin = self.affine and i == 0
        if lin:
            # the affine first stage: the launch reads k0 and forms k1 = k0 + dt b00 L k0 (Stage.f_lin),
            # never X0 = y0 + dt b00 k0; its combinations on X0 are restated on y0 (X0 = y0 + dt b00 k0)
            x = bufs['K0']
        # (the k and f coefficients are the tableau's, scaled by dt on the device: Stage.scale)
        outs, err, err_y1, store = P.launch(i, mid, lambda s: x if s == 'X' else bufs[s],
                                            restate=self._on_y0 if lin else None)
        if err is not None:
            if lin and err_y1 < 0:
                raise RuntimeError("gnpde: an affine one-stage tableau needs its y1 output for the tolerance")
            err = (st.rows, err, bufs['Y'], err_y1, self.atol_f, self.rtol_f)
        f_out = bufs['K%d' % (i + 1)] if store else None
        if lin:
            self.func.rhs_stage(t, x, ops.Stage(f_out=f_out, outs=outs, err=err, scale=st.scale,
                                                f_lin=P.beta[0][0]), linear=True)
        else:
            self.func.rhs_stage(t, x, ops.Stage(f_out=f_out, outs=outs, err=err, scale=st.scale))

    def _on_y0(self, spec):
        """A launch-0 combination on base X0 restated on y0: X0 + dt(sum d_j k_j + cf f)
        = y0 + dt((b00 + d_0) k0 + ...) (X0 = y0 + dt b00 k0)."""
        base, terms, cf = spec
        if base != 'X':
            return spec
        b00 = self.plan.beta[0][0]
        d = dict(terms)
        d['K0'] = d.get('K0', 0.0) + b00
        return ('Y', [(k, c) for k, c in d.items() if c != 0.0], cf)

    def _step(self, st, t_cur, dt, mid, first=False):
        """Enqueue one step (stage-input pass, RHS launches, error reduction); returns
        the device error sum."""
        P = self.plan
        bufs = st.bufs
        if self.krylov is not None:
            self._krylov_launches(st, t_cur, first)
        else:
            if not self.affine:  # the first stage input X0 = y0 + dt b00 k0 (the affine mode never forms it)
                self._apply(ops.Stage(outs=[(bufs['X0'], bufs['Y'], 1.0, 0.0, [(bufs['K0'], P.beta[0][0])])],
                                      scale=st.scale), None, None, bufs['Y'])
            for i in range(P.ns):
                ti = t_cur + dt if P.alpha[i] == 1. else t_cur + P.alpha[i] * dt
                self._launch(i, st, bufs['X%d' % i], ti, mid)
        if self._dev_control():  # the error sum and the controller: two launches, no host work
            ops.adaptive_control(st.rows, st.rows.numel() * self.C, self.order, self.safety_f, self.ifactor_f,
                                 self.dfactor_f, st.dt, st.scale, st.rec, ws=st.ws, t=st.tdev)
            return st.rec
        return self._err_sum(st.rows)

    def _krylov_launches(self, st, t, first=False):
        """The launches of one affine step in the Krylov basis (_KrylovPlan): u_{p+1} =
        dt L u_p into K{p+1} for p < ns - 1, then the launch over u_{ns-1} that writes y1,
        f1 (K{ns}) and the error rows.  The RHS is autonomous: every launch at t."""
        K = self.krylov
        ns = K.ns
        bufs = st.bufs
        u = [bufs['K0']] + [bufs['K%d' % p] for p in range(1, ns)]
        y1t, (ft, fcf), (et, ecf) = K.last_launch_terms()
        outs = [(bufs['Y1'], bufs['Y'], 1.0, 0.0, [(u[p], c) for p, c in y1t]),
                (bufs['K%d' % ns], None, 0.0, fcf, [(u[p], c) for p, c in ft])]
        err = (st.rows, (None, 0.0, ecf, [(u[p], c) for p, c in et]), bufs['Y'], 0, self.atol_f, self.rtol_f)
        last = ops.Stage(outs=outs, err=err, scale=st.scale, f_lin=1.0, unscaled=(1,))
        # the first attempt after a lin_init probe: u_1 = dt v in place (v = L f0 in K1, the same
        # fp32 product the launch over u_0 would store), the K1 launches from u_1 on
        p0 = 1 if first else 0
        if first:
            if hasattr(self.func, 'nfe'):  # the reference evaluates it: the counter keeps torchdiffeq's NFE
                self.func.nfe += 1
            ops.stage_apply(ops.Stage(outs=[(u[1], None, 0.0, 0.0, [(u[1], 1.0)])], scale=st.scale), None, None,
                            u[1])
        form = None  # the folded dense output: the step's first launch forms its coefficients, the last applies them
        if self.fold and ns >= 2:
            last.dense = (st.dslot, st.drows if self.lay is not None else None, None, None, st.dtab,
                          self._dense_table(u, ft, fcf))
            form = (None, None, st.tdev, st.dt, st.dtab, last.dense_matrix())
        for p in range(p0, ns - 1):
            self.func.rhs_stage(t, u[p], ops.Stage(outs=[(u[p + 1], None, 0.0, 1.0, [])], scale=st.scale,
                                                   dense=form if p == p0 else None), linear=True)
        self.func.rhs_stage(t, u[ns - 1], last, linear=True)

    def _dense_table(self, u, ft, fcf):
        """The basis coefficients of the step's dense output over the last Krylov launch's
        operands (ABI 8 Stage.dense): with w = (cy0 + cy1 + cym, h cy1, h cym, cf0, cf1),
        out = w0 y0 + sum_p [w1 G[p] + w2 (Mu[p] + c_mid[ns] f1_p) + w3 [p = 0] + w4 f1_p] u_p
              + (w2 c_mid[ns] + w4) fcf f'
        where f1 = sum_p f1_p u_p + fcf f' is the next step's f0 (u_ns substituted) — the
        combination _interp_into forms from y0, the u_p and f1 in a pass of its own."""
        K, P = self.krylov, self.plan
        ns = K.ns
        cm = P.c_mid[ns]
        f1 = dict(ft)
        table = {'base': [1.0, 0.0, 0.0, 0.0, 0.0], 'f': [0.0, 0.0, cm * fcf, 0.0, fcf]}
        for p in range(ns):
            b = f1.get(p, 0.0)
            w = [0.0, K.G[p], K.Mu[p] + cm * b, 1.0 if p == 0 else 0.0, b]
            if any(v != 0.0 for v in w):
                table[u[p]] = w
        return table

    def _dev_control(self):
        """The step-size controller runs on the device (a device solve with the
        default RMS norm): the host reads {ratio, dt, next dt} once per step."""
        return not self.host and 'norm' not in self.options

    def _rec_reader(self, st, rec, slot=None):
        """A device fp64 record (the step's {ratio, dt, next dt, e2}; h of the initial
        step, slot 2) copied to pinned host memory behind an event (slots 0 / 1
        alternate: a step ahead may be in flight): a callable that waits for that copy
        only and returns the values."""
        if isinstance(rec, _HostRecord):  # copied by the replayed step graph itself
            ev = torch.cuda.Event()
            ev.record()
            hb = rec.buf

            def read_graph():
                ev.synchronize()
                return hb.tolist()
            return read_graph
        if st.rec_host is None:
            st.rec_host = torch.empty((3, 4), dtype=torch.float64, pin_memory=True)
        if slot is None:
            slot = st.rec_slot
            st.rec_slot ^= 1
        h = st.rec_host[slot, :rec.numel()]
        h.copy_(rec, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()

        def read():
            ev.synchronize()
            return h.tolist()
        return read

    def _lin_init_launches(self, st, t0):
        """The lin_init initial step: phase 0 (y0, f0 -> h0, d1) on a second stream beside the
        probe v = L f0 (it needs no h0), then phase 1 from v; v lands in K1, the first step's
        u_1 buffer (_krylov_launches).  No host read (capturable: _prologue)."""
        bufs = st.bufs
        Y, K0, v = bufs['Y'], bufs['K0'], bufs['K1']
        h, hf = st.h, st.scale
        if st.iws0 is None:
            nb = _lib.fn("gnpde_initial_step_workspace_bytes")()
            st.iws0 = torch.empty(nb, dtype=torch.uint8, device=Y.device)
            st.iws1 = torch.empty(nb, dtype=torch.uint8, device=Y.device)
        main = torch.cuda.current_stream(Y.device)
        if st.side is None:
            st.side = torch.cuda.Stream(Y.device)
        st.side.wait_stream(main)
        with torch.cuda.stream(st.side):
            ops.initial_step(Y, K0, None, self.atol_f, self.rtol_f, self.order, h, hf, ws=st.iws0)
        self.func.rhs_stage(t0, K0, ops.Stage(f_out=v), linear=True)
        main.wait_stream(st.side)
        ops.initial_step_lin(Y, v, self.atol_f, self.rtol_f, self.order, h, hf, ws=st.iws1)

    def _prologue(self, st, graphs_ok, t0):
        """f0 into K0 and the lin_init initial step as ONE captured graph (PROLOGUE_GRAPH) once
        the module is warm.  Returns True when replayed (the caller reads h)."""
        if not (PROLOGUE_GRAPH and graphs_ok and st.warm and _nfe_headroom(self.func, 2)):
            return False
        bufs = st.bufs
        if st.pro is None:
            nfe = getattr(self.func, 'nfe', None)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=st.mempool):
                self.func.rhs_stage(t0, bufs['Y'], ops.Stage(f_out=bufs['K0']))
                self._lin_init_launches(st, t0)
            if st.mempool is None:
                st.mempool = g.pool()
            if nfe is not None:
                self.func.nfe = nfe  # capture records launches, it evaluates nothing
            st.pro = g
        st.pro.replay()
        if hasattr(self.func, 'nfe'):
            self.func.nfe += 2
        self._first = True
        return True

    def _initial_step_device(self, st, t0):
        """_select_initial_step on the device (gnpde_initial_step_*: the two fixed-order
        norm reductions and the scalar rules in HIP, the probe y0 + h0 f0 as one stage
        pass with h0 as its device coefficient scale, f1 by the RHS): one host read.
        The probe's RHS is evaluated at t0 (the RHS is autonomous: h0 stays on the
        device)."""
        bufs = st.bufs
        Y, K0 = bufs['Y'], bufs['K0']
        h, hf = st.h, st.scale  # h[2] is st.dt: the device controller starts from it
        if self.lin_init:
            self._lin_init_launches(st, t0)
            self._first = True
            return self._rec_reader(st, h, slot=2)
        if self.init_rows:
            # from the f0 launch's rows; then the rows of L f0 (the probe's linear part on f0, no
            # output): d2 = rms(L f0 / scale) = rms((f1 - f0) / scale) / h0 for f1 = f(y0 + h0 f0)
            n = float(st.rows.numel() * self.C)
            ops.initial_step_rows(st.rows, st.rows2, n, self.order, h, hf, ws=st.iws)
            self.func.rhs_stage(t0, K0, ops.Stage(err=(st.rows, (None, 0.0, 1.0, []), Y, -2, self.atol_f,
                                                       self.rtol_f)), linear=True)
            ops.initial_step_rows(st.rows, None, n, self.order, h, hf, ws=st.iws)
            return self._rec_reader(st, h, slot=2)
        ops.initial_step(Y, K0, None, self.atol_f, self.rtol_f, self.order, h, hf)
        probe, f1 = bufs['X0'], bufs['Y1']  # free until the first step
        if self.affine:  # f1 = f0 + h0 L f0 from a launch over f0 (no probe pass)
            self.func.rhs_stage(t0, K0, ops.Stage(f_out=f1, scale=hf, f_lin=1.0), linear=True)
        else:
            ops.stage_apply(ops.Stage(outs=[(probe, Y, 1.0, 0.0, [(K0, 1.0)])], scale=hf), None, None, Y)
            self.func.rhs_stage(t0, probe, ops.Stage(f_out=f1))
        ops.initial_step(Y, K0, f1, self.atol_f, self.rtol_f, self.order, h, hf)
        return self._rec_reader(st, h, slot=2)  # the first step's size: read when it is needed

    def _state(self, y0):
        """The module's cached buffers / graphs for this shape, tolerance and graph
        state (a new entry when any of them changed)."""
        P = self.plan
        if self.host or not ADAPTIVE_GRAPH or not _replayable(self.func) or \
                'norm' in self.options:  # a sharded RHS's global norm: a collective inside the step
            return _AdaptiveState(P, y0, self.host), False
        state = _capture_state(self.func, y0)
        key = _graph_cache_key(self.func, 'adaptive:' + P.method + (':krylov' if self.krylov is not None else ''), y0, state)
        if key is None:
            return _AdaptiveState(P, y0, self.host), False
        key = key + (self.atol_f, self.rtol_f, torch.cuda.current_stream(y0.device).cuda_stream,
                     'norm' in self.options)
        hit = _ADAPTIVE_CACHE.get(self.func)
        if hit is not None and hit[0] == key:
            return hit[1], True
        ast = _AdaptiveState(P, y0, self.host)
        _ADAPTIVE_CACHE[self.func] = (key, ast, state)
        return ast, True

    def _run_step(self, st, graphs_ok, t_cur, dt, mid):
        """One step: replayed from its graph when the binding's graph exists (captured
        on first use once the module is warm), eagerly otherwise.  The first attempt after
        a lin_init probe takes its own variant (u_1 from the probe)."""
        P = self.plan
        first, self._first = self._first, False
        if graphs_ok and st.warm and _nfe_headroom(self.func, P.ns):
            gk = (id(st.bufs['Y']), id(st.bufs['K0']), bool(mid), self.fold, self.lay is not None, GRAPH_RECORD_COPY,
                  first)
            ent = st.graphs.get(gk)
            if ent is None:
                nfe = getattr(self.func, 'nfe', None)
                g = torch.cuda.CUDAGraph()
                # the device controller's record copied to a pinned buffer of this graph by the graph
                # itself (GRAPH_RECORD_COPY): no separate copy behind the replay (the same graph is
                # replayed again only after its record was read: the bindings rotate through three)
                hb = torch.empty(4, dtype=torch.float64, pin_memory=True) \
                    if (GRAPH_RECORD_COPY and self._dev_control()) else None
                with torch.cuda.graph(g, pool=st.mempool):
                    err = self._step(st, t_cur, dt, mid, first)
                    if hb is not None:
                        hb.copy_(err, non_blocking=True)
                if st.mempool is None:
                    st.mempool = g.pool()
                if nfe is not None:
                    self.func.nfe = nfe  # capture records launches, it evaluates nothing
                ent = (g, err if hb is None else _HostRecord(hb))
                st.graphs[gk] = ent
            ent[0].replay()
            if hasattr(self.func, 'nfe'):
                self.func.nfe += P.ns
            return ent[1]
        err = self._step(st, t_cur, dt, mid, first)
        st.warm = True
        return err

    def integrate(self, t):
        """The adaptive loop.  A device solve of a module offering a locality numbering
        (ops.NodeLayout, as the fixed-grid path) runs in it: the entry pass writes
        sol[0] and the permuted state from one read of y0, every RHS launch gathers
        from the degree-ordered rows, and outputs return to the caller's numbering
        (the dense output's single pass stores there directly, out_rows).  Row
        values are bit-identical to the user numbering; the error norm's fixed-order
        sum runs over rows in the other order (fp64 rounding only)."""
        P = self.plan
        th = _host_times(t)  # cached per time tensor: no device read for an ODEblock's self.t
        y0 = self.y0.contiguous()
        self.C = y0.shape[-1]
        dev = y0.device
        sol = torch.empty((len(th),) + tuple(y0.shape), dtype=y0.dtype, device=dev)
        lay = None if self.host else _node_layout(self.func, y0)
        self.lay = lay
        if lay is not None:
            self.func._layout = lay
        try:
            return self._integrate(th, y0, sol, lay)
        finally:
            if lay is not None:
                self.func._layout = None

    def _integrate(self, th, y0, sol, lay):
        P = self.plan
        dev = y0.device
        st, graphs_ok = self._state(y0)
        bufs = st.bufs
        if st.canon is not None:
            # every solve starts from the same binding of the rotating y / f0 buffers, so it walks
            # the same sequence of bindings and replays the same step graphs (a solve starting
            # where the last one ended met bindings whose graphs were not captured yet)
            bufs.update(st.canon)
        # The dense output folded into the last launch of every step (DENSE_FOLD; ABI 8): a
        # solve to one output time in the Krylov basis under the device controller.  Each
        # step's launch writes the interpolant at th[1] straight into sol[1] (the caller's
        # numbering) when the step crosses it, by the device time the controller advances;
        # the accepted crossing step writes last (a rejected or discarded step either does
        # not cross or is followed by one that does), so no dense-output pass follows.
        self.fold = (DENSE_FOLD and not self.host and self.krylov is not None and self.krylov.ns >= 2 and
                     self._dev_control() and
                     len(th) == 2 and th[1] > th[0] and getattr(self.func, 'fold_dense', False))
        if not self.host:
            hv = st.dsc_np
            hv[0], hv[1] = th[0], th[-1]
            hv[2:].view(np.int64)[0] = sol[1].data_ptr() if self.fold else 0
            st.dsc.copy_(st.dsc_host, non_blocking=True)
        if self.fold:
            if lay is not None and st.drows_src is not lay.order32:
                if st.drows is None:
                    st.drows = torch.empty_like(lay.order32)
                st.drows.copy_(lay.order32)
                st.drows_src = lay.order32
        if self.host:
            sol[0].copy_(y0)
            bufs['Y'].copy_(y0)
        else:
            _entry_copy(y0, bufs['Y'], sol[0], lay.order if lay is not None else None)
        t0 = torch.tensor(th[0], dtype=torch.float64)
        dev_init = not self.host and getattr(self.func, 'autonomous', False) and 'norm' not in self.options
        # the initial-step selection's squared sums formed by the f0 and probe launches themselves
        # (an affine RHS: the probe is the linear part on f0), no passes over y0, f0, f1
        self.init_rows = (INIT_ROWS and dev_init and self.affine and self._scalars['first_step'] is None)
        self.lin_init = (LIN_INIT and not self.init_rows and dev_init and self.krylov is not None and
                         self.krylov.ns >= 3 and self._scalars['first_step'] is None)
        dt_read = None  # the device initial step's reader: the first step is enqueued before it is read
        if self.init_rows:
            if st.rows2 is None:
                st.rows2 = torch.empty_like(st.rows)
                st.iws = torch.empty(_lib.fn("gnpde_initial_step_workspace_bytes")(), dtype=torch.uint8,
                                     device=dev)
            # f0 into K0 with the rows sum (f0 / scale)^2 (err) and sum (y0 / scale)^2 (scale_rows),
            # scale = atol + rtol |y0| (err_y1 = -2)
            self.func.rhs_stage(t0, bufs['Y'], ops.Stage(
                f_out=bufs['K0'], err=(st.rows, (None, 0.0, 1.0, []), bufs['Y'], -2, self.atol_f, self.rtol_f),
                scale_rows=st.rows2))
        elif dev_init and self.lin_init and self._prologue(st, graphs_ok, t0):
            dt_read = self._rec_reader(st, st.h, slot=2)  # f0 and the initial step replayed
        elif dev_init:  # f0 straight into K0 (the RHS epilogue's f_out)
            self.func.rhs_stage(t0, bufs['Y'], ops.Stage(f_out=bufs['K0']))
        else:
            f0 = self.func(t0, bufs['Y'])
            bufs['K0'].copy_(f0)
        dt_on_device = False
        if self._scalars['first_step'] is None:
            if dev_init:
                if dt_read is None:
                    dt_read = self._initial_step_device(st, t0)
                dt = None
                dt_on_device = True  # st.dt and st.scale hold it already
            else:
                dt = float(self._select_initial_step(t0.to(dev) if not self.host else t0, bufs['K0']))
        else:
            dt = float(self._scalars['first_step'])
        t_cur = th[0]
        last = None  # (t_prev, dt) of the last accepted step
        self._dense = None
        dev_ctl = self._dev_control()
        if dev_ctl and not dt_on_device:  # the device controller carries dt (and the scale) from step to step
            st.dt.fill_(dt)
            st.scale.fill_(dt)
        # Steps enqueued ahead (ADAPTIVE_SPEC): while the host waits for step n's record, step
        # n+1 already runs on the binding an acceptance gives, from the device controller's dt.
        # A third y / f0 buffer keeps step n's inputs intact, so a rejection only discards the
        # step ahead (its RHS evaluations are not counted) and restores dt on the device.
        # In this mode every step keeps its dense-output k's (one variant per binding, so a
        # solve replays three captured graphs): whether a step crosses an output time is
        # known only once its dt is read.
        spec_ok = dev_ctl and graphs_ok and ADAPTIVE_SPEC and P.fsal
        if spec_ok and 'Ys' not in bufs:
            bufs['Ys'], bufs['Ks'] = torch.empty_like(bufs['Y']), torch.empty_like(bufs['K0'])
        if st.canon is None or len(st.canon) < len(bufs):  # (no step has rotated them in this solve yet)
            st.canon = dict(bufs)
        pending = None  # the record reader of the step enqueued ahead: the current step
        pre_interp = None  # (output index, t0, dt) of a dense output enqueued ahead of its step's record
        if dt_read is not None:
            if spec_ok and th[-1] > th[0]:  # the first step runs while the host waits for its size
                pending = self._rec_reader(st, self._run_step(st, graphs_ok, t_cur, 0.0, True))
            dt = dt_read()[2]
        cap, hook = self.max_attempts, self.accept_hook
        for i_out in range(1, len(th)):
            next_t = th[i_out]
            while next_t > t_cur:
                if cap is not None and self.n_steps >= cap:
                    self.capped = True
                    break
                check_step(t_cur, dt, self.n_steps, self.max_num_steps)
                mid = t_cur + dt >= next_t  # an accepted step would cross an output time: keep the dense-output k's
                if pending is not None:
                    read, pending = pending, None
                else:
                    if not dev_ctl:
                        st.scale.fill_(dt)
                    err = self._run_step(st, graphs_ok, t_cur, dt, mid or spec_ok)
                    read = self._rec_reader(st, err) if dev_ctl else None
                ahead = None
                # ahead only after a step whose k's the dense output does not need (the step ahead
                # overwrites them); it keeps its own (mid variant: its dt is not known yet)
                if spec_ok and st.warm and not mid and self.n_steps + 1 < self.max_num_steps and \
                        (cap is None or self.n_steps + 1 < cap) and _nfe_headroom(self.func, 2 * P.ns):
                    rotate(bufs, P, 1)
                    ahead = self._rec_reader(st, self._run_step(st, graphs_ok, t_cur + dt, dt, True))
                # the step crossing next_t (steps-ahead mode, its k's kept): its dense output is
                # enqueued before its record is read, so the pass follows the step on the device
                # without the host's round trip; used if the step is accepted (a rejected step's
                # successor writes the output again)
                if spec_ok and mid and ahead is None and t_cur + dt > next_t and not self.fold:
                    self._dense = dict(bufs, scale=dt)
                    self._interp_into(sol[i_out], (t_cur, dt), next_t, t_cur + dt, lay)
                    pre_interp = (i_out, t_cur, dt)
                dt_next = None
                if dev_ctl:
                    ratio, _dt, dt_next, _e2 = read()  # the one host read of the step
                elif err.dim() == 0:
                    ratio = math.sqrt(float(err) / (y0.numel()))  # the one host read of the step
                else:
                    e2, n = (float(v) for v in err.tolist())
                    ratio = math.sqrt(e2 / n) if n > 0 else 0.0
                if ratio <= 1:
                    t_prev, t_cur = t_cur, t_cur + dt
                    last = (t_prev, dt)
                    # a step that crossed an output time keeps its operands for the dense output (the
                    # references as they are now; the buffers are only rewritten by the next step)
                    self._dense = dict(bufs, scale=dt) if mid else None
                    if ahead is not None:
                        pending = ahead  # already on the accepted binding
                    else:
                        rotate(bufs, P, 1)
                    if hook is not None:
                        # bufs['Y'] holds y1 now; a step enqueued ahead only reads it, and the hook's
                        # launch follows that step on the stream: no copy, no synchronisation
                        hook(bufs['Y'], t_cur, lay)
                elif ahead is not None:  # rejected: discard the step ahead, step n again from its inputs
                    rotate(bufs, P, -1)
                    st.dt.fill_(dt_next)
                    st.scale.fill_(dt_next)
                    st.tdev[0].fill_(t_cur)  # (the discarded step's controller may have advanced it)
                    if hasattr(self.func, 'nfe'):
                        self.func.nfe -= P.ns
                if dt_next is None:  # (the host controller; the device controller's record carries its own)
                    dt_next = next_dt(dt, ratio, float(P.order), self.safety_f, self.ifactor_f, self.dfactor_f)
                dt = dt_next
                self.n_steps += 1
            if self.capped and pending is not None:
                # (a cap below one attempt: the first step, enqueued while its size was read, is dropped)
                pending = None
                if hasattr(self.func, 'nfe'):
                    self.func.nfe -= P.ns
            if next_t == t_cur or last is None or self.capped:
                # (capped: the state at the last accepted t1, written after anything a folded or
                # pre-enqueued dense output of a rejected step left in this slice)
                if self.host:
                    sol[i_out].copy_(bufs['Y'])
                else:
                    _to_user(bufs['Y'], sol[i_out], lay)
            elif pre_interp != (i_out,) + tuple(last) and not self.fold:  # (not already enqueued / folded)
                self._interp_into(sol[i_out], last, next_t, t_cur, lay)
        return sol

    def _interp_into(self, out, last, t, t1, lay=None):
        """torchdiffeq's 4th-order dense output (_interp_fit / _interp_evaluate, with the
        tableau's mid-point coefficients) of the last accepted step at time t:
        y_mid = y0 + dt sum_j c_mid[j] k_j, then the polynomial, a combination of y0,
        y1, y_mid, f0 and f1 — folded into ONE stage pass over y0 (its base), f1 (its
        f input) and the other rows as operands (y_mid substituted), stored in the
        caller's numbering (out_rows); two passes when the operands exceed the
        stage's table."""
        P = self.plan
        t0, dt = last
        d = self._dense
        if d is None:
            raise RuntimeError("gnpde: dense output of a step whose stage derivatives were not kept")
        y_prev, y_cur = d['Y'], d['Y1']
        f0, f1 = d['K0'], d['K%d' % P.ns]
        wts = cy0, cy1, cym, cf0, cf1 = dense_weights((t - t0) / (t1 - t0), dt)
        rows = None if (lay is None or self.host) else lay.order32
        K = self.krylov
        if K is not None:
            # y1 and y_mid restated on the u_p (K0 .. K{ns-1}): one pass over y0, the u_p and f1
            terms = []
            for p in range(P.ns):
                c = cy1 * dt * K.G[p] + cym * dt * K.Mu[p] + (cf0 if p == 0 else 0.0)
                if c != 0.0:
                    terms.append((d['K%d' % p], c))
            self._apply(ops.Stage(outs=[(out, y_prev, cy0 + cy1 + cym, cym * dt * P.c_mid[P.ns] + cf1, terms)],
                                  out_rows=rows), f1, y_prev, y_prev)
            return
        cb, cf_f1, terms = dense_combo(P, wts, dt, y_cur, f0, f1, lambda j: d['K%d' % j])
        if len(terms) <= _lib.STAGE_MAX_K:
            self._apply(ops.Stage(outs=[(out, y_prev, cb, cf_f1, terms)], out_rows=rows), f1, y_prev, y_prev)
            return
        ymid = torch.empty_like(out)
        mterms = [(d['K%d' % j], dt * P.c_mid[j]) for j in range(P.ns + 1) if P.c_mid[j] != 0.0]
        self._apply(ops.Stage(outs=[(ymid, y_prev, 1.0, 0.0, mterms)]), None, None, y_prev)
        self._apply(ops.Stage(outs=[(out, y_prev, cy0, 0.0, [(y_cur, cy1), (ymid, cym), (f0, cf0), (f1, cf1)])],
                              out_rows=rows), None, None, y_prev)


def adaptive_step_graph(func):
    """A captured fused adaptive step of ``func`` (the last solve's cache entry), or
    None: replaying it re-runs one whole step (its launches, the error reduction and
    the device controller) on the buffers it was captured with — the measurement hook
    of bench.py's dopri5 line and tools/pmc_run.py (not part of a solve)."""
    hit = _ADAPTIVE_CACHE.get(func)
    if hit is None or not hit[1].graphs:
        return None
    # a step like most of a solve's: not the first attempt after a lin_init probe (key[-1])
    ents = [e for k, e in hit[1].graphs.items() if not k[-1]] or list(hit[1].graphs.values())
    return ents[0][0]


def odeint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, combine=None):
    """torchdiffeq.odeint(func, y0, t, rtol, atol, method, options) -> [len(t), *y0.shape]."""
    method = method or 'dopri5'
    options = dict(options or {})
    if isinstance(y0, (tuple, list)):  # the regularised RHS's state (gnpde.regularized_ODE_function)
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(t)
        if t.dim() != 1 or len(t) < 2:
            raise ValueError("t must be a 1-D tensor with at least two time points")
        return _odeint_tuple(func, tuple(y0), t, method, options, combine)
    if combine is None:
        if not y0.is_cuda:
            raise RuntimeError("gnpde.odeint: y0 must be a ROCm device tensor (stage combinations run in HIP)")
        combine = _Combine()
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dim() != 1 or len(t) < 2:
        raise ValueError("t must be a 1-D tensor with at least two time points")
    if method in FIXED_METHODS:
        return odeint_fixed(func, y0, t, method, options.get('step_size'), combine, graph=options.get('gnpde_graph'),
                            step_hook=options.get('gnpde_accept_hook'))
    if method in ADAPTIVE_METHODS:
        kw = dict(method=method, first_step=options.get('first_step'),
                  max_num_steps=options.get('max_num_steps', 2 ** 31 - 1), norm=options.get('norm', _rms_norm))
        hooked = options.get('gnpde_accept_hook') is not None or options.get('gnpde_max_attempts') is not None
        if hooked:  # the early-stop integrator (gnpde.early_stop_solver); plain solves pass neither
            kw.update(accept_hook=options.get('gnpde_accept_hook'), max_attempts=options.get('gnpde_max_attempts'))
        if _fused_adaptive_ok(func, y0, combine, options):
            solver = _RKAdaptiveFused(func, y0, rtol, atol, combine, options=options, **kw)
            odeint.last_path = 'fused_krylov' if solver.krylov is not None else 'fused_stage'
        elif not hooked and _adaptive_backprop_ok(func, y0, combine, options):
            # backprop through the adaptive solve of the Laplacian as one node (gnpde.adaptive_backprop)
            w, _ = func._weights_tensor()
            out = _LaplacianAdaptiveFn.apply(y0, func.alpha_train, func.beta_train, w, func, _host_times(t), method,
                                             rtol, atol, options.get('first_step'), kw['max_num_steps'])
            odeint.last_path = 'fused_backprop'
            odeint.last_dense_fold = False
            return out
        else:
            solver = _RKAdaptive(func, y0, rtol, atol, combine, **kw)
            odeint.last_path = 'restated'
        out = solver.integrate(t)
        odeint.last_n_steps = solver.n_steps
        odeint.last_capped = solver.capped
        odeint.last_dense_fold = bool(getattr(solver, 'fold', False))
        return out
    if method in MULTISTEP_METHODS:
        if options.get('gnpde_adams'):
            return odeint_adams(func, y0, t, method, rtol, atol, options, combine)
        raise NotImplementedError("gnpde.odeint: method %r is opt-in: set options['gnpde_adams'] = True "
                                  "(adjoint_options['gnpde_adams'] for the adjoint solve; ODEblock sets both from "
                                  "opt['gnpde_adams'])" % method)
    raise NotImplementedError("gnpde.odeint: method %r not supported (supported: %s)" %
                              (method, ', '.join(FIXED_METHODS + ADAPTIVE_METHODS)))


odeint.last_n_steps = 0
# the last adaptive or multistep solve's loop: 'fused_krylov', 'fused_stage', 'restated', 'adams_fused' or
# 'adams_restated'
odeint.last_path = None
odeint.last_adams = None  # the last multistep solve: per-step corrector 'iterations', 'converged', and 'ratios'
odeint.last_capped = False  # whether it stopped at options['gnpde_max_attempts'] before the output time
odeint.last_dense_fold = False  # whether its dense output was folded into the steps (DENSE_FOLD)
odeint.last_reg_path = None  # the last tuple-state (regularised) solve: 'fused' or 'restated'


# --------------------------------------------------------------------------- adjoint
def _mixed_norm_fn(sizes):
    """torchdiffeq's norm for tuple states (max over the components of their RMS
    norms), applied to the flattened augmented state [y | adj_y | adj_params...]."""
    bounds = []
    o = 0
    for n in sizes:
        bounds.append((o, o + n))
        o += n

    def norm(z):
        return torch.stack([_rms_norm(z[a:b]) for a, b in bounds if b > a]).max()
    return norm


def _laplacian_aug(func, params, y_shape, ny, ans):
    """The augmented RHS of _OdeintAdjoint for the Laplacian (src/function_laplacian_diffusion.py,
    f = sigma(alpha)(A y - y) [+ beta x0]) without autograd: per evaluation two K1 launches
    and at most one dot,
        dy/ds     = -f(y)                          K1 over the CSR, its epilogue storing -f
        da/ds     = L^T a                          K1 over the CSC (L = sigma(alpha)(A - I))
        dalpha/ds = (1 - sigma(alpha)) <L^T a, y>  fp64 row terms in that launch's epilogue
        dbeta/ds  = <a, x0>                        (add_source) one fp64 dot
    written into one output buffer in the packed layout [y | a | params]; the other
    parameters' components are 0.  For the adaptive adjoint methods (torchdiffeq's
    solver loop, the mixed norm); the fixed-grid rk4 adjoint runs _LaplacianAdjointFn.
    None when the RHS is not the HIP Laplacian on a device fp32 state."""
    if not (FUSED_ADJOINT and ans.is_cuda and ans.dtype == torch.float32 and len(y_shape) == 3 and
            laplacian_adjoint_ok(func, params)):
        return None
    o = laplacian_operands(func, ans[0], csr=True, private_csc=True, acc=0, acc_zero=False)
    g, w_csr, w_csc, add_source, x0, alpha, beta, drow = (o.g, o.w_csr, o.w_csc, o.add_source, o.x0, o.alpha, o.beta,
                                                          o.acc)
    slots = {}
    o = 2 * ny
    for p in params:
        slots[id(p)] = (o, p.numel())
        o += p.numel()

    def aug(s, z):
        # one RHS evaluation per augmented one, as torchdiffeq's backward calls func (and its guard)
        if func.nfe > func.opt["max_nfe"]:
            raise MaxNFEException
        func.nfe += 1
        y = z[:ny].view(y_shape)
        a = z[ny:2 * ny].view(y_shape)
        out = torch.empty_like(z)
        ops.spmm_rhs(g, w_csr, y, x0=x0, alpha=alpha, beta=beta, rhs=True, alpha_sigmoid=True,
                     add_source=add_source, stage=ops.Stage(outs=[(out[:ny].view(y_shape), None, 0.0, -1.0, [])]))
        ops.spmm_rhs(g, w_csc, a, alpha=alpha, rhs=True, alpha_sigmoid=True, transpose=True,
                     stage=ops.Stage(outs=[(out[ny:2 * ny].view(y_shape), None, 0.0, 1.0, [])],
                                     dot=(y, drow, 1.0, False)))
        out[2 * ny:].zero_()
        if id(func.alpha_train) in slots:
            oa, _ = slots[id(func.alpha_train)]
            out[oa:oa + 1].copy_(alpha_grad(drow, alpha.double()).reshape(1))
        if add_source and id(func.beta_train) in slots:
            ob, _ = slots[id(func.beta_train)]
            out[ob:ob + 1].copy_(ops.dot(a, x0).reshape(1))
        return out
    return aug


FUSED_ADAPTIVE_ADJOINT = os.environ.get('GNPDE_FUSED_ADAPTIVE_ADJOINT', '1') != '0'


def _adaptive_adjoint_ok(func, ans, a_method, params, a_options):
    """The adaptive adjoint of a Laplacian RHS runs fused (gnpde.adjoint_adaptive): an
    adaptive adjoint method with torchdiffeq's default adjoint norm (no user 'norm'),
    a device fp32 state, weights that are not adjoint parameters, the sigmoid alpha,
    and adjoint parameters among the module's own."""
    if not (FUSED_ADJOINT and FUSED_ADAPTIVE_ADJOINT and a_method in ADAPTIVE_METHODS) or \
            'norm' in (a_options or {}):
        return False
    if not (ans.is_cuda and ans.dtype == torch.float32 and ans.dim() == 4):
        return False
    return laplacian_adjoint_ok(func, params)


class _OdeintAdjoint(torch.autograd.Function):
    """torchdiffeq.odeint_adjoint (0.2.x OdeintAdjointMethod) restated: the
    forward integrates without recording; the backward integrates the augmented
    system (y, a_y, a_theta) from t[-1] back to t[0] with
        dy/dt = f,  da_y/dt = -a_y^T df/dy,  da_theta/dt = -a_y^T df/dtheta
    (vector-Jacobian products through the RHS autograd: K1 over the CSC, the
    SDDMM and the attention backward), adding the output gradient at every
    requested time.  Time runs backwards by integrating in s = -t."""

    @staticmethod
    def forward(ctx, y0, t, cfg, *params):
        func, rtol, atol, method, options = cfg[:5]
        with torch.no_grad():
            ans = odeint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options, combine=cfg[9])
        ctx.cfg = cfg
        ctx.params = params  # the leaf parameters themselves: the VJPs are taken with respect to them
        ctx.save_for_backward(t, ans)
        return ans

    @staticmethod
    def backward(ctx, grad_y):
        func, _rtol, _atol, _method, _options, a_rtol, a_atol, a_method, a_options, combine = ctx.cfg
        t, ans = ctx.saved_tensors
        params = ctx.params
        if _adaptive_adjoint_ok(func, ans, a_method, params, a_options):
            # the Laplacian's adaptive adjoint, fused (gnpde.adjoint_adaptive): the same loop with the
            # packed state's stage combinations, error rows and alpha integrand in the K1 epilogues
            with torch.no_grad():
                solver = AdaptiveAdjoint(func, params, a_method, a_rtol, a_atol, a_options)
                gy, ga, gb = solver.run(_host_times(t), ans, grad_y)
            _OdeintAdjoint.last_path = 'fused_adaptive'
            out = param_grads(params, [(func.alpha_train, ga), (func.beta_train, gb)])
            return (gy.view(grad_y.shape[1:]).to(grad_y.dtype), None, None) + tuple(out)
        y_shape = ans.shape[1:]
        ny = ans[0].numel()
        sizes = [ny, ny] + [p.numel() for p in params]

        pdt = torch.float64 if ans.dtype == torch.float64 else torch.float32  # (fp64: the host tests)

        def pack(y, ay, ap):
            return torch.cat([y.reshape(-1).to(pdt), ay.reshape(-1).to(pdt)] + [a.reshape(-1).to(pdt) for a in ap])

        def aug_autograd(s, z):
            y = z[:ny].view(y_shape)
            ay = z[ny:2 * ny].view(y_shape)
            with torch.enable_grad():
                yv = y.detach().requires_grad_(True)
                f = func(-s, yv)
                grads = torch.autograd.grad(f, (yv,) + tuple(params), -ay, allow_unused=True)
            vjp_y = grads[0] if grads[0] is not None else torch.zeros_like(y)
            vjp_p = [torch.zeros_like(p) if g is None else g for g, p in zip(grads[1:], params)]
            return -pack(f.detach(), vjp_y, vjp_p)  # d/ds = -d/dt

        # the Laplacian's vector-Jacobian products by K1 launches (no autograd), else autograd's
        aug = _laplacian_aug(func, params, y_shape, ny, ans)
        _OdeintAdjoint.last_path = 'direct_aug' if aug is not None else 'autograd'
        aug = aug or aug_autograd
        opts = dict(a_options or {})
        if a_method in ADAPTIVE_METHODS and 'norm' not in opts:
            opts['norm'] = _mixed_norm_fn(sizes)
        ay = grad_y[-1]
        ap = [torch.zeros_like(p) for p in params]
        # weights the RHS closes over are constants of the backward (torchdiffeq: VJPs w.r.t. y and
        # adjoint_params only): the autograd VJPs see them detached
        const_w = hasattr(func, 'adjoint_const_weights') and func.adjoint_direct_ok(params)
        try:
            if const_w:
                func.adjoint_const_weights = True
            with torch.no_grad():
                for i in range(len(t) - 1, 0, -1):
                    z0 = pack(ans[i], ay, ap)
                    s = torch.stack([-t[i], -t[i - 1]])
                    z1 = odeint(aug, z0, s, rtol=a_rtol, atol=a_atol, method=a_method, options=opts,
                                combine=combine)[1]
                    ay = z1[ny:2 * ny].view(y_shape).to(grad_y.dtype) + grad_y[i - 1]
                    o = 2 * ny
                    ap = []
                    for p in params:
                        ap.append(z1[o:o + p.numel()].view(p.shape).to(p.dtype))
                        o += p.numel()
        finally:
            if const_w:
                func.adjoint_const_weights = False
        return (ay, None, None) + tuple(ap)


_OdeintAdjoint.last_path = None  # which backward the last one ran: 'fused_adaptive', 'direct_aug' or 'autograd'


# Fused continuous adjoint of the Laplacian RHS (src/base_classes.py:45-49 with opt['adjoint'],
# src/block_constant.py:34-44: odeint_adjoint with adjoint_method / adjoint_step_size; the
# ogbn-arxiv and Photo best_params run adjoint_method 'rk4', src/best_params.py:6-7).
FUSED_ADJOINT = os.environ.get('GNPDE_FUSED_ADJOINT', '1') != '0'


class _AdjointRHS(object):
    """The adjoint component of the augmented system in s = -t, a' = L^T a with
    L = sigma(alpha)(A - I): K1 over the CSC with the RHS epilogue, whose dot term
    adds coef_i <o_i, y_i> (o_i = L^T a_i, y_i the y component's input at the same
    stage) per row in fp64 — the alpha gradient's integrand sigma'(alpha)<(A^T - I)a, y>
    up to the factor (1 - sigma(alpha)) applied once at the end."""

    def __init__(self, gr, w_csc, alpha, sig, drow):
        self.gr, self.w_csc, self.alpha, self.sig, self.drow = gr, w_csc, alpha, sig, drow
        self.ys, self.coefs, self.i = None, None, 0

    def begin_step(self, ys, coefs):
        self.ys, self.coefs, self.i = ys, coefs, 0

    def rhs_stage(self, t, x, stage):
        stage.dot = (self.ys[self.i], self.drow, self.coefs[self.i], True)
        self.i += 1
        ops.spmm_rhs(self.gr, self.w_csc, x, alpha=self.alpha, rhs=True, alpha_sigmoid=self.sig, transpose=True,
                     stage=stage)


def _fused_adjoint_ok(func, y0, adjoint_method, adjoint_params):
    """odeint_adjoint of a Laplacian RHS with a fixed-grid rk4 adjoint runs fused
    (_LaplacianAdjointFn): a device fp32 state, weights without their own gradient,
    the sigmoid alpha, and adjoint parameters among the module's own."""
    if not (FUSED_ADJOINT and adjoint_method == 'rk4' and y0.is_cuda and y0.dtype == torch.float32 and
            y0.dim() == 3):
        return False
    return laplacian_adjoint_ok(func, adjoint_params)


class _LaplacianAdjointFn(torch.autograd.Function):
    """torchdiffeq.odeint_adjoint (0.2.x OdeintAdjointMethod) of f(y) = sigma(alpha)(A y - y)
    [+ beta x0] with a fixed-grid rk4 adjoint, fused.  Forward: the no-grad solve
    (the fused adaptive step for dopri5).  Backward, per interval [t_{i-1}, t_i] from
    the last, the augmented system integrated over s = -t with torchdiffeq's grid
    (adjoint_options step_size) exactly as torchdiffeq does — y restarts from the
    forward solution at t_i and is integrated backwards too:
        dy/ds = -f(y)                      a fused rk4 step of f with dt = -h
        da/ds = L^T a                      a fused rk4 step over the CSC (_AdjointRHS)
        d alpha/ds = sigma'(alpha) <(A^T - I) a, y>   row terms in the CSC epilogues (dot_rows)
        d beta/ds  = <a, x0>               (add_source) fp64 dots of the stage inputs
    and a += grad_y[i-1] at each output time.  Eight K1 launches per rk4 step, the
    stage combinations in their epilogues, the state in the graph's in-degree
    numbering; the parameter gradients summed once at the end.  The RHS counter
    advances by one per augmented evaluation, as torchdiffeq's backward calls func."""

    @staticmethod
    def forward(ctx, y0, t, cfg, *params):
        func, rtol, atol, method, options = cfg[:5]
        with torch.no_grad():
            ans = odeint(func, y0, t, rtol=rtol, atol=atol, method=method, options=options)
        ctx.cfg = cfg
        ctx.params = params
        ctx.save_for_backward(t, ans)
        return ans

    @staticmethod
    def backward(ctx, grad_y):
        func = ctx.cfg[0]
        a_options = ctx.cfg[8] or {}
        t, ans = ctx.saved_tensors
        params = ctx.params
        t_h = _host_times(t)
        grad_y = grad_y.contiguous()
        with torch.no_grad():
            lay = _node_layout(func, ans[0])
            if lay is not None:
                func._layout = lay
            try:
                o = laplacian_operands(func, ans[0], private_csc=True, acc=1)
                gb, drow = o.acc[0], o.acc[1:]
                add_source, x0 = o.add_source, o.x0
                arhs = _AdjointRHS(o.g, o.w_csc, o.alpha, True, drow)
                step = a_options.get('step_size')

                def internal(v):
                    if lay is None:
                        return v.clone()
                    return _to_internal(v, lay)
                a = internal(grad_y[-1])
                ws_y, ws_a = _Workspace(), _Workspace()
                ybuf = [torch.empty_like(a), torch.empty_like(a)]
                abuf = [torch.empty_like(a), torch.empty_like(a)]
                for i in range(len(t_h) - 1, 0, -1):
                    y = internal(ans[i])
                    # torchdiffeq's grid of the flipped interval, in t's dtype (as its fixed-grid solver)
                    s_t = torch.tensor([-t_h[i], -t_h[i - 1]], dtype=t.dtype)
                    grid = (fixed_grid(s_t, float(step)) if step is not None else s_t).tolist()
                    for sa, sb in zip(grid[:-1], grid[1:]):
                        h = sb - sa
                        if h == 0.0:
                            continue
                        yo = ybuf[0] if ybuf[0] is not y else ybuf[1]
                        ao = abuf[0] if abuf[0] is not a else abuf[1]
                        _fused_step('rk4', func, -sa, -h, -sb, y, ws_y, out=yo)
                        ys = [y, ws_y['a'], ws_y['b'], ws_y['c']]
                        arhs.begin_step(ys, [h / 8.0, 3.0 * h / 8.0, 3.0 * h / 8.0, h / 8.0])
                        _fused_step('rk4', arhs, sa, h, sb, a, ws_a, out=ao)
                        if add_source:  # d beta/ds = <a, x0> at the four stages
                            for c, av in zip((1.0, 3.0, 3.0, 1.0), (a, ws_a['a'], ws_a['b'], ws_a['c'])):
                                gb = gb + (c * h / 8.0) * ops.dot(av, x0)
                        y, a = yo, ao
                    a = a + internal(grad_y[i - 1])
                ga = alpha_grad(drow, o.alpha)
                if lay is not None:
                    gy = torch.empty_like(a)
                    _to_user(a, gy, lay)
                else:
                    gy = a
            finally:
                func._layout = None
        out = param_grads(params, [(func.alpha_train, ga), (func.beta_train, gb if add_source else None)])
        return (gy.view(grad_y.shape[1:]), None, None) + tuple(out)


def odeint_adjoint(func, y0, t, rtol=1e-7, atol=1e-9, method=None, options=None, adjoint_rtol=None,
                   adjoint_atol=None, adjoint_method=None, adjoint_options=None, adjoint_params=None, combine=None):
    """torchdiffeq.odeint_adjoint(func, y0, t, ...) with its defaults: the adjoint
    tolerances / method default to the forward ones, adjoint_options to the
    forward options (without 'norm') when the methods match, adjoint_params to
    func's parameters that require grad.  Gradients reach y0 and adjoint_params
    (as in torchdiffeq, not other tensors the RHS closes over).  ``combine``: odeint's
    (the host tests inject _torch_combine for CPU tensors; None: the HIP stage combinations)."""
    method = method or 'dopri5'
    if isinstance(y0, (tuple, list)):
        raise NotImplementedError("gnpde.odeint_adjoint: a tuple state (ODE regularisers with adjoint=True) is out "
                                  "of scope; train regularised solves with odeint (opt['adjoint'] = False)")
    if adjoint_params is None:
        adjoint_params = tuple(p for p in func.parameters() if p.requires_grad)
    adjoint_params = tuple(adjoint_params)
    adjoint_rtol = rtol if adjoint_rtol is None else adjoint_rtol
    adjoint_atol = atol if adjoint_atol is None else adjoint_atol
    adjoint_method = method if adjoint_method is None else adjoint_method
    if adjoint_options is None:
        adjoint_options = {k: v for k, v in (options or {}).items() if k != 'norm'} if adjoint_method == method \
            else {}
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    cfg = (func, rtol, atol, method, options, adjoint_rtol, adjoint_atol, adjoint_method, adjoint_options, combine)
    if _fused_adjoint_ok(func, y0, adjoint_method, adjoint_params):
        return _LaplacianAdjointFn.apply(y0, t, cfg, *adjoint_params)
    return _OdeintAdjoint.apply(y0, t, cfg, *adjoint_params)


__all__ = ['odeint', 'odeint_adjoint', 'fixed_grid', 'FIXED_METHODS', 'ADAPTIVE_METHODS', 'MULTISTEP_METHODS',
           'math']
