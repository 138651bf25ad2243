"""What the adaptive solver loops share: the embedded tableaus and their stage plans,
the layout copies, torchdiffeq's host controller, the dense-output weights and the
operands of the Laplacian's adjoint launches.

Used by integrator (_RKAdaptiveFused and the adjoint autograd nodes), adaptive_backprop
and adjoint_adaptive; imports ops and _lib only, so those three import it at top level.
"""
import torch

from . import _lib, ops

# Dormand-Prince-Shampine (torchdiffeq dopri5.py)
_DP_ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1., 1.]
_DP_BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
_DP_C_SOL = [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84, 0]
_DP_C_ERROR = [
    35 / 384 - 1951 / 21600,
    0,
    500 / 1113 - 22642 / 50085,
    125 / 192 - 451 / 720,
    -2187 / 6784 - -12231 / 42400,
    11 / 84 - 649 / 6300,
    -1. / 60.,
]
_DP_C_MID = [
    6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
    187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2,
]

# Bogacki-Shampine 3(2) (torchdiffeq bosh3.py)
_BS_ALPHA = [1 / 2, 3 / 4, 1.]
_BS_BETA = [[1 / 2], [0., 3 / 4], [2 / 9, 1 / 3, 4 / 9]]
_BS_C_SOL = [2 / 9, 1 / 3, 4 / 9, 0.]
_BS_C_ERROR = [2 / 9 - 7 / 24, 1 / 3 - 1 / 4, 4 / 9 - 1 / 3, -1 / 8]
_BS_C_MID = [0., 0.5, 0., 0.]

# Heun-Euler 2(1) (torchdiffeq adaptive_heun.py; the reference's default adjoint_method,
# src/run_GNN.py:334, src/best_params.py)
_AH_ALPHA = [1.]
_AH_BETA = [[1.]]
_AH_C_SOL = [0.5, 0.5]
_AH_C_ERROR = [0.5, -0.5]
_AH_C_MID = [0.5, 0.]

# Runge-Kutta-Fehlberg 2(1) (torchdiffeq fehlberg2.py)
_FE_ALPHA = [1 / 2, 1.]
_FE_BETA = [[1 / 2], [1 / 256, 255 / 256]]
_FE_C_SOL = [1 / 512, 255 / 256, 1 / 512]
_FE_C_ERROR = [-1 / 512, 0., 1 / 512]
_FE_C_MID = [0., 0.5, 0.]

# name -> (order, alpha, beta, c_sol, c_error, c_mid)
_TABLEAUS = {
    'dopri5': (5, _DP_ALPHA, _DP_BETA, _DP_C_SOL, _DP_C_ERROR, _DP_C_MID),
    'bosh3': (3, _BS_ALPHA, _BS_BETA, _BS_C_SOL, _BS_C_ERROR, _BS_C_MID),
    'fehlberg2': (2, _FE_ALPHA, _FE_BETA, _FE_C_SOL, _FE_C_ERROR, _FE_C_MID),
    'adaptive_heun': (2, _AH_ALPHA, _AH_BETA, _AH_C_SOL, _AH_C_ERROR, _AH_C_MID),
}


# --------------------------------------------------------------------------- host controller
def next_dt(dt, ratio, order, safety=0.9, ifactor=10.0, dfactor=0.2):
    """torchdiffeq's _optimal_step_size in host floats: the step after one of size dt
    whose error ratio was ``ratio``."""
    if ratio == 0:
        return dt * ifactor
    df = 1.0 if ratio < 1 else dfactor
    return dt * min(ifactor, max(safety / ratio ** (1.0 / order), df))


def check_step(t_cur, dt, n_steps, max_num_steps):
    """The adaptive loops' guards before a step (torchdiffeq's assertions)."""
    if not (t_cur + dt > t_cur):
        raise AssertionError('underflow in dt {}'.format(float(dt)))
    if n_steps >= max_num_steps:
        raise AssertionError('max_num_steps exceeded ({}>={})'.format(n_steps, max_num_steps))


# --------------------------------------------------------------------------- dense output
def dense_weights(x, dt):
    """torchdiffeq's 4th-order dense output (_interp_fit / _interp_evaluate) at the
    fraction x of a step of size dt as weights (cy0, cy1, cym, cf0, cf1) on y0, y1,
    y_mid, f0 and f1."""
    x2, x3, x4 = x * x, x * x * x, x * x * x * x
    cy0 = 1.0 - 11.0 * x2 + 18.0 * x3 - 8.0 * x4
    cy1 = -5.0 * x2 + 14.0 * x3 - 8.0 * x4
    cym = 16.0 * x2 - 32.0 * x3 + 16.0 * x4
    cf0 = dt * (x - 4.0 * x2 + 5.0 * x3 - 2.0 * x4)
    cf1 = dt * (x2 - 3.0 * x3 + 2.0 * x4)
    return cy0, cy1, cym, cf0, cf1


def dense_combo(plan, weights, dt, y1, f0, f1, k):
    """The dense output as ONE stage pass over y0 (its base) and f1 (its f input), with
    y_mid = y0 + dt sum_j c_mid[j] k_j substituted:
        out = (cy0 + cym) y0 + cy1 y1 + sum_j cym dt c_mid[j] k_j + cf0 f0 + cf1 f1.
    ``k(j)`` gives stage derivative j (asked only where c_mid[j] != 0; k(0) is f0 and
    k(ns) f1, whose coefficients are merged).  Returns (base coefficient, f coefficient,
    [(operand, coefficient)])."""
    cy0, cy1, cym, cf0, cf1 = weights
    coef = {}  # id -> [tensor, coefficient] of the operands besides y0 (base) and f1 (f input)
    order = []

    def add(tn, c):
        if c == 0.0:
            return
        if id(tn) not in coef:
            coef[id(tn)] = [tn, 0.0]
            order.append(id(tn))
        coef[id(tn)][1] += c
    add(y1, cy1)
    for j in range(plan.ns + 1):
        if _nz(plan.c_mid[j]):
            add(k(j) if j < plan.ns else f1, cym * dt * plan.c_mid[j])
    add(f0, cf0)
    cf_f1 = coef.pop(id(f1))[1] + cf1 if id(f1) in coef else cf1
    return cy0 + cym, cf_f1, [tuple(coef[i]) for i in order if i in coef]


# --------------------------------------------------------------------------- stage plans
# An embedded Runge-Kutta step of torchdiffeq's adaptive solver (dopri5 — the method
# of every src/best_params.py entry — bosh3, fehlberg2, adaptive_heun) with every
# stage combination and the error estimate in the RHS epilogues (gnpde_stage_
# epilogue_t, the wide epilogue): launch i evaluates k_{i+1} = f(X_i) and writes the
# next stage input X_{i+1} from the rows it holds; the last launch forms the rows of
# the squared error norm.  One host read per step (the norm); no separate
# combination passes besides the step's first stage input.  The plan below derives
# every launch's operands from the tableau, choosing per combination the form that
# reads fewest state arrays:
#   from the launch's own input:  X_{i+1} = X_i + dt sum_j (b_{i+1,j} - b_{i,j}) k_j + dt b_{i+1,i+1} f
#   from the step start:          X_{i+1} = y0  + dt sum_j b_{i+1,j} k_j + dt b_{i+1,i+1} f
# (same values up to rounding: a combination of the k's scaled by dt, never a
# difference of states, so the error estimate keeps its precision).

def _nz(c):
    return c != 0.0


class _AdaptivePlan(object):
    """Per-launch operands of one step of an embedded tableau.

    Symbols: 'Y' the step start y0, 'X' the launch's own input, 'E' the error
    partial, 'K<j>' stage derivative j (K0 = f0 from the previous step).  Each
    combination is (base symbol or None, [(K<j>, coefficient / dt)...], f
    coefficient / dt); dt multiplies every k and f coefficient at run time."""

    def __init__(self, method):
        order, alpha, beta, c_sol, c_err, c_mid = _TABLEAUS[method]
        self.method, self.order, self.alpha, self.beta = method, order, alpha, beta
        self.c_sol, self.c_err, self.c_mid = c_sol, c_err, c_mid
        ns = len(alpha)
        self.ns = ns
        self.fsal = c_sol[-1] == 0 and list(c_sol[:-1]) == list(beta[-1])
        self.launches = []
        reads = []  # K indices each launch reads
        for i in range(ns):
            L = {'next': None, 'y1': None, 'epart': None, 'err': None}
            rd = set()
            if i < ns - 1:
                d = [(j, beta[i + 1][j] - beta[i][j]) for j in range(i + 1)]
                d = [(j, c) for j, c in d if _nz(c)]
                yv = [(j, beta[i + 1][j]) for j in range(i + 1) if _nz(beta[i + 1][j])]
                if len(d) <= len(yv) + 1:
                    L['next'] = ('X', [('K%d' % j, c) for j, c in d], beta[i + 1][i + 1])
                    rd |= {j for j, _ in d}
                else:
                    L['next'] = ('Y', [('K%d' % j, c) for j, c in yv], beta[i + 1][i + 1])
                    rd |= {j for j, _ in yv}
            else:
                if not self.fsal:
                    yv = [(j, c_sol[j]) for j in range(ns) if _nz(c_sol[j])]
                    L['y1'] = ('Y', [('K%d' % j, c) for j, c in yv], c_sol[ns])
                    rd |= {j for j, _ in yv}
            reads.append(rd)
            self.launches.append(L)
        # the error combination e = dt sum_j c_err[j] k_j (k_ns = the last launch's f): all in
        # the last launch, or its first ns terms precomputed by the launch before (a second
        # output 'E') when that launch already reads most of their operands
        last = ns - 1
        ev = [(j, c_err[j]) for j in range(ns) if _nz(c_err[j])]
        direct = {j for j, _ in ev if j < ns} - reads[last]
        pre_ok = ns >= 2
        if pre_ok:
            held = reads[last - 1] | {last}  # launch ns-2 reads its operands and holds k_{ns-1} = its own f
            pre_cost = 2 + len({j for j, _ in ev} - held)
            pre_ok = pre_cost < len(direct) + (0 if last in reads[last] else 0)
        if pre_ok:
            self.launches[last - 1]['epart'] = (None, [('K%d' % j, c) for j, c in ev if j < last], c_err[last])
            self.launches[last]['err'] = ('E', [], c_err[ns])
            reads[last - 1] |= {j for j, _ in ev if j < last}
        else:
            self.launches[last]['err'] = (None, [('K%d' % j, c) for j, c in ev], c_err[ns])
            reads[last] |= {j for j, _ in ev}
        self.reads = reads
        # k_j stored when a later launch reads it (k_ns: always, the next step's f0)
        self.store = set()
        for i in range(ns):
            for j in reads[i]:
                if j >= 1:
                    self.store.add(j)
        self.store.add(ns)
        # dense output (a step that may cross an output time): every k with a c_mid term
        self.store_mid = {j for j in range(1, ns + 1) if _nz(c_mid[j])} - self.store

    def combo(self, spec, sym, mult=1.0):
        """(base tensor, cb, cf, [(k tensor, c)]) of a plan combination.  ``sym`` (a
        callable or a mapping) gives the tensor of a symbol; the k and f coefficients are
        the tableau's times ``mult``: 1.0 where the device scales them by dt (Stage.scale),
        the host's dt otherwise."""
        get = sym if callable(sym) else sym.__getitem__
        base, terms, cfc = spec
        bt = get(base) if base is not None else None
        return bt, (1.0 if bt is not None else 0.0), cfc * mult, [(get(k), c * mult) for k, c in terms]

    def launch(self, i, mid, sym, mult=1.0, restate=None):
        """What launch i writes: (outs, err, err_y1, store) — the Stage's ``outs`` list
        [(destination, base, cb, cf, terms)], the error combination (or None) with its
        err_y1 flag (0: the tolerance takes y1 from output 0), and whether k_{i+1} is
        stored (``mid``: also the k's only the dense output reads).  ``restate`` maps
        each spec before it is resolved (the fused solver's affine first launch)."""
        get = sym if callable(sym) else sym.__getitem__
        L = self.launches[i]
        spec = (lambda s: s) if restate is None else restate
        outs = [(get(dst),) + self.combo(spec(L[key]), get, mult)
                for key, dst in (('next', 'X%d' % (i + 1)), ('y1', 'Y1'), ('epart', 'E')) if L[key] is not None]
        err = self.combo(spec(L['err']), get, mult) if L['err'] is not None else None
        j = i + 1
        return outs, err, (0 if L['y1'] is not None else -1), (j in self.store or bool(mid and j in self.store_mid))

    def state_passes(self):
        """Full-state reads / writes per step beyond each launch's own gathers,
        input row and one output (the bench's overhead check)."""
        r = 2  # the step's first stage input: y0 and k0
        w = 1
        for i, L in enumerate(self.launches):
            outs = [c for c in (L['next'], L['y1'], L['epart']) if c is not None]
            r += len(self.reads[i]) + sum(1 for c in outs if c[0] in ('Y', 'E'))
            if L['err'] is not None:
                r += 1 + (1 if L['err'][0] == 'E' else 0)  # y0 for the tolerance, E
            stored = (i + 1) in self.store
            w += len(outs) + (1 if stored else 0) - 1
        return r, w


_PLANS = {}


def _adaptive_plan(method):
    p = _PLANS.get(method)
    if p is None:
        p = _PLANS[method] = _AdaptivePlan(method)
    return p


class _KrylovPlan(object):
    """The step of an FSAL tableau for an affine RHS f(y) = L y + s in the Krylov basis
    u_p = (dt L)^p f0 (u_0 = f0 = f(y0)).  Every stage derivative is a fixed
    combination of them: k_0 = u_0, k_{i+1} = f(y0 + dt sum_j beta[i][j] k_j)
    = k_0 + sum_j beta[i][j] (dt L) k_j, so k_i = sum_p B[i][p] u_p with
    B[i+1][p] = sum_j beta[i][j] B[j][p-1].  A step is ns launches of the linear part,
    u_{p+1} = dt L u_p, each reading only its own input (no stage operand); the last
    (over u_{ns-1}, with f_lin = 1: f' = u_{ns-1} + u_ns) forms
      y1  = y0 + dt sum_p G[p] u_p,                 G[p]   = sum_j c_sol[j] B[j][p]
      f1  = sum_p B[ns][p] u_p                      (the next step's f0: unscaled)
      e   = dt sum_p Eps[p] u_p,                    Eps[p] = sum_j c_err[j] B[j][p]
    with u_ns = f' - u_{ns-1} substituted.  Mathematically the tableau's step; Eps[p]
    vanishes exactly for p below the embedded order (the order conditions of the
    linear problem), which the fp64 sums leave at rounding level and the plan zeroes,
    so the error estimate carries no stage-combination cancellation noise.  Dense
    output: y_mid = y0 + dt (sum_p Mu[p] u_p + c_mid[ns] f1), Mu[p] = sum_{j<ns}
    c_mid[j] B[j][p], with y1 restated on the u_p (one pass over ns + 2 rows)."""

    def __init__(self, plan):
        ns, beta = plan.ns, plan.beta
        B = [[1.0]]
        for i in range(ns):
            B.append([1.0] + [sum(beta[i][j] * B[j][p - 1] for j in range(p - 1, i + 1))
                              for p in range(1, i + 2)])
        self.B = B

        def comb(c, upto):
            v = [sum(c[j] * B[j][p] for j in range(p, upto)) for p in range(ns + 1)]
            big = max(1.0, max(abs(x) for x in v))
            return [0.0 if abs(x) < 1e-12 * big else x for x in v]
        self.G = comb(plan.c_sol, ns + 1)
        self.Eps = comb(plan.c_err, ns + 1)
        self.Mu = comb(plan.c_mid, ns)
        self.Bn = list(B[ns])
        self.ns = ns

    def last_launch_terms(self):
        """(y1 terms, (f1 terms, f1 cf), (error terms, error cf)) of the last launch over
        u_{ns-1}, as [(p, coefficient)] with u_ns = f' - u_{ns-1} substituted."""
        ns = self.ns

        def sub(v):
            t = [(p, v[p]) for p in range(ns - 1) if v[p] != 0.0]
            c = v[ns - 1] - v[ns]
            if c != 0.0:
                t.append((ns - 1, c))
            return t, v[ns]
        y1 = [(p, self.G[p]) for p in range(ns) if self.G[p] != 0.0]
        return y1, sub(self.Bn), sub(self.Eps)

    def state_passes(self):
        """Full-state reads / writes per step beyond each launch's gathers, input row
        and one output: the last launch reads y0 (the y1 base and the tolerance) and
        u_0 .. u_{ns-2}, and writes a second output (f1)."""
        return self.ns, 1


_KRYLOV_PLANS = {}


def _krylov_plan(plan):
    """The _KrylovPlan of a tableau plan, built once (its fp64 sums cost ~50 us of host
    time, which every solve paid before its first launch)."""
    k = _KRYLOV_PLANS.get(plan.method)
    if k is None:
        k = _KRYLOV_PLANS[plan.method] = _KrylovPlan(plan)
    return k


def rotate(bufs, plan, d=1):
    """Advance (d = 1) or undo (d = -1) the binding of y0 / f0 after an accepted
    step: two buffers swap; with the third (steps ahead: 'Ys' / 'Ks') the three rotate."""
    for a, b, c in (('Y', 'Y1', 'Ys'), ('K0', 'K%d' % plan.ns, 'Ks')):
        if c not in bufs:
            bufs[a], bufs[b] = bufs[b], bufs[a]
        elif d > 0:
            bufs[a], bufs[b], bufs[c] = bufs[b], bufs[c], bufs[a]
        else:
            bufs[a], bufs[b], bufs[c] = bufs[c], bufs[a], bufs[b]
    if plan.fsal:
        bufs['X%d' % (plan.ns - 1)] = bufs['Y1']


class _AdaptiveState(object):
    """Buffers and captured step graphs of one module's fused adaptive solves of one
    state shape and tolerance (kept across odeint calls, like integrator._StatePool)."""

    def __init__(self, plan, y0, host):
        new = lambda: torch.empty_like(y0, memory_format=torch.contiguous_format)  # noqa: E731
        b = {'Y': new(), 'Y1': new(), 'K0': new()}
        for j in sorted(plan.store | plan.store_mid):
            b['K%d' % j] = new()
        xa, xb = new(), new()
        for i in range(plan.ns):
            b['X%d' % i] = b['Y1'] if (plan.fsal and i == plan.ns - 1) else (xa if i % 2 == 0 else xb)
        if any(L['epart'] is not None for L in plan.launches):
            b['E'] = new()
        self.bufs = b
        self.rows = torch.empty(y0.numel() // y0.shape[-1], dtype=torch.float64, device=y0.device)
        # the step size the stage coefficients are scaled by (device fp32 scalar; the host-stage
        # test RHS objects apply it in their own precision)
        self.scale = torch.zeros((), dtype=torch.float32 if not host else torch.float64, device=y0.device)
        # the device controller's step size (fp64) and its record {ratio, dt, next dt} (device solves)
        # h = {h0, d1, first step} of the device initial-step selection; dt is h[2] (a view), so
        # the first step's size and scale are in place when the selection ends
        self.h = None if host else torch.zeros(3, dtype=torch.float64, device=y0.device)
        self.dt = None if host else self.h[2]
        self.rec = None if host else torch.zeros(4, dtype=torch.float64, device=y0.device)
        self.ws = None if host else torch.empty(_lib.fn("gnpde_dot_workspace_bytes")(), dtype=torch.uint8,
                                                device=y0.device)
        self.rec_host, self.rec_slot = None, 0  # pinned copies of rec (_rec_reader)
        # the folded dense output (DENSE_FOLD): the device time {step start, output time} the controller
        # advances, the slot holding the output array's address, the output row map (a copy: the
        # captured launch reads this buffer whatever layout object the solve has)
        # one device record {t0, t_out, output address} (fp64 / fp64 / int64 views) set per solve by one
        # copy from a pinned host twin
        self.dsc = None if host else torch.zeros(3, dtype=torch.float64, device=y0.device)
        self.dsc_host = None if host else torch.zeros(3, dtype=torch.float64, pin_memory=True)
        self.dsc_np = None if host else self.dsc_host.numpy()  # (host writes through numpy: no torch ops)
        self.tdev = None if host else self.dsc[:2]
        self.dslot = None if host else self.dsc[2:].view(torch.int64)
        self.dtab = None if host else torch.zeros(_lib.DENSE_SLOTS + 1, dtype=torch.float32, device=y0.device)
        self.drows, self.drows_src = None, None
        # the initial-step selection from the f0 / probe launches' row sums (INIT_ROWS): a second
        # row array (the f0 launch's scale_rows) and the reduction's workspace
        self.rows2, self.iws = None, None
        self.side = None  # the second stream of the initial step (LIN_INIT)
        # the captured prologue of a lin_init solve (f0 and the initial-step launches) and the
        # workspaces of its two reductions (phase 0 runs beside the probe: two buffers)
        self.pro = None
        self.iws0 = self.iws1 = None
        self.canon = None  # the y / f0 buffer binding every solve starts from (_integrate)
        self.graphs = {}   # (id Y, id K0, mid, fold, renumbered) -> (graph, error-sum tensor)
        self.mempool = None
        self.warm = False


# --------------------------------------------------------------------------- layout copies
def _node_layout(func, y0):
    """The locality numbering (ops.NodeLayout) the fused path keeps the state in, or None."""
    fn = getattr(func, 'node_layout', None)
    return fn(y0) if fn is not None else None


def _entry_copy(y0, buf, sol0, order):
    """buf = y0 in the solve's numbering (order: internal row k holds user row
    order[k]), sol0 = y0: one pass (gnpde_rows_copy) when rows are 16-byte
    multiples, torch copies otherwise."""
    if y0.is_cuda and (y0.shape[-1] * y0.element_size()) % 16 == 0 and y0.is_contiguous():
        ops.rows_copy(y0, buf, order=order, dst_copy=sol0)
        return
    sol0.copy_(y0)
    if order is None:
        buf.copy_(y0)
    else:
        C = y0.shape[-1]
        torch.index_select(y0.reshape(-1, C), 0, order, out=buf.view(-1, C))


def _to_internal(src, lay, out=None):
    """src (caller's numbering) gathered into the solve's numbering: into ``out`` (a
    plain copy without a layout), or a fresh tensor."""
    if out is not None and lay is None:
        return out.copy_(src)
    if src.is_cuda and (src.shape[-1] * src.element_size()) % 16 == 0 and (out is not None or src.is_contiguous()):
        dst = torch.empty_like(src) if out is None else out
        ops.rows_copy(src.contiguous(), dst, order=lay.order)
        return dst
    if out is None:
        return lay.to_internal(src)
    C = src.shape[-1]
    return torch.index_select(src.reshape(-1, C), 0, lay.order, out=out.view(-1, C))


def _to_user(src, dst, lay):
    """dst = src in the caller's numbering (a fresh solution slice)."""
    if lay is None:
        dst.copy_(src)
    elif src.is_cuda and (src.shape[-1] * src.element_size()) % 16 == 0:
        ops.rows_copy(src, dst, order=lay.new_id)
    else:
        C = src.shape[-1]
        torch.index_select(src.reshape(-1, C), 0, lay.new_id, out=dst.view(-1, C))


# --------------------------------------------------------------------------- the Laplacian's adjoint
class LaplacianOperands(object):
    """What the launches of the Laplacian's adjoint (L^T over the CSC, the alpha rows,
    <., x0>) read: the graph, the COO weights and their CSR- / CSC-order gathers, detached
    alpha and beta, whether alpha goes through the sigmoid, add_source with x0, and the
    fp64 accumulator (``acc``: its last R entries are the per-row alpha terms)."""
    __slots__ = ('g', 'w', 'w_csr', 'w_csc', 'alpha', 'beta', 'sig', 'add_source', 'x0', 'acc')


def laplacian_operands(func, y_like, csr=False, private_csc=False, snapshot=False, acc=None, acc_zero=True):
    """The LaplacianOperands of ``func`` for a state shaped like y_like.  csr: also the
    CSR-order weights (the module's cache).  private_csc: the CSC-order weights as this
    call's own gather, not the module's cached buffer.  acc: the scalar slots before the
    R row terms of the fp64 accumulator (None: no buffer).

    snapshot=False hands out the module's own tensors: cached weight buffers and the
    stable x0, which a later no_grad solve refreshes in place.  That is right for the
    continuous-adjoint nodes (_OdeintAdjoint, _LaplacianAdjointFn, AdaptiveAdjoint), which
    call this when backward runs and read the module as it is then: torchdiffeq's own
    semantics, whose backward calls func.  snapshot=True is for a node that differentiates
    what its forward computed (the discrete adjoints): alpha, beta and x0 are copies, and
    the CSC weights a buffer the module never refreshes (a private gather, or the cached
    one taken with grad mode on — it is off inside a Function's forward — which
    csr_weights then marks as seen by autograd)."""
    o = LaplacianOperands()
    o.g = g = func.graph_for(y_like)
    o.w, tag = func._weights_tensor()
    o.w_csr = func.csr_weights(g, o.w, tag) if csr else None
    if private_csc:
        o.w_csc = g.gather_weights(o.w.detach().float() if o.w.dtype != torch.float32 else o.w.detach(),
                                   transpose=True)
    else:
        with torch.set_grad_enabled(snapshot or torch.is_grad_enabled()):
            o.w_csc = func.csr_weights(g, o.w, tag, transpose=True)
    o.alpha, o.beta = func.alpha_train.detach(), func.beta_train.detach()
    o.sig = not func.opt.get('no_alpha_sigmoid', False)
    o.add_source = bool(func.opt.get('add_source', False))
    o.x0 = func.stable_x0(y_like) if o.add_source else None
    if snapshot:
        o.alpha, o.beta = o.alpha.clone(), o.beta.clone()
        o.x0 = o.x0.clone() if o.x0 is not None else None
    o.acc = None
    if acc is not None:
        n = acc + y_like.numel() // y_like.shape[-1]
        o.acc = (torch.zeros if acc_zero else torch.empty)(n, dtype=torch.float64, device=y_like.device)
    return o


def laplacian_adjoint_ok(func, params):
    """The adjoint of ``func`` may run by K1 launches (no autograd): the HIP Laplacian
    with weights that are not adjoint parameters (adjoint_direct_ok), the sigmoid alpha,
    and adjoint parameters among the module's own."""
    fn = getattr(func, 'adjoint_direct_ok', None)
    if fn is None or not fn(params) or not hasattr(func, 'rhs_stage') or func.opt.get('no_alpha_sigmoid', False):
        return False
    own = {id(p) for p in func.parameters()}
    return all(id(p) in own for p in params)


def alpha_grad(drow, alpha):
    """The alpha gradient from its per-row terms <L^T a, y> (fp64): their sum times
    sigma'(alpha) / sigma(alpha) = 1 - sigma(alpha), the sigmoid in alpha's precision."""
    return ops.sum_f64(drow) * (1.0 - torch.sigmoid(alpha).double())


def param_grads(params, grads):
    """One gradient per entry of ``params``: ``grads`` is [(parameter, value)], the value
    a tensor, a host float, or None; every other parameter gets zeros."""
    out = []
    for p in params:
        v = next((v for q, v in grads if q is p), None)
        if v is None:
            out.append(torch.zeros_like(p))
        elif isinstance(v, torch.Tensor):
            out.append(v.to(p.dtype).reshape(p.shape))
        else:
            out.append(torch.full(p.shape, v, dtype=p.dtype, device=p.device))
    return out
