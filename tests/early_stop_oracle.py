"""The early-stop integrator in float64 numpy — TEST INFRASTRUCTURE (the reference's
src/early_stop_solver.py read as gnpde.early_stop_solver's docstring records): the
accepted-step loop of oracle.gnpde_oracle.odeint_adaptive (its tableaus imported,
the oracle itself untouched) with the attempt cap and a score after every accepted
step, and the same over the rk4 grid.  Every scored step is returned with its t1,
per-row predictions, the three correct-row counts and the top-2 logit margin of
every row, with the bests picked by the strict ``val > best_val`` rule."""
import numpy as np

import gnpde_oracle as O


class Step(object):
    __slots__ = ('t1', 'y', 'pred', 'counts', 'margin', 'absdot')

    def __init__(self, t1, y, pred, counts, margin, absdot):
        self.t1, self.y, self.pred, self.counts, self.margin, self.absdot = t1, y, pred, counts, margin, absdot


class Result(object):
    """steps: the scored steps; y: the returned state; n_attempts / n_accepted / n_rejected;
    best_train / best_val / best_test / best_time; sizes: the three mask sizes."""


def decode(y, W, b, Cd=None):
    """relu of the first Cd columns, the linear layer: logits [R, K] in float64, and per row
    max_c sum_j |W_cj z_j| (the size of the fp32 dot's rounding)."""
    W = np.asarray(W, np.float64)
    Cd = W.shape[1] if Cd is None else Cd
    z = np.maximum(np.asarray(y, np.float64).reshape(-1, y.shape[-1])[:, :Cd], 0.0)
    logits = z @ W.T + (0.0 if b is None else np.asarray(b, np.float64))
    return logits, (z @ np.abs(W).T).max(1)


def score(y, W, b, masks, labels):
    """(pred [R], counts (3,), margin [R], absdot [R]) of one state; masks: three bool [R]."""
    logits, absdot = decode(y, W, b)
    pred = logits.argmax(1)  # numpy: the first maximal class
    if logits.shape[1] > 1:
        top2 = np.sort(logits, 1)[:, -2:]
        margin = top2[:, 1] - top2[:, 0]
    else:
        margin = np.full(len(pred), np.inf)
    counts = tuple(int(((pred == labels) & m).sum()) for m in masks)
    return pred, counts, margin, absdot


def _finish(res, masks):
    res.sizes = tuple(int(m.sum()) for m in masks)
    res.best_train = res.best_val = res.best_test = res.best_time = 0
    for s in res.steps:
        acc = [c / n if n else 0.0 for c, n in zip(s.counts, res.sizes)]
        if acc[1] > res.best_val:
            res.best_train, res.best_val, res.best_test, res.best_time = acc[0], acc[1], acc[2], s.t1
    return res


def early_stop_adaptive(func, y0, t_end, method, rtol, atol, W, b, masks, labels, max_attempts):
    """odeint_adaptive's loop over [0, t_end] with at most max_attempts attempts (rejected
    ones included) and a score after every accepted step; returns the state at t_end
    (dense output) or, when the cap was reached first, at the last accepted t1."""
    order, A, bsol, e, mid = O.ADAPTIVE_TABLEAUS[method]
    fsal = bsol[-1] == 0 and list(bsol[:-1]) == list(A[-1])
    rms = lambda v: float(np.sqrt(np.mean(np.square(v))))  # noqa: E731
    y = np.asarray(y0, np.float64)
    f = func(0.0, y)
    sc = atol + np.abs(y) * rtol
    d0, d1 = rms(y / sc), rms(f / sc)
    h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
    f_probe = func(h0, y + h0 * f)
    d2 = rms((f_probe - f) / sc) / h0
    h1 = max(1e-6, h0 * 1e-3) if (d1 <= 1e-15 and d2 <= 1e-15) else (0.01 / max(d1, d2)) ** (1.0 / order)
    h = min(100 * h0, h1)
    t = 0.0
    res = Result()
    res.steps, res.n_attempts, res.n_rejected = [], 0, 0
    seg = None
    while t_end > t and res.n_attempts < max_attempts:
        ks = [f]
        for row in A:
            ks.append(func(t + h * sum(row), y + h * sum(c * k for c, k in zip(row, ks))))
        y_new = y + h * sum(c * k for c, k in zip(A[-1], ks)) if fsal else y + h * sum(c * k for c, k in zip(bsol, ks))
        err = h * sum(c * k for c, k in zip(e, ks))
        ratio = rms(err / (atol + rtol * np.maximum(np.abs(y), np.abs(y_new))))
        if ratio <= 1:
            seg = (t, t + h, y, y_new, ks[0], ks[-1], y + h * sum(c * k for c, k in zip(mid, ks)), h)
            t, y, f = t + h, y_new, ks[-1]
            res.steps.append(Step(t, y, *score(y, W, b, masks, labels)))
        else:
            res.n_rejected += 1
        h = h * 10.0 if ratio == 0 else h * min(10.0, max(0.9 * ratio ** (-1.0 / order), 0.2 if ratio >= 1 else 1.0))
        res.n_attempts += 1
    res.n_accepted = len(res.steps)
    res.capped = t_end > t
    if res.capped or seg is None or t == t_end:
        res.y = y
    else:
        ta, tb, ya, yb, fa, fb, ym, hs = seg
        p4 = 2 * hs * (fb - fa) - 8 * (yb + ya) + 16 * ym
        p3 = hs * (5 * fa - 3 * fb) + 18 * ya + 14 * yb - 32 * ym
        p2 = hs * (fb - 4 * fa) - 11 * ya - 5 * yb + 16 * ym
        x = (t_end - ta) / (tb - ta)
        res.y = ya + x * (hs * fa) + x ** 2 * p2 + x ** 3 * p3 + x ** 4 * p4
    return _finish(res, masks)


def early_stop_rk4(func, y0, t_end, step_size, W, b, masks, labels):
    """oracle.odeint_fixed's rk4 (3/8 rule) over torchdiffeq's grid with a score after every step."""
    y = np.asarray(y0, np.float64)
    grid = O.fixed_grid(0.0, t_end, step_size)
    res = Result()
    res.steps = []
    for ta, tb in zip(grid[:-1], grid[1:]):
        ta, tb = float(ta), float(tb)
        dt = tb - ta
        k1 = func(ta, y)
        k2 = func(ta + dt / 3.0, y + dt * k1 / 3.0)
        k3 = func(ta + dt * 2.0 / 3.0, y + dt * (k2 - k1 / 3.0))
        k4 = func(tb, y + dt * (k1 - k2 + k3))
        y = y + (k1 + 3.0 * (k2 + k3) + k4) * dt * 0.125
        res.steps.append(Step(tb, y, *score(y, W, b, masks, labels)))
    res.y = y
    res.n_attempts = res.n_accepted = len(res.steps)
    res.n_rejected, res.capped = 0, False
    return _finish(res, masks)


def undecided(step, W, delta_state=1e-5):
    """Rows whose oracle prediction an fp32 solve within the project's state parity bar may
    not reproduce: margin <= delta = 2 (delta_state max_c ||W_c||_1 + Cd 2^-24 max_c sum_j |W_cj z_j|)."""
    W = np.asarray(W, np.float64)
    delta = 2.0 * (delta_state * np.abs(W).sum(1).max() + W.shape[1] * 2.0 ** -24 * step.absdot)
    return step.margin <= delta
