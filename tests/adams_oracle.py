"""Numpy oracle of the Adams-Bashforth-Moulton multistep solvers (gnpde.integrator:
explicit_adams / implicit_adams; torchdiffeq 0.2.x fixed_adams), in any float dtype.

Coefficients come from the defining formula evaluated with fractions.Fraction:

    AB[k][j] = int_0^1 l_j(s) ds over the nodes 0, -1, ..., -(k-1)
    AM[k][j] = int_0^1 l_j(s) ds over the nodes 1,  0, ..., -(k-2)

(l_j the Lagrange basis polynomial of node j).  Per step from (t0, y0) to t1 = t0 + dt:

1. f0 = f(t0, y0) joins the front of prev_f (at most max_order - 1 entries);
2. order = min(len(prev_f), max_order - 1);
3. order < 3: the step is an rk4 (3/8 rule) step with k1 = f0 and nothing more (as
   torchdiffeq: the corrector belongs to the Adams branch);
4. else dy = dt sum_j AB[order][j] prev_f[j]; explicit_adams stops here;
5. implicit_adams: m = AM[order + 1], delta = dt sum_j m[j+1] prev_f[j]; up to max_iters times
   dy_old = dy, dy = dt m[0] f(t1, y0 + dy) + delta, ratio = max |dy_old - dy| /
   (atol + rtol max(|dy_old|, |dy|)); stop when ratio < 1 (a NaN is not converged);
6. never converged: prev_f drops its oldest entry;
7. y1 = y0 + dy.
"""
import collections
from fractions import Fraction

import numpy as np


def _basis_integral(nodes, j):
    """int_0^1 of the Lagrange basis polynomial of nodes[j], exactly."""
    poly, den = [Fraction(1)], Fraction(1)
    for m, xm in enumerate(nodes):
        if m == j:
            continue
        new = [Fraction(0)] * (len(poly) + 1)
        for k, c in enumerate(poly):
            new[k + 1] += c
            new[k] -= c * xm
        poly = new
        den *= nodes[j] - xm
    return sum(c / (k + 1) for k, c in enumerate(poly)) / den


def bashforth(k):
    nodes = [Fraction(-i) for i in range(k)]
    return [_basis_integral(nodes, j) for j in range(k)]


def moulton(k):
    nodes = [Fraction(1 - i) for i in range(k)]
    return [_basis_integral(nodes, j) for j in range(k)]


_TABLES = {}


def tables():
    """({k: AB[k]}, {k: AM[k]}) for k = 1 .. 12 as floats (each Fraction rounded once)."""
    if not _TABLES:
        _TABLES['ab'] = {k: [float(c) for c in bashforth(k)] for k in range(1, 13)}
        _TABLES['am'] = {k: [float(c) for c in moulton(k)] for k in range(1, 13)}
    return _TABLES['ab'], _TABLES['am']


def grid(t0, t1, step_size, dtype=np.float64):
    """torchdiffeq's fixed grid (_grid_constructor_from_step_size) in ``dtype``."""
    dtype = np.dtype(dtype).type
    t0, t1, h = dtype(t0), dtype(t1), dtype(step_size)
    niters = int(np.ceil((t1 - t0) / h + dtype(1)))
    g = np.arange(niters).astype(dtype) * h + t0
    g[-1] = t1
    return [float(v) for v in g]


Result = collections.namedtuple('Result', 'y sol iterations ratios converged nfe')


def solve(f, y0, grid_t, method, rtol=1e-7, atol=1e-9, max_order=12, max_iters=4, dtype=np.float64, times=None):
    """Integrate over the grid points ``grid_t``.  Returns Result: y (the state at the last grid
    point), sol (the states at ``times``, linearly interpolated inside a step; None without
    times), iterations (corrector iterations per step, 0 for rk4 / explicit steps), ratios
    (per step, the list of every iteration's ratio), converged (per step) and nfe."""
    assert method in ('explicit_adams', 'implicit_adams')
    ab, am = tables()
    dtype = np.dtype(dtype).type
    y = np.asarray(y0, dtype)
    prev = collections.deque(maxlen=max(max_order - 1, 0))
    nfe = [0]

    def rhs(t, v):
        nfe[0] += 1
        return np.asarray(f(t, v), dtype)

    def lincomb(vals, coefs, dt):
        acc = np.zeros_like(y)
        for c, v in zip(coefs, vals):
            acc = acc + dtype(dt * c) * v
        return acc

    iterations, ratios, converged = [], [], []
    sol = None if times is None else [y]
    j = 1
    for ta, tb in zip(grid_t[:-1], grid_t[1:]):
        dt = tb - ta
        f0 = rhs(ta, y)
        prev.appendleft(f0)
        order = min(len(prev), max_order - 1)
        its, rs, conv = 0, [], True
        if order < 3:
            k2 = rhs(ta + dt / 3.0, y + dtype(dt / 3.0) * f0)
            k3 = rhs(ta + dt * 2.0 / 3.0, y + dtype(dt * (-1.0 / 3.0)) * f0 + dtype(dt) * k2)
            k4 = rhs(tb, y + dtype(dt) * f0 + dtype(-dt) * k2 + dtype(dt) * k3)
            y1 = y + dtype(dt * 0.125) * f0 + dtype(dt * 0.375) * k2 + dtype(dt * 0.375) * k3 + dtype(dt * 0.125) * k4
        else:
            hist = list(prev)[:order]
            dy = lincomb(hist, ab[order], dt)
            if method == 'implicit_adams':
                m = am[order + 1]
                delta = lincomb(hist, m[1:], dt)
                conv = False
                for _ in range(max_iters):
                    dy_old = dy
                    dy = delta + dtype(dt * m[0]) * rhs(tb, y + dy)
                    with np.errstate(invalid='ignore', divide='ignore'):
                        tol = dtype(atol) + dtype(rtol) * np.maximum(np.abs(dy_old), np.abs(dy))
                        q = np.abs(dy_old - dy) / tol
                    r = float('nan') if np.isnan(q).any() else float(q.max())
                    its += 1
                    rs.append(r)
                    if r < 1.0:
                        conv = True
                        break
                if not conv:
                    prev.pop()
            y1 = y + dy
        iterations.append(its)
        ratios.append(rs)
        converged.append(conv)
        while sol is not None and j < len(times) and tb >= times[j]:
            if times[j] == tb:
                sol.append(y1)
            elif times[j] == ta:
                sol.append(y)
            else:
                sol.append(y + dtype((times[j] - ta) / (tb - ta)) * (y1 - y))
            j += 1
        y = y1
    return Result(y, None if sol is None else np.stack(sol), iterations, ratios, converged, nfe[0])


def margin_ok(ratios, lo=2.0 / 3.0, hi=1.5):
    """Every convergence ratio lies outside [lo, hi]: the iteration counts do not hinge on
    rounding."""
    return all(not (lo <= r <= hi) for rs in ratios for r in rs)
