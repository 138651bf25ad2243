"""Float64 torch restatement (CPU) of the regularised Laplacian solve: the oracle of
tests/test_reg_host.py and tests/test_gpu_reg.py.

A is dense, taken from the COO lists with duplicates summed (A[b, src(e), dst(e)] += w_e, as the
reference's sparse_coo_tensor(...).to_dense()).  The regularisers are written literally, the
directional one with autograd.grad(dx, x, dx, create_graph=True) (``double_backward=True``) or by
its analytic vector-Jacobian product v = a (A^T f - f); the tuple-state euler, midpoint and rk4
3/8 steps are torchdiffeq's.
"""
import numpy as np
import torch

F64 = torch.float64


def t64(a, requires_grad=False):
    return torch.as_tensor(np.asarray(a), dtype=F64).clone().requires_grad_(requires_grad)


def dense_adjacency(edge_index, w, N):
    """[B,N,N] float64: A[b, src, dst] = the sum of the weights of the edges (src, dst); w a torch
    tensor [B,E] (autograd flows to it) or [B,E,h] (its head mean)."""
    ei = torch.as_tensor(np.asarray(edge_index), dtype=torch.int64)
    B, _, E = ei.shape
    if w.dim() == 3:
        w = w.mean(dim=2)
    flat = (torch.arange(B)[:, None] * N * N + ei[:, 0] * N + ei[:, 1]).reshape(-1)
    return torch.zeros(B * N * N, dtype=F64).index_add(0, flat, w.reshape(-1).to(F64)).view(B, N, N)


class Laplacian(object):
    """f(t, x) = a (A x - x) [+ beta x0], a = sigmoid(alpha) unless no_alpha_sigmoid."""

    def __init__(self, edge_index, w, N, alpha, beta, x0=None, add_source=False, no_alpha_sigmoid=False):
        self.w = w
        self.A = dense_adjacency(edge_index, w, N)
        self.alpha, self.beta, self.x0 = alpha, beta, x0
        self.add_source, self.no_alpha_sigmoid = add_source, no_alpha_sigmoid

    @property
    def a(self):
        return self.alpha if self.no_alpha_sigmoid else torch.sigmoid(self.alpha)

    def __call__(self, t, x):
        f = self.a * (torch.matmul(self.A, x) - x)
        if self.add_source:
            f = f + self.beta * self.x0
        return f

    def vjp(self, f):
        """(df/dx)^T f, analytic."""
        return self.a * (torch.matmul(self.A.transpose(1, 2), f) - f)


def quadratic_cost(x, t, dx, func):
    return 0.5 * dx.pow(2).mean(dim=-1)


def directional_derivative(x, t, dx, func, double_backward=True):
    if double_backward:
        v = torch.autograd.grad(dx, x, dx, create_graph=True)[0]
    else:
        v = func.vjp(dx)
    return 0.5 * v.pow(2).mean(dim=-1)


KINDS = {'kinetic': quadratic_cost, 'directional': directional_derivative}


def reg_rhs(func, kinds, double_backward=True):
    """(t, (x, r_1, ...)) -> (f, e_1, ...) for kinds among 'kinetic', 'directional'."""
    def rhs(t, state):
        x = state[0]
        if not x.requires_grad:
            x.requires_grad_(True)
        dx = func(t, x)
        out = [dx]
        for k in kinds:
            if k == 'directional':
                out.append(directional_derivative(x, t, dx, func, double_backward))
            else:
                out.append(quadratic_cost(x, t, dx, func))
        return tuple(out)
    return rhs


def _axpy(y, ks, cs, dt):
    return tuple(yi + dt * sum(c * k[i] for c, k in zip(cs, ks)) for i, yi in enumerate(y))


def step(method, rhs, t0, dt, y):
    if method == 'euler':
        return _axpy(y, [rhs(t0, y)], [1.0], dt)
    if method == 'midpoint':
        k1 = rhs(t0, y)
        return _axpy(y, [rhs(t0 + 0.5 * dt, _axpy(y, [k1], [0.5], dt))], [1.0], dt)
    if method == 'rk4':  # torchdiffeq rk4_alt_step_func, the 3/8 rule
        k1 = rhs(t0, y)
        k2 = rhs(t0 + dt / 3.0, _axpy(y, [k1], [1.0 / 3.0], dt))
        k3 = rhs(t0 + dt * 2.0 / 3.0, _axpy(y, [k1, k2], [-1.0 / 3.0, 1.0], dt))
        k4 = rhs(t0 + dt, _axpy(y, [k1, k2, k3], [1.0, -1.0, 1.0], dt))
        return _axpy(y, [k1, k2, k3, k4], [0.125, 0.375, 0.375, 0.125], dt)
    raise ValueError(method)


def solve(func, kinds, x, t0, t1, n_steps, method, double_backward=True):
    """(z, (r_1(T), ...)) of the tuple state (x, 0, ...) over n_steps equal steps."""
    rhs = reg_rhs(func, kinds, double_backward)
    y = (x,) + tuple(torch.zeros(x.shape[:-1], dtype=F64) for _ in kinds)
    dt = (t1 - t0) / n_steps
    for i in range(n_steps):
        y = step(method, rhs, t0 + i * dt, dt, y)
    return y[0], tuple(y[1:])


def hub_graph(rng, B, N, E, hub_edges, dup, n_isolated=2):
    """[B,2,E] int64: a source hub (node 1, hub_edges edges), ``dup`` duplicated edges, self loops,
    and n_isolated nodes no edge touches."""
    ei = np.zeros((B, 2, E), dtype=np.int64)
    for b in range(B):
        live = np.arange(N - n_isolated)
        src, dst = rng.choice(live, size=E), rng.choice(live, size=E)
        src[:hub_edges] = 1
        dst[hub_edges:hub_edges + 3] = src[hub_edges:hub_edges + 3]
        if dup:
            pick = rng.choice(E - dup, size=dup)
            src[E - dup:], dst[E - dup:] = src[pick], dst[pick]
        perm = rng.permutation(E)
        ei[b, 0], ei[b, 1] = src[perm], dst[perm]
    return ei
