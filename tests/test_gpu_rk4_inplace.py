"""The no-grad fixed-grid rk4 solve in three state buffers (gnpde.integrator):
stage 3 writes x4 over x2 and stage 4 writes y1 over y, each an output that aliases one of
its own operands.  The solve must equal, bit for bit, a chain of default (out-of-place)
_fused_step calls, leave the caller's y0 alone, and the aliasing rule of ops.Stage /
include/gnpde.h must hold.
"""
import ctypes

import numpy as np
import pytest
import torch

import gnpde
from gnpde import _lib, integrator as gi, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = 0.0625  # a power of two: the grid times and every step size are exact in the time tensor's fp32
ALPHA, BETA = 0.3, -0.2
OPT = {'hidden_dim': 0, 'block': 'constant', 'add_source': True, 'no_alpha_sigmoid': False, 'max_nfe': 10 ** 6,
       'multi_modal': False}
# a state the integrator keeps in the user numbering, and the smallest one it renumbers
# (ops.LAYOUT_MIN_ROWS rows, 16 MB: the node layout and out_rows are in play)
SIZES = {"small": (2000, 14000), "layout": (32768, 230000)}


class Problem(object):
    def __init__(self, name):
        N, E = SIZES[name]
        self.N, self.C = N, 128
        self.ei, self.w = synthetic.rw_graph(N, E, seed=11, device=DEV)
        self.x = synthetic.features(1, N, self.C, seed=12, device=DEV)
        self.x0 = synthetic.features(1, N, self.C, seed=13, device=DEV)
        self.chains = {}

    def func(self):
        f = gnpde.LaplacianODEFunc(self.C, self.C, dict(OPT, hidden_dim=self.C), DEV).to(DEV)
        with torch.no_grad():
            f.alpha_train.fill_(ALPHA)
            f.beta_train.fill_(BETA)
        f.edge_index, f.edge_weight, f.x0 = self.ei, self.w, self.x0
        return f

    def chain(self, n):
        """The state after 1 .. n default _fused_step calls (new tensors, user numbering): computed once."""
        have = self.chains.get('y', [])
        if len(have) < n:
            f = self.func()
            ws = gi._Workspace()
            y = self.x if not have else have[-1]
            with torch.no_grad():
                for k in range(len(have), n):
                    y1 = gi._fused_step('rk4', f, k * DT, DT, (k + 1) * DT, y, ws)
                    assert y1.data_ptr() != y.data_ptr()
                    have.append(y1)
                    y = y1
            self.chains['y'] = have
        return have


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = Problem(name)
    return _problems[name]


def solve(func, pr, times, graph):
    with torch.no_grad():
        z = gnpde.odeint(func, pr.x, torch.tensor(times, device=DEV), method='rk4',
                         options={'step_size': DT, 'gnpde_graph': graph})
    torch.cuda.synchronize()
    return z


STEPS = (1, 2, 6, 7, 13)  # both sides of GRAPH_MIN_STEPS, odd and even


@pytest.mark.parametrize("graph", (False, True), ids=("eager", "replayed"))
@pytest.mark.parametrize("n", STEPS)
@pytest.mark.parametrize("size", ("small", "layout"))
def test_solve_equals_the_chain_of_default_steps(size, n, graph):
    assert gi.GRAPH_MIN_STEPS in range(min(STEPS) + 1, max(STEPS))
    pr = problem(size)
    assert gi.RK4_INPLACE
    func = pr.func()
    assert (func.node_layout(pr.x) is not None) == (size == "layout")
    keep = pr.x.clone()
    z = solve(func, pr, [0.0, n * DT], graph)
    want = pr.chain(n)[n - 1]
    assert torch.equal(z[0], keep) and torch.equal(pr.x, keep)  # the caller's y0 is never written
    assert torch.equal(z[1], want)
    # a second solve on the same module (its buffers and captured graphs reused): equal bits
    z2 = solve(func, pr, [0.0, n * DT], graph)
    assert torch.equal(z2[1], z[1]) and torch.equal(pr.x, keep)


@pytest.mark.parametrize("graph", (False, True), ids=("eager", "replayed"))
@pytest.mark.parametrize("size", ("small", "layout"))
def test_two_output_times(size, graph):
    pr = problem(size)
    func = pr.func()
    z = solve(func, pr, [0.0, 6 * DT, 13 * DT], graph)
    ys = pr.chain(13)
    assert torch.equal(z[1], ys[5]) and torch.equal(z[2], ys[12])
    # an output time inside a step: interpolated between the states around it (torchdiffeq)
    z = solve(func, pr, [0.0, 6.5 * DT, 13 * DT], graph)
    assert torch.equal(z[2], ys[12])
    mid = ys[5] + 0.5 * (ys[6] - ys[5])
    assert float((z[1] - mid).abs().max()) <= 1e-5 * float(mid.abs().max())


def test_inplace_step_equals_the_default_step():
    pr = problem("small")
    f = pr.func()
    with torch.no_grad():
        want = gi._fused_step('rk4', f, 0.0, DT, DT, pr.x, gi._Workspace())
        y = pr.x.clone()
        got = gi._fused_step('rk4', f, 0.0, DT, DT, y, gi._Workspace(), inplace=True)
        assert got.data_ptr() == y.data_ptr() and torch.equal(y, want)
        y, out = pr.x.clone(), torch.empty_like(pr.x)
        gi._fused_step('rk4', f, 0.0, DT, DT, y, gi._Workspace(), out=out, inplace=True)
        assert torch.equal(out, want) and torch.equal(y, pr.x)  # with ``out`` the input is left alone


def _rhs(pr, g, x, stage):
    wc = g.gather_weights(pr.w)
    a, b = torch.tensor(ALPHA, device=DEV), torch.tensor(BETA, device=DEV)
    return ops.spmm_rhs(g, wc, x, pr.x0, a, b, add_source=True, stage=stage)


def test_stage_aliasing_rule():
    pr = problem("small")
    g = ops.GraphCSR(pr.ei, pr.N)
    k = synthetic.features(1, pr.N, pr.C, seed=21, device=DEV)
    base = synthetic.features(1, pr.N, pr.C, seed=22, device=DEV)
    out = torch.empty_like(k)
    _rhs(pr, g, pr.x, ops.Stage(outs=[(out, base, -1.0, DT, [(k, 2.0)])]))
    # the output over a k operand
    k2 = k.clone()
    _rhs(pr, g, pr.x, ops.Stage(outs=[(k2, base, -1.0, DT, [(k2, 2.0)])]))
    assert torch.equal(k2, out)
    # the output over its base
    b2 = base.clone()
    _rhs(pr, g, pr.x, ops.Stage(outs=[(b2, b2, -1.0, DT, [(k, 2.0)])]))
    assert torch.equal(b2, out)
    # not through out_rows
    perm = torch.from_numpy(np.random.default_rng(3).permutation(pr.N).astype(np.int32)).to(DEV)
    k3, b3 = k.clone(), base.clone()
    with pytest.raises(ValueError, match="out_rows"):
        _rhs(pr, g, pr.x, ops.Stage(outs=[(k3, base, -1.0, DT, [(k3, 2.0)])], out_rows=perm))
    with pytest.raises(ValueError, match="out_rows"):
        _rhs(pr, g, pr.x, ops.Stage(outs=[(b3, b3, -1.0, DT, [(k, 2.0)])], out_rows=perm))
    assert torch.equal(k3, k) and torch.equal(b3, base)
    # the library refuses the same struct (a caller of the C ABI)
    st = ops.Stage(outs=[(k3, base, -1.0, DT, [(k3, 2.0)])]).struct(pr.x.view(-1, pr.C))
    st.out_rows = perm.data_ptr()
    wc = g.gather_weights(pr.w)
    a, b = torch.tensor(ALPHA, device=DEV), torch.tensor(BETA, device=DEV)
    plan = g.csr.plan
    rc = _lib.call_rc("gnpde_spmm_rhs_f32", ops._ptr(plan.items), plan.n_items, ops._ptr(plan.heavy), plan.n_heavy,
                      ops._ptr(g.csr.col), ops._ptr(wc), pr.C, ops._ptr(pr.x), pr.C, ops._ptr(pr.x0), pr.C,
                      ops._ptr(a), ops._ptr(b), ops._flags(True, True, True), None, pr.C,
                      ops._ptr(ops._partials(plan, pr.C, pr.x.device)), plan.n_slots, ctypes.byref(st),
                      ops._stream(pr.x.device))
    assert rc == _lib.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(k3, k)
    # never the RHS input
    x = pr.x.clone()
    with pytest.raises(ValueError, match="RHS input"):
        _rhs(pr, g, x, ops.Stage(outs=[(x, base, 1.0, DT, [])]))
    assert torch.equal(x, pr.x)
