"""CPU: the ODE regularisers' oracle and host logic (no GPU).

* tests/reg_oracle.py reproduces the reference's own values (tests/golden/reg/*.npz: its
  LaplacianODEFunc, quadratic_cost and total_derivative of f + 0*t) to 1e-12 relative;
* the oracle's analytic vector-Jacobian form v = a (A^T f - f) equals its double-backward form,
  values and gradients (x, alpha, beta, weights), at the RHS and through whole solves;
* create_regularization_fns: order, skipping, the keys that raise;
* ops.row_energy_torch / ops.row_axpy_torch against numpy;
* without opt['gnpde_regularization'] the regularised paths still raise, naming the key.
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import reg_oracle as RO
from conftest import GOLDEN
from gnpde import ops
from gnpde import regularized_ODE_function as R

FILES = sorted(glob.glob(os.path.join(GOLDEN, "reg", "*.npz")))


def _load(path):
    z = np.load(path)
    return z, json.loads(str(z["meta"]))


def _oracle_func(z, meta, grad=False):
    w = RO.t64(z["weights"], grad)
    alpha, beta = RO.t64(z["alpha_train"], grad), RO.t64(z["beta_train"], grad)
    func = RO.Laplacian(z["edge_index"], w, meta["N"], alpha, beta, x0=RO.t64(z["x0"]),
                        add_source=meta["add_source"], no_alpha_sigmoid=meta["no_alpha_sigmoid"])
    return func


def test_golden_files_present():
    assert len(FILES) >= 3
    metas = [_load(p)[1] for p in FILES]
    assert {m["B"] for m in metas} == {1, 2}


@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_oracle_reproduces_reference(path):
    z, meta = _load(path)
    ei = z["edge_index"]
    # the fixtures' graphs hold what they promise: duplicates and isolated rows
    for b in range(meta["B"]):
        pairs = set(zip(ei[b, 0].tolist(), ei[b, 1].tolist()))
        assert len(pairs) < ei.shape[2]
        assert len(set(ei[b].reshape(-1).tolist())) < meta["N"]
    func = _oracle_func(z, meta)
    x = RO.t64(z["x"], True)
    f = func(0.0, x)
    for dbl in (True, False):
        got = {"f": f, "kinetic": RO.quadratic_cost(x, 0.0, f, func),
               "directional": RO.directional_derivative(x, 0.0, f, func, double_backward=dbl)}
        for k, v in got.items():
            want = z[k]
            err = np.abs(v.detach().numpy() - want).max() / np.abs(want).max()
            assert err <= 1e-12, (k, dbl, err)


def _grads(path, dbl, solve):
    z, meta = _load(path)
    func = _oracle_func(z, meta, grad=True)
    x = RO.t64(z["x"], True)
    rng = np.random.default_rng(5)
    if solve is None:
        f = func(0.0, x)
        vals = (f, RO.quadratic_cost(x, 0.0, f, func), RO.directional_derivative(x, 0.0, f, func, dbl))
    else:
        zT, regs = RO.solve(func, ('kinetic', 'directional'), x, 0.0, 0.6, 2, solve, double_backward=dbl)
        vals = (zT,) + regs
    loss = sum((RO.t64(rng.standard_normal(v.shape)) * v).sum() for v in vals)
    gs = torch.autograd.grad(loss, [x, func.alpha, func.beta, func.w], allow_unused=True)
    return [v.detach().numpy() for v in vals], [None if g is None else g.numpy() for g in gs]


@pytest.mark.parametrize("solve", [None, 'euler', 'midpoint', 'rk4'])
@pytest.mark.parametrize("path", FILES, ids=[os.path.basename(p)[:-4] for p in FILES])
def test_analytic_vjp_equals_double_backward(path, solve):
    va, ga = _grads(path, False, solve)
    vd, gd = _grads(path, True, solve)
    for a, d in zip(va + ga, vd + gd):
        assert (a is None) == (d is None)
        if a is not None:
            assert np.abs(a - d).max() <= 1e-12 * max(np.abs(d).max(), 1e-300)


def test_create_regularization_fns():
    fns, coeffs = R.create_regularization_fns({'directional_penalty': 0.5, 'kinetic_energy': 0.25,
                                               'jacobian_norm2': None, 'total_deriv': None})
    assert fns == [R.quadratic_cost, R.directional_derivative] and coeffs == [0.25, 0.5]
    assert R.create_regularization_fns({}) == ([], [])
    assert R.create_regularization_fns({'kinetic_energy': None, 'directional_penalty': 1.0}) == \
        ([R.directional_derivative], [1.0])
    for key in ('jacobian_norm2', 'total_deriv'):
        with pytest.raises(NotImplementedError, match=key):
            R.create_regularization_fns({'kinetic_energy': 1.0, key: 0.1})
    assert gnpde.create_regularization_fns is R.create_regularization_fns
    from gnpde import base_classes
    assert base_classes.RegularizedODEfunc is R.RegularizedODEfunc


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (2, 7, 12)])
def test_row_passes_torch_vs_numpy(shape):
    rng = np.random.default_rng(3)
    ks = [rng.standard_normal(shape).astype(np.float32) for _ in range(3)]
    cs = [0.5, 0.25, 2.0]
    want = sum(c * (k.astype(np.float64) ** 2).sum(-1) for c, k in zip(cs, ks))
    tk = [torch.from_numpy(k) for k in ks]
    got = ops.row_energy_torch(tk, cs)
    assert got.dtype == torch.float32 and got.shape == shape[:-1]
    # float64 sums of at most 36 terms in another order: 36 * 2^-53 relative, then one fp32 rounding
    assert np.abs(got.numpy() - want).max() <= np.spacing(np.float32(np.abs(want).max()))
    acc = torch.ones(int(np.prod(shape[:-1])), dtype=torch.float64)
    ops.row_energy_torch(tk, cs, acc=acc, accumulate=True)
    assert np.abs(acc.numpy() - (1.0 + want.reshape(-1))).max() <= 1e-14 * np.abs(want).max()
    ops.row_energy_torch(tk[:1], cs[:1], acc=acc)
    one = (cs[0] * (ks[0].astype(np.float64) ** 2).sum(-1)).reshape(-1)
    assert np.abs(acc.numpy() - one).max() <= 1e-14 * np.abs(one).max()  # stored, not added to
    g = [rng.standard_normal(shape[:-1]).astype(np.float32), rng.standard_normal(shape[:-1]).astype(np.float32)]
    wa = ks[0].astype(np.float64) + 0.3 * g[0][..., None].astype(np.float64) * ks[1] \
        - 1.5 * g[1][..., None].astype(np.float64) * ks[2]
    ga = ops.row_axpy_torch(tk[0], [(0.3, torch.from_numpy(g[0]), tk[1]), (-1.5, torch.from_numpy(g[1]), tk[2])])
    assert np.abs(ga.numpy() - wa).max() <= np.spacing(np.float32(np.abs(wa).max()))
    gn = ops.row_axpy_torch(None, [(2.0, torch.from_numpy(g[0]).double(), tk[1])])
    assert np.array_equal(gn.numpy(), (2.0 * g[0][..., None].astype(np.float64) * ks[1]).astype(np.float32))


class _Const(torch.nn.Module):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt

    def forward(self, t, x):
        return -x


def test_without_the_opt_in_key_it_still_raises():
    opt = {'hidden_dim': 4, 'method': 'euler', 'step_size': 0.5, 'max_nfe': 100, 'add_source': False,
           'no_alpha_sigmoid': False, 'block': 'constant', 'multi_modal': False}
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [R.quadratic_cost], opt, 'cpu', torch.tensor([0.0, 1.0]))
    assert blk.nreg == 1
    blk.train()
    with pytest.raises(NotImplementedError, match="gnpde_regularization"):
        blk._integrate(torch.zeros(1, 3, 4), {'step_size': 0.5})
    with pytest.raises(NotImplementedError, match="gnpde_regularization"):
        blk.reg_odefunc(torch.tensor(0.0), (torch.zeros(1, 3, 4), torch.zeros(1, 3)))
    # the holder keeps the reference's attribute path and state_dict keys
    keys = set(blk.state_dict())
    assert {'odefunc.alpha_train', 'reg_odefunc.odefunc.alpha_train'} <= keys


def test_regularized_rhs_calls_every_fn_in_order():
    seen = []

    def fn_a(x, t, dx, odefunc):
        seen.append('a')
        return dx.sum(-1)

    def fn_b(x, t, dx, odefunc):
        seen.append('b')
        return x.sum(-1)

    f = _Const({R.OPT_KEY: True})
    reg = R.RegularizedODEfunc(f, [fn_a, fn_b])
    x = torch.arange(6.0).view(1, 2, 3)
    out = reg(torch.tensor(0.0), (x, torch.zeros(1, 2), torch.zeros(1, 2)))
    assert seen == ['a', 'b'] and len(out) == 3
    assert torch.equal(out[0], -x) and torch.equal(out[1], (-x).sum(-1)) and torch.equal(out[2], x.sum(-1))
    other = _Const({R.OPT_KEY: True})
    assert torch.equal(reg.bound(other)(0.0, (x, torch.zeros(1, 2)))[0], -x)


def test_tuple_state_out_of_scope_cases_raise():
    from gnpde import integrator as gode
    f = _Const({R.OPT_KEY: True})
    reg = R.RegularizedODEfunc(f, [lambda x, t, dx, o: dx.sum(-1)])
    st = (torch.zeros(1, 2, 3), torch.zeros(1, 2))
    t = torch.tensor([0.0, 1.0])
    for method, word in (('dopri5', 'adaptive'), ('explicit_adams', 'multistep'), ('implicit_adams', 'multistep')):
        with pytest.raises(NotImplementedError, match=word):
            gode.odeint(reg, st, t, method=method, options={'step_size': 0.5, 'gnpde_adams': True},
                        combine=gode._torch_combine)
    with pytest.raises(NotImplementedError, match="adjoint"):
        gode.odeint_adjoint(reg, st, t, method='euler', options={'step_size': 0.5})
    with pytest.raises(NotImplementedError, match="bf16"):
        gode.odeint(reg, (st[0].bfloat16(), st[1]), t, method='euler', options={'step_size': 0.5},
                    combine=gode._torch_combine)


@pytest.mark.parametrize("method", ['euler', 'midpoint', 'rk4'])
def test_tuple_state_fixed_grid_on_cpu(method):
    """The per-RHS tuple-state loop against the oracle's stepper, on an injected CPU RHS."""
    from gnpde import integrator as gode
    f = _Const({R.OPT_KEY: True})
    reg = R.RegularizedODEfunc(f, [lambda x, t, dx, o: 0.5 * dx.pow(2).mean(-1)])
    x = torch.linspace(-1, 1, 6, dtype=torch.float64).view(1, 2, 3)
    out = gode.odeint(reg, (x, torch.zeros(1, 2, dtype=torch.float64)), torch.tensor([0.0, 1.0], dtype=torch.float64),
                      method=method, options={'step_size': 0.25}, combine=gode._torch_combine)
    assert gode.odeint.last_reg_path == 'restated'
    assert isinstance(out, tuple) and out[0].shape == (2, 1, 2, 3) and out[1].shape == (2, 1, 2)

    def rhs(t, s):
        return (-s[0], 0.5 * s[0].pow(2).mean(-1))
    y = (x, torch.zeros(1, 2, dtype=torch.float64))
    for i in range(4):
        y = RO.step(method, rhs, 0.25 * i, 0.25, y)
    assert torch.allclose(out[0][1], y[0], rtol=1e-14, atol=0) and torch.allclose(out[1][1], y[1], rtol=1e-14, atol=0)
    assert torch.equal(out[0][0], x) and torch.equal(out[1][0], torch.zeros(1, 2, dtype=torch.float64))
