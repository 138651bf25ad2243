"""Host-side logic of the multistep solvers (explicit_adams / implicit_adams) on CPU float64,
with the torch stage combiner injected (the product path combines on the GPU): coefficient
tables, the solver loop against the numpy oracle (tests/adams_oracle.py), non-convergence,
gradients through the explicit solve and through odeint_adjoint, and the opt-in."""
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

import adams_oracle as AO
import gnpde
from gnpde import adams_coefficients as AC
from gnpde import integrator as gode

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 6, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'implicit_adams', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': False, 'max_nfe': 1000,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16}

METHODS = ('explicit_adams', 'implicit_adams')


class LinearRHS(object):
    """f(t, y) = y A^T with a call counter (6 x 6, as tests/test_host_logic.py's linear RHS)."""

    def __init__(self, seed=5, scale=0.5):
        rng = np.random.default_rng(seed)
        self.A = rng.standard_normal((6, 6)) * scale
        self.y0 = rng.standard_normal(6)
        self.At = torch.from_numpy(self.A)
        self.nfe = 0

    def __call__(self, t, y):
        self.nfe += 1
        return y @ self.At.T

    def np(self, t, y):
        return y @ self.A.T


def _solve(rhs, method, ts, step, y0=None, **kw):
    opts = dict(gnpde_adams=True, step_size=step)
    opts.update({k: kw.pop(k) for k in ('max_order', 'max_iters') if k in kw})
    rhs.nfe = 0
    y0 = torch.from_numpy(rhs.y0) if y0 is None else y0
    return gode.odeint(rhs, y0, torch.tensor(ts, dtype=torch.float64), method=method, options=opts,
                       combine=gode._torch_combine, **kw)


def test_coefficient_tables_match_the_fraction_formula():
    assert AC.MAX_ORDER == 12 and sorted(AC.ADAMS_BASHFORTH) == sorted(AC.ADAMS_MOULTON) == list(range(1, 13))
    for k in range(1, 13):
        assert AC.ADAMS_BASHFORTH[k] == tuple(float(c) for c in AO.bashforth(k))
        assert AC.ADAMS_MOULTON[k] == tuple(float(c) for c in AO.moulton(k))
        assert sum(AO.bashforth(k)) == 1 and sum(AO.moulton(k)) == 1  # both integrate constants exactly
    assert AO.bashforth(3) == [Fraction(23, 12), Fraction(-16, 12), Fraction(5, 12)]
    assert AO.moulton(4) == [Fraction(9, 24), Fraction(19, 24), Fraction(-5, 24), Fraction(1, 24)]
    assert sum(abs(c) for c in AC.ADAMS_BASHFORTH[11]) == pytest.approx(591.27, abs=5e-3)
    assert AC.ADAMS_MOULTON[12][0] == pytest.approx(0.274266, abs=5e-7)
    assert gode.MULTISTEP_METHODS == METHODS


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("max_order", [3, 4, 5, 12])
def test_solver_matches_oracle(method, max_order):
    """Values at output times off the grid, the RHS count and the corrector iteration counts."""
    rhs = LinearRHS()
    # 20 steps of 0.025: the order-11 predictor is unstable on this spectrum (|lambda| <= 1.16) and
    # amplifies the rounding differences of the two matrix products; here they stay below 1e-14
    ts, step = [0.0, 0.07, 0.3, 0.5], 0.025
    rtol, atol = 1e-6, 1e-8
    want = AO.solve(rhs.np, rhs.y0, AO.grid(ts[0], ts[-1], step), method, rtol, atol, max_order=max_order, times=ts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # max_order 3: the all-rk4 warning (checked below)
        got = _solve(rhs, method, ts, step, rtol=rtol, atol=atol, max_order=max_order).numpy()
    assert got.shape == (4, 6)
    assert np.abs(got - want.sol).max() <= 1e-12
    assert rhs.nfe == want.nfe
    assert gode.odeint.last_adams['iterations'] == want.iterations
    assert gode.odeint.last_adams['converged'] == want.converged
    assert gode.odeint.last_path == 'adams_restated'
    if max_order == 3:
        assert want.nfe == 4 * len(want.iterations)  # every step an rk4 step
    elif method == 'explicit_adams':
        assert want.nfe == 4 * 2 + (len(want.iterations) - 2)  # two rk4 start steps, then one RHS per step
    else:
        assert max(want.iterations) >= 2 and want.iterations[:2] == [0, 0]
    # the oracle itself follows the exact flow: the least accurate case, the third-order predictor
    # alone, has a global error near (3/8) h^3 |lambda|^4 |y| T ~ 1e-5 here
    import scipy.linalg
    exact = scipy.linalg.expm(rhs.A * ts[-1]) @ rhs.y0
    assert np.abs(want.y - exact).max() <= 1e-4


def test_max_iters_one_never_converges():
    """max_iters = 1 at dt 0.25: every Adams step fails the test, the warning fires, the history
    drops its oldest entry and the values still follow the oracle."""
    rhs = LinearRHS()
    ts = [0.0, 4.0]
    want = AO.solve(rhs.np, rhs.y0, AO.grid(0.0, 4.0, 0.25), 'implicit_adams', 1e-7, 1e-9, max_order=6, max_iters=1,
                    times=ts)
    adams_steps = [i for i, n in enumerate(want.iterations) if n]
    assert len(adams_steps) == len(want.iterations) - 2
    assert not any(want.converged[i] for i in adams_steps)
    assert min(r for rs in want.ratios for r in rs) > 1.5  # far from the threshold: not a rounding matter
    with pytest.warns(UserWarning, match="did not converge") as rec:
        got = _solve(rhs, 'implicit_adams', ts, 0.25, rtol=1e-7, atol=1e-9, max_order=6, max_iters=1).numpy()
    assert len([w for w in rec if "did not converge" in str(w.message)]) == 1  # once per solve
    assert np.abs(got - want.sol).max() <= 1e-12
    assert gode.odeint.last_adams['converged'] == want.converged and rhs.nfe == want.nfe
    # dropping the oldest entry changes the result: the same solve keeping it differs
    keep = AO.solve(rhs.np, rhs.y0, AO.grid(0.0, 4.0, 0.25), 'implicit_adams', 1e-7, float('inf'), max_order=6,
                    max_iters=1)
    assert all(keep.converged) and np.abs(keep.y - want.y).max() > 1e-9


def test_nan_ratio_is_not_converged():
    f = lambda t, y: y * float('nan') if t > 0.6 else -y  # noqa: E731
    with pytest.warns(UserWarning, match="did not converge"):
        gode.odeint(f, torch.ones(3, dtype=torch.float64), torch.tensor([0.0, 1.0], dtype=torch.float64),
                    method='implicit_adams', options=dict(gnpde_adams=True, step_size=0.25, max_order=4),
                    combine=gode._torch_combine)
    assert gode.odeint.last_adams['converged'][-1] is False
    assert np.isnan(gode.odeint.last_adams['ratios'][-1])


def test_explicit_solve_under_autograd():
    """explicit_adams is linear in y0: d sum(y(T)) / d y0 is the column sum of the step operator,
    which the oracle gives on the identity basis."""
    rhs = LinearRHS()
    y0 = torch.from_numpy(rhs.y0).requires_grad_(True)
    out = _solve(rhs, 'explicit_adams', [0.0, 2.0], 0.125, y0=y0, max_order=8)
    out[-1].sum().backward()
    basis = AO.solve(rhs.np, np.eye(6), AO.grid(0.0, 2.0, 0.125), 'explicit_adams', max_order=8).y  # row i: e_i's image
    assert np.abs(y0.grad.numpy() - basis.sum(axis=1)).max() <= 1e-10


def test_odeint_adjoint_matches_oracle_augmented_system():
    """odeint_adjoint with method = adjoint_method = 'implicit_adams': the y0-gradient of
    sum(y(T)) against the oracle integrating the same augmented system (y, a) over s = -t,
    dy/ds = -y A^T, da/ds = a A, from (y(T), 1) — _OdeintAdjoint's construction without
    parameters."""
    rhs = LinearRHS()
    T, step, rtol, atol = 1.5, 0.125, 1e-6, 1e-8
    opts = dict(gnpde_adams=True, step_size=step, max_order=6, max_iters=8)
    y0 = torch.from_numpy(rhs.y0).requires_grad_(True)
    out = gode.odeint_adjoint(rhs, y0, torch.tensor([0.0, T], dtype=torch.float64), rtol=rtol, atol=atol,
                              method='implicit_adams', options=opts, adjoint_method='implicit_adams',
                              adjoint_options=dict(opts), adjoint_params=(), combine=gode._torch_combine)
    fwd = AO.solve(rhs.np, rhs.y0, AO.grid(0.0, T, step), 'implicit_adams', rtol, atol, max_order=6, max_iters=8)
    assert np.abs(out[-1].detach().numpy() - fwd.y).max() <= 1e-12
    out[-1].sum().backward()

    def aug(s, z):
        return np.concatenate([-(z[:6] @ rhs.A.T), z[6:] @ rhs.A])
    z0 = np.concatenate([out[-1].detach().numpy(), np.ones(6)])
    back = AO.solve(aug, z0, AO.grid(-T, -0.0, step), 'implicit_adams', rtol, atol, max_order=6, max_iters=8)
    assert max(back.iterations) >= 1
    assert np.abs(y0.grad.numpy() - back.y[6:]).max() <= 1e-9
    # and the adjoint is the gradient of the flow up to the discretisation
    import scipy.linalg
    assert np.abs(y0.grad.numpy() - scipy.linalg.expm(rhs.A * T).T @ np.ones(6)).max() <= 1e-3


def test_opt_in_and_option_checks():
    rhs = LinearRHS()
    t = torch.tensor([0.0, 1.0], dtype=torch.float64)
    y0 = torch.from_numpy(rhs.y0)
    for method in METHODS:
        with pytest.raises(NotImplementedError, match="gnpde_adams"):
            gode.odeint(rhs, y0, t, method=method, options=dict(step_size=0.25), combine=gode._torch_combine)
        with pytest.raises(NotImplementedError, match="gnpde_adams"):
            gode.odeint_adjoint(rhs, y0.clone().requires_grad_(True), t, method=method, options=dict(step_size=0.25),
                                adjoint_params=(), combine=gode._torch_combine)
        with pytest.raises(ValueError, match="max_order"):
            _solve(rhs, method, [0.0, 1.0], 0.25, max_order=13)
    with pytest.warns(UserWarning, match="rk4"):
        _solve(rhs, 'implicit_adams', [0.0, 1.0], 0.25, max_order=3)
    assert gode.odeint.last_adams['iterations'] == [0, 0, 0, 0]
    assert gode.FIXED_METHODS == ('euler', 'midpoint', 'rk4')
    assert gode.ADAPTIVE_METHODS == ('dopri5', 'bosh3', 'fehlberg2', 'adaptive_heun')


def test_max_nfe_raised_at_the_exact_call():
    class Guarded(LinearRHS):
        def __call__(self, t, y):
            if self.nfe > 9:
                raise gnpde.MaxNFEException
            return LinearRHS.__call__(self, t, y)
    rhs = Guarded()
    with pytest.raises(gnpde.MaxNFEException):
        _solve(rhs, 'explicit_adams', [0.0, 4.0], 0.25, max_order=4)
    assert rhs.nfe == 10  # two rk4 steps (8), two Adams steps, the next call raises


def test_block_passes_the_key():
    seen = {}

    def fake(func, x, t, **kw):
        seen.clear()
        seen.update(kw)
        return torch.stack([x, x])
    opt = dict(OPT, gnpde_adams=True, adjoint=True, adjoint_method='implicit_adams')
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], opt, None, t=torch.tensor([0, 1]))
    blk.train_integrator = blk.test_integrator = fake
    x = torch.ones(1, 3, 6)
    blk.eval()
    blk._integrate(x, dict(step_size=1, max_iters=5))
    assert seen['options'] == dict(step_size=1, max_iters=5, gnpde_adams=True) and 'adjoint_options' not in seen
    blk.train()
    blk._integrate(x, dict(step_size=1, max_iters=5))
    assert seen['options']['gnpde_adams'] is True
    assert seen['adjoint_options'] == dict(step_size=1, max_iters=5, gnpde_adams=True)
    assert seen['method'] == seen['adjoint_method'] == 'implicit_adams'
    blk.opt['max_order'] = 8
    blk._integrate(x, dict(step_size=1, max_iters=5))
    assert seen['options']['max_order'] == seen['adjoint_options']['max_order'] == 8
    plain = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], dict(OPT, adjoint=True), None, t=torch.tensor([0, 1]))
    plain.train_integrator = fake
    plain.train()
    plain._integrate(x, dict(step_size=1, max_iters=5))
    assert seen['options'] == dict(step_size=1, max_iters=5) == seen['adjoint_options']


def test_early_stop_and_sharded_solves_refuse_the_methods():
    es = gnpde.EarlyStopInt(1.0, dict(OPT, max_test_steps=10, earlystopxT=1))
    with pytest.raises(NotImplementedError, match="multistep"):
        es(None, torch.ones(1, 3, 2), None)
    with pytest.raises(NotImplementedError, match="early-stop"):
        gode.odeint(lambda t, y: -y, torch.ones(3, dtype=torch.float64), torch.tensor([0.0, 1.0]),
                    method='explicit_adams', combine=gode._torch_combine,
                    options=dict(gnpde_adams=True, step_size=0.25, gnpde_accept_hook=lambda *a: None))
    Sharded = type('Sharded', (), {'__module__': 'gnpde.dist', '__call__': lambda self, t, y: -y})
    with pytest.raises(NotImplementedError, match="gnpde.dist"):
        gode.odeint(Sharded(), torch.ones(3, dtype=torch.float64), torch.tensor([0.0, 1.0]), method='implicit_adams',
                    options=dict(gnpde_adams=True, step_size=0.25), combine=gode._torch_combine)
