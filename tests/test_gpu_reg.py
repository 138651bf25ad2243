"""GPU: the ODE regularisers (opt['gnpde_regularization']) — the row passes of
csrc/regularizers.hip against float64 numpy, the regularised right-hand side and whole training
solves against the float64 torch oracle (tests/reg_oracle.py: dense A, the directional term by
autograd.grad(dx, x, dx, create_graph=True)).

Tolerances.
* row_energy, fp64 form, non-negative coefficients: 1e-12 relative — at most 1024 non-negative
  fp64 terms per row (4 arrays x 256 columns), so the error is at most 1024 * 2^-53 = 1.2e-13.
* row_energy, fp32 form, and row_axpy: one fp32 ulp of the extended-precision value (each stored
  value is an fp64 sum rounded once), as tests/test_gpu_adams.py.
* values 1e-5 and gradients 1e-4 of max |.|: the project's parity and gradient bars.

The solve-level loss is sum(w*z) + c1*mean(r1) + c2*mean(r2) with c_j = B*N*C/2, so that the
regularisers' part of every gradient is of the size of the state's part and an error in it cannot
hide below the bar; the gradients of the regularisers' part alone are checked as well.
"""
import numpy as np
import pytest
import torch

import gnpde
import reg_oracle as RO
from gnpde import integrator as gode
from gnpde import ops
from gnpde import regularized_ODE_function as R
from test_gpu_parity import DEV, OPT, T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (64, 128), (33, 256), (257, 162)]
VTOL, GTOL = 1e-5, 1e-4
LD = np.longdouble


def _ulp(ref):
    return np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _within_ulp(got, ref):
    got = got.double().cpu().numpy().reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    return bool((np.abs(got - ref) <= _ulp(ref)).all())


def _dev(a, offset=0):
    """A device copy of ``a``; offset=1: its base 4 bytes past a 16-byte boundary."""
    a = np.ascontiguousarray(a)
    if not offset:
        return T(a)
    buf = torch.empty(a.size + 4, dtype=torch.float32, device=DEV)
    lead = (offset - (buf.data_ptr() % 16) // 4) % 4
    out = buf[lead:lead + a.size].view(a.shape)
    out.copy_(torch.from_numpy(a))
    assert out.data_ptr() % 16 == 4 * offset
    return out


# ---------------------------------------------------------------- kernels
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_row_energy_vs_float64(shape, offset):
    Rr, C = shape
    rng = np.random.default_rng(100 * Rr + C)
    ks = [rng.standard_normal(shape).astype(np.float32) for _ in range(4)]
    cs = [0.5 / C, 0.0, 0.375, 2.0]
    dks = [_dev(k, offset) for k in ks]
    prev = rng.uniform(0.0, 3.0, Rr)
    for n in (1, 2, 3, 4):
        want = sum(LD(c) * (k.astype(LD) ** 2).sum(-1) for c, k in zip(cs[:n], ks[:n]))
        for accumulate in (False, True):
            acc = T(prev.copy())
            out = ops.row_energy(dks[:n], cs[:n], acc=acc, accumulate=accumulate)
            assert out is acc
            ref = (want + prev if accumulate else want).astype(np.float64)
            err = np.abs(acc.cpu().numpy() - ref)
            assert (err <= 1e-12 * np.abs(ref)).all(), (n, accumulate, float((err / np.maximum(ref, 1e-300)).max()))
            again = T(prev.copy())
            ops.row_energy(dks[:n], cs[:n], acc=again, accumulate=accumulate)
            assert torch.equal(acc, again)
        e32 = ops.row_energy(dks[:n], cs[:n])
        assert e32.shape == (Rr,) and e32.dtype == torch.float32
        assert _within_ulp(e32, want.astype(np.float64))
        assert torch.equal(e32, ops.row_energy(dks[:n], cs[:n]))
        assert _within_ulp(ops.row_energy_torch(dks[:n], cs[:n]), want.astype(np.float64))


def test_row_energy_bits_do_not_depend_on_alignment_or_batch_shape():
    rng = np.random.default_rng(7)
    k = rng.standard_normal((2, 37, 128)).astype(np.float32)
    a = ops.row_energy([_dev(k)], [1.0])
    assert a.shape == (2, 37)
    # the scalar form sums a row's columns in another order: equal to one ulp, and the row owner
    # and order are fixed by the row length alone, so a flattened view gives the same bits
    assert _within_ulp(ops.row_energy([_dev(k, 1)], [1.0]), a.double().cpu().numpy())
    assert torch.equal(a.view(-1), ops.row_energy([_dev(k.reshape(74, 128))], [1.0]))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_row_axpy_vs_float64(shape, offset):
    Rr, C = shape
    rng = np.random.default_rng(200 * Rr + C)
    base, s0, s1 = (rng.standard_normal(shape).astype(np.float32) for _ in range(3))
    g0, g1 = rng.standard_normal(Rr).astype(np.float32), rng.standard_normal(Rr)
    c0, c1 = 0.3, -1.7
    db, d0, d1 = _dev(base, offset), _dev(s0, offset), _dev(s1, offset)
    t0 = c0 * g0.astype(LD)[:, None] * s0.astype(LD)
    t1f = c1 * g1.astype(np.float32).astype(LD)[:, None] * s1.astype(LD)
    t1d = c1 * g1.astype(LD)[:, None] * s1.astype(LD)
    # one term, no base, fp32 g
    out = ops.row_axpy(None, [(c0, T(g0), d0)])
    assert _within_ulp(out, t0.astype(np.float64))
    assert torch.equal(out, ops.row_axpy(None, [(c0, T(g0), d0)]))
    # two terms on a base, fp32 g
    out = ops.row_axpy(db, [(c0, T(g0), d0), (c1, T(g1.astype(np.float32)), d1)])
    want = (base.astype(LD) + t0 + t1f).astype(np.float64)
    assert _within_ulp(out, want)
    assert _within_ulp(ops.row_axpy_torch(db, [(c0, T(g0), d0), (c1, T(g1.astype(np.float32)), d1)]), want)
    # fp64 g, in place over the base
    keep = db.clone() if not offset else _dev(base, offset)
    res = ops.row_axpy(keep, [(c0, T(g0.astype(np.float64)), d0), (c1, T(g1), d1)], out=keep)
    assert res is keep
    assert _within_ulp(keep, (base.astype(LD) + t0 + t1d).astype(np.float64))


def test_row_passes_reject_bad_arguments():
    x = torch.zeros(4, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.row_energy([x] * 5, [1.0] * 5)
    with pytest.raises(ValueError):
        ops.row_energy([torch.zeros(4, 257, device=DEV)], [1.0])
    with pytest.raises(ValueError):
        ops.row_energy([x], [1.0], acc=torch.zeros(3, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        ops.row_axpy(None, [(1.0, torch.zeros(3, device=DEV), x)])
    with pytest.raises(gnpde._lib.GnpdeError):
        ops.row_axpy(None, [(1.0, torch.zeros(4, device=DEV), x)], out=x)


# ---------------------------------------------------------------- shared cases
def _case(B, C, seed, N=150, E=900):
    rng = np.random.default_rng(seed)
    ei = RO.hub_graph(rng, B, N, E, hub_edges=300, dup=40)
    w = rng.uniform(0.05, 0.4, (B, E)).astype(np.float32)
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    x0 = rng.standard_normal((B, N, C)).astype(np.float32)
    return dict(B=B, N=N, C=C, ei=ei, w=w, x=x, x0=x0, alpha=float(np.float32(0.3)), beta=float(np.float32(0.6)),
                rng=rng)


def _opt(C, **kw):
    return dict(OPT, hidden_dim=C, gnpde_regularization=True, **kw)


def _set(func, c, w_grad):
    with torch.no_grad():
        func.alpha_train.fill_(c['alpha'])
        func.beta_train.fill_(c['beta'])
    func.edge_index = T(c['ei'])
    func.edge_weight = T(c['w']).requires_grad_(w_grad)
    func.x0 = T(c['x0'])


def _oracle(c, add_source, no_alpha_sigmoid):
    w = RO.t64(c['w'], True)
    return RO.Laplacian(c['ei'], w, c['N'], RO.t64(c['alpha'], True), RO.t64(c['beta'], True), x0=RO.t64(c['x0']),
                        add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid)


def _close(got, want, tol, what):
    if want is None:
        assert got is None or float(got.abs().max()) == 0.0, what
        return
    want = want.detach().numpy()
    err = np.abs(got.detach().double().cpu().numpy() - want).max() / max(np.abs(want).max(), 1e-30)
    assert err <= tol, (what, err)


# ---------------------------------------------------------------- RHS level
@pytest.mark.parametrize("add_source,no_alpha_sigmoid", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("C", [5, 128, 162])
@pytest.mark.parametrize("B", [1, 2])
def test_regularized_rhs_vs_oracle(B, C, add_source, no_alpha_sigmoid):
    c = _case(B, C, 1000 * B + C)
    opt = _opt(C, add_source=add_source, no_alpha_sigmoid=no_alpha_sigmoid)
    func = gnpde.LaplacianODEFunc(C, C, opt, DEV).to(DEV)
    _set(func, c, True)
    reg = R.RegularizedODEfunc(func, [R.quadratic_cost, R.directional_derivative])
    x = T(c['x']).requires_grad_(True)
    zeros = torch.zeros(B, c['N'], device=DEV)
    got = reg(torch.tensor(0.0), (x, zeros, zeros))
    of = _oracle(c, add_source, no_alpha_sigmoid)
    xo = RO.t64(c['x'], True)
    want = RO.reg_rhs(of, ('kinetic', 'directional'))(0.0, (xo, None, None))
    assert len(got) == 3 and got[1].shape == (B, c['N']) and got[2].shape == (B, c['N'])
    ws = [c['rng'].standard_normal(v.shape) for v in want]
    for g, w_, name in zip(got, want, ('f', 'kinetic', 'directional')):
        _close(g, w_, VTOL, name)
    loss = sum((T(w_).float() * g).sum() for w_, g in zip(ws, got))
    loss_o = sum((RO.t64(w_) * v).sum() for w_, v in zip(ws, want))
    gg = torch.autograd.grad(loss, [x, func.alpha_train, func.beta_train, func.edge_weight], allow_unused=True)
    go = torch.autograd.grad(loss_o, [xo, of.alpha, of.beta, of.w], allow_unused=True)
    for g, w_, name in zip(gg, go, ('x', 'alpha_train', 'beta_train', 'edge_weight')):
        _close(g, w_, GTOL, 'grad ' + name)


def test_directional_penalty_needs_the_laplacian():
    C = 8
    opt = _opt(C, function='transformer', attention_dim=8, heads=2)
    func = gnpde.ODEFuncTransformerAtt(C, C, opt, DEV).to(DEV)
    x = torch.zeros(1, 4, C, device=DEV)
    with pytest.raises(NotImplementedError, match="directional_penalty"):
        R.directional_derivative(x, 0.0, x, func)
    assert R.quadratic_cost(x, 0.0, x + 1.0, func).shape == (1, 4)


# ---------------------------------------------------------------- solve level
KINDS = {'kinetic': R.quadratic_cost, 'directional': R.directional_derivative}
SOLVES = [  # kinds, method, steps, B, C, add_source
    (('kinetic',), 'euler', 2, 1, 128, False),
    (('directional',), 'euler', 3, 2, 162, True),
    (('kinetic', 'directional'), 'euler', 4, 2, 5, True),
    (('kinetic',), 'midpoint', 3, 2, 162, True),
    (('directional',), 'midpoint', 4, 1, 5, False),
    (('kinetic', 'directional'), 'midpoint', 2, 1, 128, True),
    (('kinetic',), 'rk4', 4, 2, 5, True),
    (('directional',), 'rk4', 2, 1, 128, False),
    (('kinetic', 'directional'), 'rk4', 3, 2, 162, True),
    (('directional', 'kinetic'), 'rk4', 2, 1, 128, True),
]


def _block(c, kinds, method, add_source, w_grad, cls=None, **kw):
    opt = _opt(c['C'], method=method, step_size=0.25, add_source=add_source, **kw)
    blk = (cls or gnpde.ConstantODEblock)(gnpde.LaplacianODEFunc, [KINDS[k] for k in kinds], opt, DEV,
                                          t=torch.tensor([0.0, 1.0])).to(DEV)
    _set(blk.odefunc, c, w_grad)
    blk.set_x0(T(c['x0']))
    return blk


def _solve_oracle(c, kinds, method, steps, add_source, ws, cj):
    of = _oracle(c, add_source, False)
    xo = RO.t64(c['x'], True)
    z, regs = RO.solve(of, kinds, xo, 0.0, 0.25 * steps, steps, method)
    reg_loss = sum(cj * r.mean() for r in regs)
    full = (RO.t64(ws) * z).sum() + reg_loss
    leaves = [xo, of.alpha, of.beta, of.w]
    return z, regs, torch.autograd.grad(full, leaves, allow_unused=True, retain_graph=True), \
        torch.autograd.grad(reg_loss, leaves, allow_unused=True)


@pytest.mark.parametrize("kinds,method,steps,B,C,add_source", SOLVES,
                         ids=["%s-%s%d-b%d-c%d" % ('+'.join(k[:3] for k in s[0]), s[1], s[2], s[3], s[4])
                              for s in SOLVES])
def test_constant_block_training_vs_oracle(kinds, method, steps, B, C, add_source):
    c = _case(B, C, 2000 * B + C + steps)
    ws = c['rng'].standard_normal((B, c['N'], C))
    cj = 0.5 * B * c['N'] * C
    zo, ro, go_full, go_reg = _solve_oracle(c, kinds, method, steps, add_source, ws, cj)
    for w_grad in (False, True):
        blk = _block(c, kinds, method, add_source, w_grad).train()
        blk.t = torch.tensor([0.0, 0.25 * steps], device=DEV)
        x = T(c['x']).requires_grad_(True)
        z, regs = blk(x, None)
        want_path = 'fused' if (method != 'midpoint' and not w_grad) else 'restated'
        assert gode.odeint.last_reg_path == want_path
        assert isinstance(regs, tuple) and len(regs) == len(kinds)
        _close(z, zo, VTOL, 'z')
        for r, r_o, k in zip(regs, ro, kinds):
            assert r.shape == (B, c['N']) and r.dtype == torch.float32
            _close(r, r_o, VTOL, k)
        f = blk.odefunc
        leaves = [x, f.alpha_train, f.beta_train] + ([f.edge_weight] if w_grad else [])
        names = ['x', 'alpha_train', 'beta_train', 'edge_weight']
        reg_loss = sum(cj * r.mean() for r in regs)
        full = (T(ws).float() * z).sum() + reg_loss
        for loss, want, tag in ((full, go_full, 'full'), (reg_loss, go_reg, 'reg only')):
            got = torch.autograd.grad(loss, leaves, allow_unused=True, retain_graph=True)
            for g, w_, name in zip(got, want, names):
                _close(g, w_, GTOL, '%s grad %s (%s)' % (tag, name, want_path))


def test_fused_solve_is_deterministic_and_matches_the_unregularised_state():
    c = _case(1, 128, 77)
    outs = []
    for _ in range(2):
        blk = _block(c, ('kinetic', 'directional'), 'rk4', True, False).train()
        x = T(c['x']).requires_grad_(True)
        z, regs = blk(x, None)
        (z.sum() + sum(r.sum() for r in regs)).backward()
        outs.append((z.detach(), regs[0].detach(), regs[1].detach(), x.grad, blk.odefunc.alpha_train.grad))
    assert gode.odeint.last_reg_path == 'fused'
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    plain = _block(c, (), 'rk4', True, False).train()
    assert torch.equal(plain(T(c['x']).requires_grad_(True), None), outs[0][0])


@pytest.mark.parametrize("cls,block", [(gnpde.AttODEblock, 'attention'), (gnpde.HardAttODEblock, 'hard_attention')])
def test_attention_blocks_training_forward(cls, block):
    """The attention blocks in training: AttODEblock's weights require grad (the per-RHS path, whose
    SDDMMs reach the attention layer); HardAttODEblock samples under no_grad (the fused path over the
    sampled graph's weights).  Values against the oracle on the weights the block handed over."""
    B, C, N, E = 1, 16, 150, 900
    c = _case(B, C, 31, N=N, E=E)
    kinds = ('kinetic', 'directional')
    # norm_idx 1: the fork's scaled_dot score is one value per source, so a softmax over a source's
    # own edges (norm_idx 0) is uniform and carries no gradient to Q and K
    extra = dict(block=block, heads=2, attention_dim=8, attention_norm_idx=1)
    if block == 'hard_attention':
        extra['att_samp_pct'] = 0.7
    blk = _block(c, kinds, 'rk4', True, False, cls=cls, **extra).train()
    blk.t = torch.tensor([0.0, 0.5], device=DEV)
    lay = blk.multihead_att_layer
    with torch.no_grad():
        for lin in (lay.Q, lay.K):
            lin.weight.copy_(torch.randn_like(lin.weight) * 0.2)
    data = gnpde.GraphData()
    data.new_graph(T(c['ei'][:, :, :E]), N)
    x = T(c['x']).requires_grad_(True)
    z, regs = blk(x, data)
    f = blk.odefunc
    w_att = f.attention_weights
    assert gode.odeint.last_reg_path == ('restated' if w_att.requires_grad else 'fused')
    assert w_att.requires_grad == (block == 'attention')
    of = RO.Laplacian(f.edge_index.cpu().numpy(), w_att.detach().double().cpu(), N, RO.t64(c['alpha']),
                      RO.t64(c['beta']), x0=RO.t64(c['x0']), add_source=True)
    zo, ro = RO.solve(of, kinds, RO.t64(c['x'], True), 0.0, 0.5, 2, 'rk4')
    _close(z, zo, VTOL, 'z')
    for r, r_o, k in zip(regs, ro, kinds):
        _close(r, r_o, VTOL, k)
    (z.sum() + sum(C * r.sum() for r in regs)).backward()
    assert torch.isfinite(x.grad).all() and float(x.grad.abs().max()) > 0
    if block == 'attention':
        assert lay.Q.weight.grad is not None and float(lay.Q.weight.grad.abs().max()) > 0


# ---------------------------------------------------------------- unchanged behaviour, out of scope
def test_eval_forward_returns_a_tensor_and_none_coefficients_change_nothing():
    c = _case(2, 128, 55)
    blk = _block(c, ('kinetic',), 'rk4', True, False).eval()
    with torch.no_grad():
        z = blk(T(c['x']), None)
    assert isinstance(z, torch.Tensor) and z.shape == (2, c['N'], 128)
    fns, coeffs = R.create_regularization_fns({'kinetic_energy': None, 'jacobian_norm2': None, 'total_deriv': None,
                                               'directional_penalty': None})
    assert fns == [] and coeffs == []
    res = []
    for key in (True, False):
        opt = dict(OPT, hidden_dim=128, method='rk4', step_size=0.25, add_source=True)
        if key:
            opt['gnpde_regularization'] = True
        b = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, fns, opt, DEV, t=torch.tensor([0.0, 1.0])).to(DEV).train()
        _set(b.odefunc, c, False)
        b.set_x0(T(c['x0']))
        x = T(c['x']).requires_grad_(True)
        out = b(x, None)
        assert isinstance(out, torch.Tensor)
        out.sum().backward()
        res.append((out.detach(), x.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_out_of_scope_cases_raise():
    c = _case(1, 8, 56)
    x = T(c['x'])
    for method, kw, word in (('dopri5', {}, 'adaptive'), ('explicit_adams', {'gnpde_adams': True}, 'multistep'),
                             ('implicit_adams', {'gnpde_adams': True}, 'multistep'),
                             ('rk4', {'adjoint': True, 'adjoint_method': 'rk4'}, 'adjoint')):
        blk = _block(c, ('kinetic',), method, False, False, **kw).train()
        with pytest.raises(NotImplementedError, match=word):
            blk(x.clone().requires_grad_(True), None)
    blk = _block(c, ('kinetic',), 'rk4', False, False).train()
    with pytest.raises(NotImplementedError, match="bf16"):
        blk(x.to(torch.bfloat16), None)
    opt = dict(OPT, hidden_dim=8, method='rk4', step_size=0.25)  # no opt-in key
    b = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [R.quadratic_cost], opt, DEV,
                               t=torch.tensor([0.0, 1.0])).to(DEV).train()
    _set(b.odefunc, c, False)
    with pytest.raises(NotImplementedError, match="gnpde_regularization"):
        b(x, None)
