"""GPU: the multistep solvers (explicit_adams / implicit_adams) — the predictor and corrector
passes of csrc/adams.hip against float64 numpy, and solves end to end against the numpy oracle
(tests/adams_oracle.py) over a float64 CSR right-hand side.

Tolerances.  Kernels: each stored value is an fp64 sum rounded once, so one fp32 ulp of the
float64 (here: extended precision) result; the convergence ratio 1e-5 relative (it is an fp64
quotient rounded to fp32).  Solves: 1e-5 of max |y| (the project's parity bar; the float32 floor
of these runs is below 1e-6), equal RHS counts and equal corrector iteration counts — the latter
only on inputs where the oracle shows the counts do not hinge on rounding (every float64 ratio
outside [2/3, 3/2], the float32 oracle run giving the same counts)."""
import numpy as np
import pytest
import scipy.sparse
import torch

import adams_oracle as AO
import gnpde
import gnpde_oracle as O
from gnpde import integrator as gode
from gnpde import ops
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, rel

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (64, 128), (33, 256), (257, 162)]  # sub-wavefront, n % 4 != 0, odd width, many workgroups


def _ulp(ref):
    """One fp32 unit in the last place at |ref| (float64 array)."""
    return np.spacing(np.abs(np.asarray(ref, np.float64)).astype(np.float32)).astype(np.float64)


def _within_ulp(got, ref):
    got = got.double().cpu().numpy().reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    return bool((np.abs(got - ref) <= _ulp(ref)).all())


def _status(ws):
    rec = ws[:4].cpu()
    return int(rec[0]), int(rec[1]), float(rec[2:3].view(torch.float32))


# ---------------------------------------------------------------- predictor
def _predict_case(H, shape, offset=0):
    R, C = shape
    n = R * C
    rng = np.random.default_rng(1000 * H + R)
    ab, am = AO.tables()
    dt = 0.05
    # coefficients on the scale of the real tables (alternating signs, sum |b| up to ~591 dt)
    cdy = [dt * c * (1.0 + 0.1 * rng.standard_normal()) for c in ab[H]]
    cde = [dt * c * (1.0 + 0.1 * rng.standard_normal()) for c in am[H + 1][1:]]
    ring = rng.standard_normal((H, n)).astype(np.float32)
    y0 = rng.standard_normal(n).astype(np.float32)
    rot = (H // 2) + 1  # hist[j] = ring slot (rot + j) % H: the newest entry sits mid-ring and the list wraps
    order = [(rot + j) % H for j in range(H)]
    ld = np.longdouble
    dy = sum(ld(c) * ring[k].astype(ld) for c, k in zip(cdy, order))
    de = sum(ld(c) * ring[k].astype(ld) for c, k in zip(cde, order))
    xr = y0.astype(ld) + dy
    # device buffers, optionally starting `offset` floats past a 16-byte boundary
    def dev(a):
        buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
        v = buf[offset:offset + a.size]
        v.copy_(T(a))
        return v
    hist = [dev(ring[k]) for k in order]
    outs = [dev(np.full(n, 7.0, np.float32)) for _ in range(3)]
    return dev(y0), hist, cdy, cde, outs, (dy.astype(np.float64), xr.astype(np.float64), de.astype(np.float64))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("H", list(range(3, 12)))
def test_predict_vs_float64(H, shape):
    y0, hist, cdy, cde, (dy, x, de), (rdy, rx, rde) = _predict_case(H, shape)
    ops.adams_predict(y0, hist, cdy, dy, x, cdelta=cde, delta=de)
    assert _within_ulp(dy, rdy) and _within_ulp(x, rx) and _within_ulp(de, rde)
    # without delta: the same dy and x, the delta array untouched
    dy2, x2 = torch.empty_like(dy), torch.empty_like(x)
    keep = de.clone()
    ops.adams_predict(y0, hist, cdy, dy2, x2)
    assert torch.equal(dy2, dy) and torch.equal(x2, x) and torch.equal(de, keep)


@pytest.mark.parametrize("H", [3, 11])
def test_predict_unaligned_base(H):
    """Arrays that start 4 bytes past a 16-byte boundary take the scalar form."""
    y0, hist, cdy, cde, (dy, x, de), (rdy, rx, rde) = _predict_case(H, (64, 128), offset=1)
    assert y0.data_ptr() % 16 == 4
    ops.adams_predict(y0, hist, cdy, dy, x, cdelta=cde, delta=de)
    assert _within_ulp(dy, rdy) and _within_ulp(x, rx) and _within_ulp(de, rde)


def test_predict_rejects_bad_arguments():
    y0 = torch.zeros(8, device=DEV)
    hist = [torch.zeros(8, device=DEV) for _ in range(12)]
    with pytest.raises(ValueError):
        ops.adams_predict(y0, hist, [1.0] * 12, torch.empty_like(y0), torch.empty_like(y0))
    with pytest.raises(ops._lib.GnpdeError, match="alias"):
        ops.adams_predict(y0, hist[:3], [1.0] * 3, hist[0], torch.empty_like(y0))


# ---------------------------------------------------------------- corrector
RTOL_C, ATOL_C, CF = 1e-2, 1e-3, 0.0137


def _correct_case(shape, plant=None, seed=0, offset=0):
    """dy_old within ~0.3 tolerances of the new dy everywhere (converged), except at `plant`
    where it is three times the new value (ratio ~ 60)."""
    R, C = shape
    n = R * C
    rng = np.random.default_rng(seed + n)
    f = rng.standard_normal(n).astype(np.float32)
    delta = (0.1 * rng.standard_normal(n)).astype(np.float32)
    y0 = rng.standard_normal(n).astype(np.float32)
    ld = np.longdouble
    new = (ld(CF) * f.astype(ld) + delta.astype(ld)).astype(np.float64)
    old = (new * (1.0 + 1e-3 * rng.standard_normal(n))).astype(np.float32)
    if plant is not None:
        f[plant], delta[plant] = 1.0, 0.5
        new[plant] = np.float64(ld(CF) * ld(1.0) + ld(np.float32(0.5)))
        old[plant] = np.float32(3.0 * new[plant])
    return f, delta, y0, old, new


def _correct_reference(old, new, y0):
    nd = new.astype(np.float32).astype(np.float64)  # the stored increment
    with np.errstate(invalid='ignore'):
        q = np.abs(old.astype(np.float64) - nd) / (ATOL_C + RTOL_C * np.maximum(np.abs(old.astype(np.float64)), np.abs(nd)))
    ratio = float('nan') if np.isnan(q).any() else float(q.max())
    return new, y0.astype(np.float64) + new, ratio


def _dev(a, offset=0):
    buf = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    v = buf[offset:offset + a.size]
    v.copy_(T(a))
    return v


def _planted_positions(n):
    """First element, last element, and one in the middle workgroup of the launch."""
    return {'first': 0, 'last': n - 1, 'middle': (n // 2) | 1 if n > 2 else n // 2}


@pytest.mark.parametrize("where", ["first", "last", "middle"])
@pytest.mark.parametrize("shape", [(3, 5), (64, 128), (257, 162)])
def test_correct_vs_float64(shape, where):
    n = shape[0] * shape[1]
    idx = _planted_positions(n)[where]
    f, delta, y0, old, new = _correct_case(shape, plant=idx)
    rdy, rx, rratio = _correct_reference(old, new, y0)
    assert rratio > 10.0
    ws = ops.adams_workspace(DEV)
    dy, x = _dev(old), torch.empty(n, device=DEV)
    ops.adams_correct(_dev(f), _dev(delta), _dev(y0), dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _within_ulp(dy, rdy) and _within_ulp(x, rx)
    conv, its, ratio = _status(ws)
    assert (conv, its) == (0, 1)
    assert abs(ratio - rratio) <= 1e-5 * rratio
    assert int(ws[4]) == 0  # the arrival counter is back at zero


def test_correct_unaligned_base():
    shape = (64, 128)
    n = shape[0] * shape[1]
    f, delta, y0, old, new = _correct_case(shape, plant=n - 3)
    rdy, rx, rratio = _correct_reference(old, new, y0)
    ws = ops.adams_workspace(DEV)
    dy, x = _dev(old, 1), _dev(np.zeros(n, np.float32), 1)
    ops.adams_correct(_dev(f, 1), _dev(delta, 1), _dev(y0, 1), dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _within_ulp(dy, rdy) and _within_ulp(x, rx)
    assert abs(_status(ws)[2] - rratio) <= 1e-5 * rratio


def test_correct_nan_is_not_converged():
    shape = (257, 162)
    n = shape[0] * shape[1]
    f, delta, y0, old, new = _correct_case(shape)
    f[n // 3] = np.nan
    ws = ops.adams_workspace(DEV)
    dy, x = _dev(old), torch.empty(n, device=DEV)
    ops.adams_correct(_dev(f), _dev(delta), _dev(y0), dy, x, CF, RTOL_C, ATOL_C, ws)
    conv, its, ratio = _status(ws)
    assert conv == 0 and its == 1 and np.isnan(ratio)
    assert bool(torch.isnan(dy[n // 3])) and int(torch.isnan(dy).sum()) == 1


def test_correct_gating_and_iteration_count():
    shape = (257, 162)
    n = shape[0] * shape[1]
    # converged at the first launch: the second (another f) must change nothing
    f, delta, y0, old, new = _correct_case(shape)
    _, _, rratio = _correct_reference(old, new, y0)
    assert rratio < 0.9
    ws = ops.adams_workspace(DEV)
    dy, x, dl, yd = _dev(old), torch.empty(n, device=DEV), _dev(delta), _dev(y0)
    ops.adams_correct(_dev(f), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    conv, its, ratio = _status(ws)
    assert (conv, its) == (1, 1) and abs(ratio - rratio) <= 1e-5 * rratio
    snap = (dy.clone(), x.clone(), ws.clone())
    ops.adams_correct(_dev(f + 1.0), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    assert torch.equal(dy, snap[0]) and torch.equal(x, snap[1]) and torch.equal(ws, snap[2])
    # the reset opens the gate again
    ops.adams_status_reset(ws)
    assert ws[:8].tolist() == [0] * 8
    ops.adams_correct(_dev(f + 1.0), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _status(ws)[:2] == (0, 1) and not torch.equal(dy, snap[0])
    # not converged: every launch counts
    ops.adams_correct(_dev(f + 2.0), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    ops.adams_correct(_dev(f + 3.0), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _status(ws)[:2] == (0, 3)
    # the same f again: dy does not move, ratio 0, converged at iteration 4; a fifth launch is gated off
    ops.adams_correct(_dev(f + 3.0), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _status(ws) == (1, 4, 0.0)
    ops.adams_correct(_dev(f), dl, yd, dy, x, CF, RTOL_C, ATOL_C, ws)
    assert _status(ws) == (1, 4, 0.0)


# ---------------------------------------------------------------- solves
N_NODES, N_EDGES, N_STEPS = 300, 1500, 16
# the block's tolerances at tol_scale 100: atol 1e-5, rtol 1e-7
TOL_SCALE, ATOL_B, RTOL_B = 100, 1e-5, 1e-7
# Input amplitude per width: the corrector's ratios scale with it (atol dominates), and at dt 0.25
# they slide through 1 as the solution decays; these amplitudes keep every ratio of the float64
# oracle run outside [2/3, 3/2] (asserted in _oracle_pair), so the iteration counts are comparable.
AMPLITUDE = {16: 0.75, 162: 0.625}
_CASES = {}


def _laplacian_case(C):
    """Random graph (rw-normalised with self loops by the block), state, the float64 / float32 CSR
    RHS f = 0.5 (A x - x) (alpha_train = 0: sigma = 0.5); shared by the tests of one width."""
    if C not in _CASES:
        rng = np.random.default_rng(300 + C)
        ei = rng.integers(0, N_NODES, size=(1, 2, N_EDGES))
        x = np.float32(AMPLITUDE[C]) * rng.standard_normal((1, N_NODES, C)).astype(np.float32)
        eo, wo = _prep_oracle(ei, N_NODES)
        A = scipy.sparse.coo_matrix((wo[0], (eo[0, 0], eo[0, 1])), shape=(N_NODES, N_NODES)).tocsr()
        A32 = A.astype(np.float32)
        f64 = lambda t, y: 0.5 * (A @ y - y)  # noqa: E731
        f32 = lambda t, y: np.float32(0.5) * (A32 @ y - y)  # noqa: E731
        # the CSR RHS is the oracle's RHS
        assert np.abs(f64(0.0, x[0].astype(np.float64)) -
                      O.laplacian_rhs(eo, x, None, 0.0, 0.0, edge_weight=wo)[0]).max() <= 1e-13
        _CASES[C] = (ei, x, f64, f32)
    return _CASES[C]


def _block(C, method, dt, max_order, max_iters=4, tol_scale=TOL_SCALE):
    t_end = N_STEPS * dt
    opt = dict(OPT, hidden_dim=C, method=method, step_size=dt, gnpde_adams=True, max_order=max_order,
               max_iters=max_iters, tol_scale=tol_scale, time=t_end)
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0.0, t_end])).to(DEV).eval()
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.0)
    return blk


def _grid(t_end, dt):
    """The solver's own grid (float32 times, as the block's t.type_as(x))."""
    t = torch.tensor([0.0, t_end], dtype=torch.float32)
    return gode._host_grid([float(v) for v in t.tolist()], torch.float32, dt)


def _oracle_pair(f64, f32, x, grid, method, max_order, rtol, atol, max_iters=4, margin=True):
    """The float64 oracle run, after the two assertions that make its iteration counts
    comparable: every ratio outside [2/3, 3/2], and the float32 run giving the same counts."""
    want = AO.solve(f64, x.astype(np.float64), grid, method, rtol, atol, max_order=max_order, max_iters=max_iters)
    low = AO.solve(f32, x, grid, method, rtol, atol, max_order=max_order, max_iters=max_iters, dtype=np.float32)
    if margin:
        assert AO.margin_ok(want.ratios), [r for rs in want.ratios for r in rs if 2 / 3 <= r <= 1.5]
    assert low.iterations == want.iterations and low.converged == want.converged
    return want


@pytest.mark.parametrize("C", [16, 162])
@pytest.mark.parametrize("method,dt,max_order", [("implicit_adams", 0.25, 8), ("implicit_adams", 0.05, 12),
                                                 ("explicit_adams", 0.02, 4), ("explicit_adams", 0.02, 12)])
def test_laplacian_block_vs_oracle(method, dt, max_order, C):
    ei, x, f64, f32 = _laplacian_case(C)
    want = _oracle_pair(f64, f32, x[0], _grid(N_STEPS * dt, dt), method, max_order, RTOL_B, ATOL_B)
    blk = _block(C, method, dt, max_order)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N_NODES)
    with torch.no_grad():
        z = blk(T(x), data)
    assert gode.odeint.last_path == 'adams_fused'
    err = rel(z[0], want.y)
    print("adams %s dt=%g max_order=%d C=%d: rel err %.3e, iterations %s" % (method, dt, max_order, C, err,
                                                                             gode.odeint.last_adams['iterations']))
    assert err <= RTOL
    assert gode.odeint.last_adams['iterations'] == want.iterations
    assert gode.odeint.last_adams['converged'] == want.converged
    assert blk.odefunc.nfe == want.nfe
    if dt == 0.25:
        assert max(want.iterations) >= 3 and min(want.iterations[2:]) == 1  # the chunk length follows the counts


def test_laplacian_block_output_inside_a_step_and_second_solve():
    """An output time off the grid (linear interpolation) through gnpde.odeint, twice on one
    module: the second solve reuses the pooled history ring and gives the same bits."""
    C, dt = 16, 0.05
    ei, x, f64, f32 = _laplacian_case(C)
    blk = _block(C, 'implicit_adams', dt, 6)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N_NODES)
    blk.reset_graph_data(data, torch.float32)
    ts = [0.0, 0.33, 0.8]
    t = torch.tensor(ts, dtype=torch.float32, device=DEV)
    opts = dict(gnpde_adams=True, step_size=dt, max_order=6)
    with torch.no_grad():
        a = gode.odeint(blk.odefunc, T(x), t, rtol=RTOL_B, atol=ATOL_B, method='implicit_adams', options=opts)
        b = gode.odeint(blk.odefunc, T(x), t, rtol=RTOL_B, atol=ATOL_B, method='implicit_adams', options=opts)
    assert gode.odeint.last_path == 'adams_fused' and torch.equal(a, b)
    ts32 = [float(v) for v in torch.tensor(ts, dtype=torch.float32).tolist()]
    grid = gode._host_grid(ts32, torch.float32, dt)
    want = AO.solve(f64, x[0].astype(np.float64), grid, 'implicit_adams', RTOL_B, ATOL_B, max_order=6, times=ts32)
    assert rel(a[:, 0], want.sol) <= RTOL


def test_transformer_rhs_vs_oracle():
    """implicit_adams over ODEFuncTransformerAtt: the fused loop with a RHS that is not K1."""
    C, heads, att, dt = 16, 2, 16, 0.05
    rng = np.random.default_rng(77)
    ei = rng.integers(0, N_NODES, size=(1, 2, N_EDGES))
    x = rng.standard_normal((1, N_NODES, C)).astype(np.float32)
    Wq, Wk = [(rng.standard_normal((att, C)) * 0.05).astype(np.float32) for _ in range(2)]
    bq, bk = [(rng.standard_normal(att) * 0.05).astype(np.float32) for _ in range(2)]
    opt = dict(OPT, hidden_dim=C, heads=heads, attention_dim=att, attention_norm_idx=0, function='transformer',
               attention_score_mode='reference')
    func = gnpde.ODEFuncTransformerAtt(C, C, opt, DEV).to(DEV)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(0.3)
        lay.Q.weight.copy_(T(Wq))
        lay.Q.bias.copy_(T(bq))
        lay.K.weight.copy_(T(Wk))
        lay.K.bias.copy_(T(bk))
    func.eval()
    func.edge_index = T(ei)
    f64 = lambda t, y: O.transformer_rhs(ei, y[None], None, Wq, bq, Wk, bk, heads, 0, 0.3, 0.0)[0]  # noqa: E731
    f32 = lambda t, y: O.transformer_rhs_f32(ei, y[None], Wq, bq, Wk, bk, heads, 0, 0.3,  # noqa: E731
                                             score_mode='reference')[0]
    grid = _grid(N_STEPS * dt, dt)
    want = _oracle_pair(f64, f32, x[0], grid, 'implicit_adams', 6, RTOL_B, ATOL_B)
    t = torch.tensor([0.0, N_STEPS * dt], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        z = gode.odeint(func, T(x), t, rtol=RTOL_B, atol=ATOL_B, method='implicit_adams',
                        options=dict(gnpde_adams=True, step_size=dt, max_order=6))
    assert gode.odeint.last_path == 'adams_fused'
    assert rel(z[1, 0], want.y) <= RTOL
    assert gode.odeint.last_adams['iterations'] == want.iterations
    assert func.nfe == want.nfe


@pytest.mark.parametrize("method", ["explicit_adams", "implicit_adams"])
def test_plain_callable_takes_the_restated_path(method):
    """Any callable on device tensors: the restated loop with the HIP stage combinations."""
    C, dt = 24, 0.05
    rng = np.random.default_rng(78)
    M = (rng.standard_normal((C, C)) * 0.2).astype(np.float32)
    x = np.float32(4.0) * rng.standard_normal((40, C)).astype(np.float32)  # (amplitude: see AMPLITUDE)
    Mt = T(M)
    calls = [0]

    def f(t, y):
        calls[0] += 1
        return y @ Mt
    f64 = lambda t, y: y @ M.astype(np.float64)  # noqa: E731
    f32 = lambda t, y: y @ M  # noqa: E731
    grid = _grid(N_STEPS * dt, dt)
    # (max_order 6: the order-11 predictor is unstable on this spectrum at dt 0.05 and lifts the float32
    # floor of the oracle itself to 2e-5)
    want = _oracle_pair(f64, f32, x, grid, method, 6, RTOL_B, ATOL_B)
    t = torch.tensor([0.0, N_STEPS * dt], dtype=torch.float32, device=DEV)
    with torch.no_grad():
        z = gode.odeint(f, T(x), t, rtol=RTOL_B, atol=ATOL_B, method=method,
                        options=dict(gnpde_adams=True, step_size=dt, max_order=6))
    assert gode.odeint.last_path == 'adams_restated'
    assert rel(z[1], want.y) <= RTOL
    assert gode.odeint.last_adams['iterations'] == want.iterations and calls[0] == want.nfe


def test_max_iters_one_on_the_device():
    """max_iters = 1 at dt 0.25 and the block's default tolerances: no Adams step converges, the
    warning fires once, the ring gives up its oldest entry each step, values follow the oracle."""
    C, dt = 16, 0.25
    ei, x, f64, f32 = _laplacian_case(C)
    rtol, atol = 1e-9, 1e-7  # tol_scale 1
    want = _oracle_pair(f64, f32, x[0], _grid(N_STEPS * dt, dt), 'implicit_adams', 8, rtol, atol, max_iters=1)
    assert want.iterations[2:] == [1] * (N_STEPS - 2) and not any(want.converged[2:])
    assert min(r for rs in want.ratios for r in rs) > 1.5
    blk = _block(C, 'implicit_adams', dt, 8, max_iters=1, tol_scale=1)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N_NODES)
    with pytest.warns(UserWarning, match="did not converge") as rec, torch.no_grad():
        z = blk(T(x), data)
    assert len([w for w in rec if "did not converge" in str(w.message)]) == 1
    assert gode.odeint.last_path == 'adams_fused'
    assert gode.odeint.last_adams['converged'] == want.converged
    assert gode.odeint.last_adams['iterations'] == want.iterations
    assert blk.odefunc.nfe == want.nfe
    assert rel(z[0], want.y) <= RTOL


def test_bf16_state_takes_the_restated_path():
    """A bf16 state is not fused: it runs the restated loop (bf16 stage passes)."""
    C, dt = 16, 0.05
    ei, x, f64, f32 = _laplacian_case(C)
    blk = _block(C, 'explicit_adams', dt, 4)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N_NODES)
    with torch.no_grad():
        z = blk(T(x).to(torch.bfloat16), data)
    assert z.dtype == torch.bfloat16 and gode.odeint.last_path == 'adams_restated'
    xb = T(x).to(torch.bfloat16).double().cpu().numpy()
    want = AO.solve(f64, xb[0], _grid(N_STEPS * dt, dt), 'explicit_adams', max_order=4)
    # 16 steps, each rounding the state to bf16 (2^-9 relative) and adding dt sum |b_j| |f_j| <= 0.05 * 3.67
    # |y| of history values rounded likewise: at most 16 * 1.2 * 2^-9 = 3.7e-2 of max |y|
    assert rel(z[0], want.y) <= 4e-2
