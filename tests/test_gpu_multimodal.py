"""GPU: the Laplacian ODE function's multi_modal branch — the flash-style cross-attention
kernel gnpde_cross_attention_f32 (ops.cross_attention) against the float64 restatement
tests/multimodal_oracle.py, and MultiModalLaplacianODEFunc (RHS, gradients, solves, a
training step) against the fixtures of the reference's own forward
(tests/golden/multimodal/mm_*.npz, mmgrad_*.npz).

Bars (the project's own): RTOL = 1e-5 as max error over max reference for every forward
quantity; gradients GRAD_RTOL = 1e-4 under the rule of test_gpu_grad_golden.py.  Both
products of the kernel are exact-fp32 fmaf chains (a few 1e-7 from float64 at these
widths; the fixtures' own fp32 runs are within 5e-6); a dropped or doubled key, a missed
rescale or a row taken from the other batch element is 1e-2 or more."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import gnpde.integrator as gi
import gnpde_oracle as O
import multimodal_oracle as MM
from conftest import GOLDEN as _GOLDEN
from gnpde import _lib, ops
from gnpde.function_laplacian_multimodal import MultiModalLaplacianODEFunc
from test_gpu_parity import DEV, OPT, RTOL, T, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "multimodal")
GRAD_RTOL = 1e-4
FWD = sorted(glob.glob(os.path.join(GOLDEN, "mm_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "mmgrad_*.npz")))
TILE = 32       # keys of a staged tile (csrc/cross_attention.hip kXaTile)


# --------------------------------------------------------------------------- the kernel
def _draw(B, N, M, C, seed):
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(s).astype(np.float32) for s in ((B, N, C), (B, M, C), (B, M, C)))


def _check_kernel(q, k, v, scale, tag):
    want, want_lse = MM.cross_attention(q, k, v, scale, lse=True)
    out, lse = ops.cross_attention(T(q), T(k), T(v), scale, lse=True)
    assert out.shape == q.shape and tuple(lse.shape) == q.shape[:-1]
    e, el = rel(out, want), rel(lse, want_lse)
    print("%s: out err %.3e, lse err %.3e" % (tag, e, el))
    assert e <= RTOL and el <= RTOL
    # without the lse output, and run again: the same bits
    assert torch.equal(ops.cross_attention(T(q), T(k), T(v), scale), out)
    out2, lse2 = ops.cross_attention(T(q), T(k), T(v), scale, lse=True)
    assert torch.equal(out2, out) and torch.equal(lse2, lse)
    return out


@pytest.mark.parametrize("C", [4, 12, 80, 162, 256])
@pytest.mark.parametrize("M", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_kernel_key_tiles_and_widths(M, C):
    """Every key-tile boundary at every width class: C % 4 != 0 (162), C % 32 != 0, the widest."""
    q, k, v = _draw(1, 33, M, C, 1000 * M + C)
    _check_kernel(q, k, v, 1.0 / np.sqrt(C), "M=%d C=%d" % (M, C))


@pytest.mark.parametrize("C", [12, 162])
@pytest.mark.parametrize("N", [1, 33, 129])
def test_kernel_row_tiles(N, C):
    """One row, a wavefront and a row, a workgroup and a row."""
    q, k, v = _draw(1, N, TILE + 1, C, 77 * N + C)
    _check_kernel(q, k, v, 1.0 / np.sqrt(C), "N=%d C=%d" % (N, C))


def test_kernel_batch_elements_keep_their_own_keys():
    """B = 2, N = 70: the second element's rows start in a workgroup of their own (a
    workgroup never straddles two elements' K / V), and the two elements' tokens differ."""
    q, k, v = _draw(2, 70, 45, 48, 5)
    k[1] *= 2.0
    v[1] += 3.0
    out = _check_kernel(q, k, v, 1.0 / np.sqrt(48), "B=2 N=70")
    # element 1 against element 0's tokens is far off: the check above separates them
    wrong = MM.cross_attention(q[1:], k[:1], v[:1], 1.0 / np.sqrt(48))
    assert rel(out[1:], wrong) > 1e-2


@pytest.mark.parametrize("where", ["first", "last", "rising"])
def test_kernel_rescales(where):
    """A dominant key in the first tile (later tiles rescale by 1 and add almost nothing),
    in the last (everything before it is scaled down by exp(-20) or so), and scores rising
    with the key index (a rescale at every tile)."""
    B, N, M, C = 1, 40, 2 * TILE + 3, 32
    rng = np.random.default_rng(11)
    q = (rng.standard_normal((B, N, C)) * 0.3 + 1.0).astype(np.float32)
    k = (rng.standard_normal((B, M, C)) * 0.1).astype(np.float32)
    v = rng.standard_normal((B, M, C)).astype(np.float32)
    if where == "rising":
        k += (np.arange(M, dtype=np.float32) * 0.05)[None, :, None]     # score ~ 0.05 m C / sqrt(C) = 0.28 m
    else:
        k[:, 5 if where == "first" else M - 1] += 4.0                   # score ~ 4 C / sqrt(C) = 23
    _check_kernel(q, k, v, 1.0 / np.sqrt(C), where)


def test_kernel_uniform_softmax():
    """k = 0 (what y = 0 and a zero K2 bias give): every score is 0, x~ = the mean of v, lse = ln M."""
    q, k, v = _draw(2, 37, 45, 20, 3)
    k[:] = 0.0
    out, lse = ops.cross_attention(T(q), T(k), T(v), 0.25, lse=True)
    want = np.broadcast_to(v.astype(np.float64).mean(axis=1, keepdims=True), q.shape)
    assert rel(out, want) <= RTOL
    assert rel(lse, np.full(q.shape[:-1], np.log(45.0))) <= RTOL


def test_kernel_refuses_what_it_does_not_serve():
    q, k, v = _draw(1, 5, 3, 257, 1)
    with pytest.raises(_lib.GnpdeError, match="C=257"):
        ops.cross_attention(T(q), T(k), T(v), 1.0)
    with pytest.raises(ValueError, match="M = 0"):
        ops.cross_attention(T(q), T(k)[:, :0], T(v)[:, :0], 1.0)
    with pytest.raises(TypeError):
        ops.cross_attention(T(q).double(), T(k), T(v), 1.0)
    # an [N, C] query is a batch of one
    q, k, v = _draw(1, 9, 4, 8, 2)
    assert torch.equal(ops.cross_attention(T(q)[0], T(k)[0], T(v)[0], 0.5), ops.cross_attention(T(q), T(k), T(v), 0.5)[0])


def test_kernel_rows_past_2_31_elements():
    """N * C just past 2^31 elements: the row offsets of q and out are 64-bit.  The first and
    the last rows against the oracle, and the torch restatement on the same rows."""
    C, M = 128, 3
    N = (1 << 31) // C + 5
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    q = torch.randn(1, N, C, device=DEV, generator=gen)
    k = torch.randn(1, M, C, device=DEV, generator=gen)
    v = torch.randn(1, M, C, device=DEV, generator=gen)
    out, lse = ops.cross_attention(q, k, v, 0.1, lse=True)
    for sl in (slice(0, 64), slice(N - 64, N)):
        want, want_lse = MM.cross_attention(q[:, sl].cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), 0.1, lse=True)
        assert rel(out[:, sl], want) <= RTOL
        assert rel(lse[:, sl], want_lse) <= RTOL
    del q, out, lse
    torch.cuda.empty_cache()


def test_torch_restatement_on_the_device():
    q, k, v = _draw(2, 70, 45, 48, 8)
    want, want_lse = MM.cross_attention(q, k, v, 0.2, lse=True)
    out, lse = ops.cross_attention_torch(T(q), T(k), T(v), 0.2, lse=True)
    assert rel(out, want) <= RTOL and rel(lse, want_lse) <= RTOL


# --------------------------------------------------------------------------- the ODE function
def _load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, **kw):
    o = dict(OPT, hidden_dim=m["C"], block='constant', function='laplacian', add_source=m["add_source"],
             no_alpha_sigmoid=m["no_alpha_sigmoid"], multi_modal=True, gnpde_multi_modal=True,
             second_modality_dim=m["D2"])
    o.update(kw)
    return o


def _params(func):
    return dict(Wq=func.Q2.weight, bq=func.Q2.bias, Wk=func.K2.weight, bk=func.K2.bias, Wv=func.V2.weight,
                bv=func.V2.bias)


def _make(d, m, **kw):
    C = m["C"]
    opt = _opt(m, **kw)
    cls = gnpde.set_function(opt)
    assert cls is MultiModalLaplacianODEFunc
    func = cls(C, C, opt, DEV).to(DEV)
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
        for n, p in _params(func).items():
            p.copy_(T(d[n]))
    func.edge_index = T(d["edge_index"])
    func.edge_weight = T(d["edge_weight"])
    func.x0 = T(d["x0"])
    func.y = T(d["y"])
    return func


@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_rhs_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    with torch.no_grad():
        f = func(torch.tensor(0.0), T(d["x"]))
        xt = func.cross_attention(T(d["x"]))
    assert func.nfe == 1
    e_f, e_xt = rel(f, d["f"]), rel(xt, MM.fixture_rhs(d)[1])
    print("%s: f err %.3e, x~ err %.3e (the fixture's fp32 run: %.3e)" % (os.path.basename(path), e_f, e_xt,
                                                                       m["ref32_dev"]))
    assert e_f <= RTOL and e_xt <= RTOL
    with torch.no_grad():  # repeated evaluations: the same bits, k / v from the cache
        kv = func.kv(func.y)
        assert torch.equal(func(torch.tensor(0.0), T(d["x"])), f)
        assert func.kv(func.y)[0] is kv[0]


def test_zero_second_modality_gives_the_value_bias():
    """y = 0: k = bk for every token, so the softmax is uniform and x~ = mean_m v = bv in every row."""
    d, m = _load(os.path.join(GOLDEN, "mm_b2_c48.npz"))
    func = _make(d, m)
    func.y = torch.zeros_like(func.y)
    with torch.no_grad():
        xt = func.cross_attention(T(d["x"]))
    assert rel(xt, np.broadcast_to(d["bv"].astype(np.float64), d["x"].shape)) <= RTOL


def test_bf16_state_and_missing_y_raise():
    d, m = _load(os.path.join(GOLDEN, "mm_c20_sharp.npz"))
    func = _make(d, m)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp32"):
        func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))
    func.y = None
    with torch.no_grad(), pytest.raises(RuntimeError, match="y is not set"):
        func(torch.tensor(0.0), T(d["x"]))


def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e" % (name, err, tol))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_grad_golden(path, monkeypatch):
    d, m = _load(path)
    func = _make(d, m)
    x = T(d["x"]).requires_grad_(True)
    func.y = T(d["y"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    scale = max(float(np.abs(d[k]).max()) for k in d.files if k.startswith("g_") and d[k].size)
    grads = dict(x=x.grad, y=func.y.grad, alpha_train=func.alpha_train.grad, beta_train=func.beta_train.grad)
    grads.update((n, p.grad) for n, p in _params(func).items())
    for n, g in grads.items():
        _check(n, g, d["g_" + n], scale)
    # the same gradients from row chunks of 7 and key chunks of 5 (the bounded-scratch route)
    import gnpde.function_laplacian_multimodal as fm
    monkeypatch.setattr(fm, "BACKWARD_CHUNK_BYTES", 7 * 4 * m["M"])
    monkeypatch.setattr(fm, "_DQ_KEYS", 5)
    x2 = T(d["x"]).requires_grad_(True)
    for p in func.parameters():
        p.grad = None
    func.y = T(d["y"]).requires_grad_(True)
    (func(torch.tensor(0.0), x2) * T(d["gout"])).sum().backward()
    _check("x (chunked)", x2.grad, d["g_x"], scale)
    _check("y (chunked)", func.y.grad, d["g_y"], scale)
    _check("Wk (chunked)", func.K2.weight.grad, d["g_Wk"], scale)


# The dopri5 solves take options['first_step'] = 0.2 on both sides, as test_gpu_adaptive_backprop.py does.
# torchdiffeq's initial-step rule starts these systems at h = 0.07 (d1, d2 of a few thousand), a step whose
# error estimate (about 1e-9) is of the size of fp32 rounding in the stage derivatives, so the controller's
# growth factor 0.9 r^(-1/5) for the SECOND step is set by that rounding.  Measured on the float64 oracle
# alone, with relative noise eps added to its RHS: the solution at t = 1 moves by 15-45 eps on
# mm_b2_c48_src and 100-150 eps on mm_n70_c48_noalpha under the default rule, against 0.9-1.9 eps for rk4
# and 2.8 eps with first_step = 0.2.  The fixtures' own fp32 reference runs (eps up to 8e-7; the
# generator admits 5e-6) would miss 1e-5 under the default rule, so that comparison checks the rounding,
# not the RHS; its figure is printed for the record (0.8-1.8e-5 here, 1.6-3.3e-5 with the torch fp32
# composition as the RHS of the fp64 solver).
@pytest.mark.parametrize("name", ["mm_b2_c48_src", "mm_n70_c48_noalpha"])
def test_solves_against_the_restatement(name):
    """rk4 with 3 steps (the stage pass on the solver's state; eager, then captured step
    graphs) and dopri5 over [0, 1] against the oracle's solvers on the oracle's RHS."""
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    x = d["x"]
    f = lambda t, y: MM.fixture_rhs(d, x=y)[0]  # noqa: E731
    last = lambda w: w[-1] if np.ndim(w) == x.ndim + 1 else w  # noqa: E731
    func = _make(d, m, max_nfe=10 ** 6)
    t3 = torch.tensor([0.0, 0.75], device=DEV)
    t1 = torch.tensor([0.0, 1.0], device=DEV)
    outs = []
    with torch.no_grad():
        for graph in (False, True, True):
            outs.append(gnpde.odeint(func, T(x), t3, method='rk4',
                                     options={'step_size': 0.25, 'gnpde_graph': graph})[-1])
    torch.cuda.synchronize()
    e_rk4 = rel(outs[0], O.odeint_fixed(f, x, 0.0, 0.75, 'rk4', 0.25))
    print("%s: rk4 err %.3e" % (name, e_rk4))
    assert e_rk4 <= RTOL
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    with torch.no_grad():
        z = gnpde.odeint(func, T(x), t1, rtol=1e-3, atol=1e-4, method='dopri5', options={'first_step': 0.2})[-1]
    n_got = gi.odeint.last_n_steps
    assert gi.odeint.last_path == 'fused_stage'
    want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4, first_step=0.2)
    e_dp = rel(z, last(want))
    print("%s: dopri5 (first_step 0.2) err %.3e, %d steps" % (name, e_dp, n_got))
    assert n_got == n_want
    assert e_dp <= RTOL
    with torch.no_grad():  # for the record: the default initial step (see the comment above)
        z0 = gnpde.odeint(func, T(x), t1, rtol=1e-3, atol=1e-4, method='dopri5')[-1]
    want0, n0 = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
    print("%s: dopri5 (default first step) err %.3e, steps %d / %d" % (name, rel(z0, last(want0)),
                                                                     gi.odeint.last_n_steps, n0))


def test_graph_replay_is_bit_equal_and_follows_y():
    """An 8-step rk4 solve with captured step graphs against one without: the same bits.
    Then another y (a new tensor), then the same tensor edited in place, then K2 edited in
    place: the cached k / v follow each time, under replay too."""
    d, m = _load(os.path.join(GOLDEN, "mm_b2_c48_src.npz"))
    x = d["x"]
    func = _make(d, m, max_nfe=10 ** 6)
    t = torch.tensor([0.0, 1.0], device=DEV)

    def solve(graph):
        with torch.no_grad():
            return gnpde.odeint(func, T(x), t, method='rk4', options={'step_size': 0.125, 'gnpde_graph': graph})[-1]

    def want(dd):
        return O.odeint_fixed(lambda tt, yy: MM.fixture_rhs(dd, x=yy)[0], x, 0.0, 1.0, 'rk4', 0.125)

    plain, replay = solve(False), solve(True)
    assert torch.equal(plain, replay) and torch.equal(solve(True), replay)
    assert rel(replay, want(d)) <= RTOL
    d2 = dict((k, d[k]) for k in d.files)
    d2["y"] = (d["y"][:, ::-1] * np.float32(1.5) + np.float32(0.25)).copy()
    func.y = T(d2["y"])
    z2 = solve(True)
    assert not torch.equal(z2, replay)
    assert rel(z2, want(d2)) <= RTOL and torch.equal(z2, solve(False))
    with torch.no_grad():
        func.y.mul_(0.5)
    d2["y"] = d2["y"] * np.float32(0.5)
    z3 = solve(True)
    assert not torch.equal(z3, z2) and rel(z3, want(d2)) <= RTOL
    with torch.no_grad():
        func.K2.weight.mul_(-1.0)
    d2["Wk"] = -d["Wk"]
    z4 = solve(True)
    assert not torch.equal(z4, z3) and rel(z4, want(d2)) <= RTOL


def test_adjoint_training_step():
    """One training step of a ConstantODEblock with adjoint=True: the generic autograd
    adjoint runs, every parameter of the branch gets a finite non-zero gradient and moves."""
    d, m = _load(os.path.join(GOLDEN, "mmgrad_b2_src.npz"))
    opt = _opt(m, adjoint=True, method='rk4', adjoint_method='rk4', step_size=0.5, adjoint_step_size=0.5,
               max_nfe=10 ** 6, self_loop_weight=1)
    blk = gnpde.ConstantODEblock(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0.0, 1.0])).to(DEV)
    func = blk.odefunc
    assert isinstance(func, MultiModalLaplacianODEFunc)
    with torch.no_grad():
        for n, p in _params(func).items():
            p.copy_(T(d[n]))
    data = gnpde.GraphData()
    # the block adds the missing self loops: both elements take element 0's edges, so their counts stay equal
    data.new_graph(T(np.repeat(d["edge_index"][:1], m["B"], axis=0)), m["N"], edge_attr=None)
    x, y = T(d["x"]), T(d["y"])
    blk.train()
    blk.set_x0(x)
    optim = torch.optim.SGD(blk.parameters(), lr=0.1)
    before = {n: p.detach().clone() for n, p in _params(func).items()}
    gi._OdeintAdjoint.last_path = None
    out = blk(x, data, y)
    assert out.shape == x.shape and func.y is y
    (out * T(d["gout"])).sum().backward()
    assert gi._OdeintAdjoint.last_path == 'autograd'
    for n, p in list(_params(func).items()) + [("alpha_train", func.alpha_train), ("beta_train", func.beta_train)]:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), n
    optim.step()
    for n, p in _params(func).items():
        assert not torch.equal(p, before[n]), n
