"""GPU: GAT mix_features — the fused output product gnpde_linear_rhs_f32 (ops.linear_rhs)
against fp64 torch-CPU, and the ODE function against the reference's own float64 run
(tests/golden/gat_mix/gatmix_*.npz, gatmixgrad_*.npz) and the fp64 restatement
tests/gat_mix_oracle.py.

Bars: the plain product (rhs=False) <= 2e-6 of its maximum (the bar of
test_gpu_parity.py::test_linear_mfma_vs_fp64: an f32 GEMM); f <= RTOL = 1e-5 relative, or
the deviation of the fixture's own fp32 reference run where that is larger; attention
<= 2e-5 absolute; the returned wx <= 2e-6 relative.  Gradients under the rule of
test_gpu_grad_golden.py.  The fused stage equals f + ops.stage_apply bit for bit."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gat_mix_oracle as M
import gat_oracle as G
import gnpde
import gnpde.integrator as gi
import gnpde_oracle as O
from conftest import GOLDEN as _GOLDEN
from gnpde import _lib, ops
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "gat_mix")
PROD_RTOL = 2e-6
ATT_ATOL = 2e-5
GRAD_RTOL = 1e-4
FWD = sorted(glob.glob(os.path.join(GOLDEN, "gatmix_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "gatmixgrad_*.npz")))
# (K, C): three shapes of the split-bf16 kernel, three of the plain one (C % 4, K % 16, K < 16)
SHAPES = [(16, 64), (64, 128), (128, 128), (48, 162), (20, 80), (8, 12)]


# --------------------------------------------------------------------------- the kernel
def _operands(R, K, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((R, K)).astype(np.float32)
    Wt = (rng.standard_normal((C, K)) * 0.3).astype(np.float32)
    x = rng.standard_normal((R, C)).astype(np.float32)
    x0 = rng.standard_normal((R, C)).astype(np.float32)
    return z, Wt, x, x0


def _want(z, Wt, x, x0, alpha, beta, sigmoid):
    ax = z.astype(np.float64) @ Wt.astype(np.float64).T
    a = 1.0 / (1.0 + np.exp(-alpha)) if sigmoid else alpha
    f = a * (ax - x)
    return ax, (f + beta * x0 if x0 is not None else f)


@pytest.mark.parametrize("K,C", SHAPES)
@pytest.mark.parametrize("R", [1, 31, 33, 100])
def test_linear_rhs_vs_fp64(R, K, C):
    z, Wt, x, x0 = _operands(R, K, C, 100 * R + K + C)
    al, be = torch.tensor(0.4, device=DEV), torch.tensor(-0.7, device=DEV)
    ax_want, _ = _want(z, Wt, x, None, 0.4, 0.0, True)
    ax = ops.linear_rhs(T(z), T(Wt), None, rhs=False)
    assert tuple(ax.shape) == (R, C)
    e = rel(ax, ax_want)
    print("R=%d K=%d C=%d: product err %.3e" % (R, K, C, e))
    assert e <= PROD_RTOL
    assert torch.equal(ops.linear_rhs(T(z), T(Wt), T(x), rhs=False), ax)  # x is not read
    for with_x0 in (False, True):
        for sigmoid in (True, False):
            f = ops.linear_rhs(T(z), T(Wt), T(x), x0=T(x0) if with_x0 else None, alpha=al, beta=be,
                               alpha_sigmoid=sigmoid, add_source=with_x0)
            _, want = _want(z, Wt, x, x0 if with_x0 else None, 0.4, -0.7, sigmoid)
            e = rel(f, want)
            print("  x0=%d sigmoid=%d: f err %.3e" % (with_x0, sigmoid, e))
            assert e <= RTOL
    torch.cuda.synchronize()


def test_linear_rhs_second_tile_per_wavefront():
    """R = 40,000 rows at C = 128: 1,250 row tiles over the 1,024 wavefronts of a column
    slice (2,048 wavefronts over two 64-column slices), so wavefronts walk a second tile."""
    R, K, C = 40000, 16, 128
    z, Wt, x, x0 = _operands(R, K, C, 5)
    al, be = torch.tensor(0.4, device=DEV), torch.tensor(-0.7, device=DEV)
    f = ops.linear_rhs(T(z), T(Wt), T(x), x0=T(x0), alpha=al, beta=be, add_source=True)
    ax_want, want = _want(z, Wt, x, x0, 0.4, -0.7, True)
    assert rel(f, want) <= RTOL
    assert rel(ops.linear_rhs(T(z), T(Wt), None, rhs=False), ax_want) <= PROD_RTOL
    for _ in range(2):
        assert torch.equal(ops.linear_rhs(T(z), T(Wt), T(x), x0=T(x0), alpha=al, beta=be, add_source=True), f)


def _stage_bufs(R, C, seed):
    rng = np.random.default_rng(seed)
    return {k: T(rng.standard_normal((R, C)).astype(np.float32)) for k in ("y0", "k1", "k2", "o0", "o1", "fo")}


def _stage(kind, b, x):
    """Stages of the fixed-grid epilogue: one / two outputs, 0-2 operands, base = x, an
    output aliasing its base, f_out."""
    if kind == "one_plain":       # one output, no base, no operand
        return ops.Stage(outs=[(b["o0"], None, 0.0, 0.25, [])]), ["o0"]
    if kind == "one_base_x":      # base = the RHS input, one operand
        return ops.Stage(outs=[(b["o0"], x, 1.0, 0.5, [(b["k1"], -0.125)])]), ["o0"]
    if kind == "two_out":         # two outputs, two shared operands, f stored too
        return ops.Stage(f_out=b["fo"], outs=[(b["o0"], b["y0"], 1.0, 0.375, [(b["k1"], 0.75), (b["k2"], -1.5)]),
                                              (b["o1"], x, 0.5, -0.25, [(b["k2"], 2.0)])]), ["fo", "o0", "o1"]
    if kind == "in_place":        # the output is its own base (accumulation in place)
        return ops.Stage(outs=[(b["y0"], b["y0"], 1.0, 1.0 / 6.0, [(b["k1"], 1.0 / 3.0)])]), ["y0"]
    if kind == "f_only":
        return ops.Stage(f_out=b["fo"]), ["fo"]
    raise KeyError(kind)


@pytest.mark.parametrize("kind", ["one_plain", "one_base_x", "two_out", "in_place", "f_only"])
@pytest.mark.parametrize("R,K,C", [(100, 64, 128), (33, 16, 64), (100, 20, 80), (31, 48, 162)])
def test_fused_stage_equals_f_then_stage_apply(R, K, C, kind):
    z, Wt, x, x0 = _operands(R, K, C, R + K + C)
    zt, Wtt, xt, x0t = T(z), T(Wt), T(x), T(x0)
    kw = dict(x0=x0t, alpha=torch.tensor(0.4, device=DEV), beta=torch.tensor(-0.7, device=DEV), add_source=True)
    f = ops.linear_rhs(zt, Wtt, xt, **kw)
    runs = []
    for fused in (True, False, True, True):
        b = _stage_bufs(R, C, 17)
        st, outs = _stage(kind, b, xt)
        assert not st.wide
        if fused:
            assert ops.linear_rhs(zt, Wtt, xt, stage=st, **kw) is None
        else:
            ops.stage_apply(st, f, xt, xt)
        runs.append([b[k].clone() for k in outs])
    torch.cuda.synchronize()
    for got in (runs[0], runs[2], runs[3]):  # fused == unfused bit for bit; three fused runs alike
        for u, v in zip(got, runs[1]):
            assert torch.equal(u, v)
    # and the value itself, against fp64
    _, fw = _want(z, Wt, x, x0, 0.4, -0.7, True)
    b = {k: v.double().cpu().numpy() for k, v in _stage_bufs(R, C, 17).items()}
    want = {"one_plain": [0.25 * fw], "one_base_x": [x + 0.5 * fw - 0.125 * b["k1"]],
            "two_out": [fw, b["y0"] + 0.375 * fw + 0.75 * b["k1"] - 1.5 * b["k2"], 0.5 * x - 0.25 * fw + 2.0 * b["k2"]],
            "in_place": [b["y0"] + fw / 6.0 + b["k1"] / 3.0], "f_only": [fw]}[kind]
    for u, w in zip(runs[0], want):
        assert rel(u, w) <= RTOL


def test_plain_product_takes_a_stage_too():
    R, K, C = 100, 64, 128
    z, Wt, x, _ = _operands(R, K, C, 3)
    zt, Wtt, xt = T(z), T(Wt), T(x)
    ax = ops.linear_rhs(zt, Wtt, xt, rhs=False)
    outs = []
    for fused in (True, False):
        b = _stage_bufs(R, C, 19)
        st = ops.Stage(outs=[(b["o0"], xt, 1.0, 0.5, [(b["k1"], 0.25)])])
        if fused:
            ops.linear_rhs(zt, Wtt, xt, rhs=False, stage=st)
        else:
            ops.stage_apply(st, ax, xt, xt)
        outs.append(b["o0"])
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("K,C", [(64, 128), (20, 80)])
def test_wide_stage_takes_the_fallback(K, C):
    """A stage with error rows: GNPDE_EUNSUPPORTED at the ABI, f + stage_apply in the binding."""
    R = 100
    z, Wt, x, x0 = _operands(R, K, C, 23)
    zt, Wtt, xt, x0t = T(z), T(Wt), T(x), T(x0)
    al = torch.tensor(0.4, device=DEV)

    def stage(b, rows):
        return ops.Stage(outs=[(b["o0"], b["y0"], 1.0, 0.5, [(b["k1"], 0.25)])],
                         err=(rows, (None, 0.0, 0.3, [(b["k1"], -0.3)]), b["y0"], 0, 1e-4, 1e-3))

    got = []
    for via_ops in (True, False):
        b, rows = _stage_bufs(R, C, 29), torch.zeros(R, dtype=torch.float64, device=DEV)
        st = stage(b, rows)
        assert st.wide
        if via_ops:
            assert ops.linear_rhs(zt, Wtt, xt, alpha=al, stage=st) is None
        else:
            ops.stage_apply(st, ops.linear_rhs(zt, Wtt, xt, alpha=al), xt, xt)
        got.append((b["o0"], rows))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    _, fw = _want(z, Wt, x, None, 0.4, 0.0, True)
    bn = {k: v.double().cpu().numpy() for k, v in _stage_bufs(R, C, 29).items()}
    y1 = bn["y0"] + 0.5 * fw + 0.25 * bn["k1"]
    assert rel(got[0][0], y1) <= RTOL
    e = 0.3 * fw - 0.3 * bn["k1"]
    rows_want = ((e / (1e-4 + 1e-3 * np.maximum(np.abs(bn["y0"]), np.abs(y1)))) ** 2).sum(axis=1)
    assert rel(got[0][1], rows_want) <= 1e-3  # squares of fp32 quotients with a small tolerance
    # the entry point itself refuses the stage (and a coefficient scale)
    for st in (stage(_stage_bufs(R, C, 29), torch.zeros(R, dtype=torch.float64, device=DEV)),
               ops.Stage(outs=[(b["o0"], None, 0.0, 1.0, [])], scale=torch.tensor(0.5, device=DEV))):
        f = torch.empty(R, C, device=DEV)
        vp = _lib.ctypes.c_void_p
        rc = _lib.call_rc("gnpde_linear_rhs_f32", vp(zt.data_ptr()), R, K, K, vp(Wtt.data_ptr()), C,
                          vp(xt.data_ptr()), C, vp(0), C, vp(al.reshape(1).data_ptr()), vp(0), _lib.EPI_RHS,
                          vp(f.data_ptr()), C, _lib.ctypes.byref(st.struct(xt)), vp(0))
        assert rc == _lib.EUNSUPPORTED


# --------------------------------------------------------------------------- the ODE function
def _load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, mix=True, **kw):
    return dict(OPT, hidden_dim=m["C"], heads=m["heads"], attention_dim=m["attention_dim"], function='GAT',
                attention_norm_idx=m["attention_norm_idx"], add_source=m["add_source"],
                no_alpha_sigmoid=m["no_alpha_sigmoid"], leaky_relu_slope=m["leaky_relu_slope"], gnpde_gat=True,
                mix_features=mix, gnpde_gat_mix_features=True, **kw)


def _make(d, m, mix=True):
    C = m["C"]
    func = gnpde.set_function(_opt(m, mix))(C, C, _opt(m, mix), DEV).to(DEV)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
        lay.W.copy_(T(d["W"]))
        lay.Wout.copy_(T(d["Wout"]))
        lay.a.copy_(T(d["a"]).view(1, -1, 1, 1))
    func.edge_index = T(d["edge_index"])
    func.x0 = T(d["x0"])
    return func


@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_gat_mix_rhs_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    with torch.no_grad():
        att, wx = func.multihead_att_layer(T(d["x"]), func.edge_index)
        f = func(torch.tensor(0.0), T(d["x"]))
        ax = func.multiply_attention(T(d["x"]), att, wx)
        ax2 = func.multiply_attention(T(d["x"]), att)
    assert att.shape == d["attention"].shape and wx.shape == d["wx"].shape and func.nfe == 1
    e_att = float(np.abs(att.double().cpu().numpy() - d["attention"]).max())
    e_wx, e_f = rel(wx, d["wx"]), rel(f, d["f"])
    bar = max(RTOL, float(np.abs(d["f_ref32"] - d["f"]).max() / np.abs(d["f"]).max()))
    print("%s: attention err %.3e, wx rel err %.3e, f rel err %.3e (bar %.3e)" % (os.path.basename(path), e_att, e_wx,
                                                                                 e_f, bar))
    assert e_att <= ATT_ATOL
    assert e_wx <= PROD_RTOL
    assert e_f <= bar
    want_ax = M.gat_mix_multiply(d["edge_index"], d["attention"], d["wx"], d["Wout"])
    assert rel(ax, want_ax) <= RTOL
    assert torch.equal(ax, ax2)
    with torch.no_grad():  # repeated evaluations: the same bits
        assert torch.equal(func(torch.tensor(0.0), T(d["x"])), f)


def test_bf16_state_raises():
    d, m = _load(os.path.join(GOLDEN, "gatmix_n0_h2.npz"))
    func = _make(d, m)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp32"):
        func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))


@pytest.mark.parametrize("norm_idx", [0, 1])
@pytest.mark.parametrize("C", [16, 128])
def test_hub_and_long_groups(C, norm_idx):
    """The hub graph of test_gpu_gat.py::test_hub_and_long_groups (a source and a destination
    of 1,100 edges, long groups) at attention_dim 16."""
    N, h, att = 64, 2, 16
    rng = np.random.default_rng(7 + C + norm_idx)
    ei = rng.integers(0, N, size=(1, 2, 2500))
    ei[0, 0, :1100] = 3
    ei[0, 1, 1100:2200] = 5
    ei[0, 0, 2200:2300] = 9
    ei[0, 1, 2300:2400] = 11
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    x0 = rng.standard_normal((1, N, C)).astype(np.float32)
    W = (rng.standard_normal((C, att)) * 0.3 / np.sqrt(C / 12.0)).astype(np.float32)
    Wout = (rng.standard_normal((att, C)) * 0.3).astype(np.float32)
    a = (rng.standard_normal(2 * att // h) * 0.5).astype(np.float32)
    m = dict(C=C, heads=h, attention_dim=att, attention_norm_idx=norm_idx, add_source=True, no_alpha_sigmoid=False,
             leaky_relu_slope=0.2)
    d = dict(alpha_train=0.3, beta_train=0.6, W=W, Wout=Wout, a=a, edge_index=ei, x0=x0)
    func = _make(d, m)
    with torch.no_grad():
        f = func(torch.tensor(0.0), T(x))
        f2 = func(torch.tensor(0.0), T(x))
    want = M.gat_mix_rhs(ei, x, x0, W, Wout, a, h, norm_idx, 0.2, 0.3, 0.6, add_source=True)
    assert rel(f, want) <= RTOL
    assert torch.equal(f, f2)


def _block(cls, m, ei, N, **kw):
    opt = _opt(m, max_nfe=10 ** 6, **kw)
    blk = cls(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    rng = np.random.default_rng(11)
    C, att, h = m["C"], m["attention_dim"], m["heads"]
    W = (rng.standard_normal((C, att)) * 0.3).astype(np.float32)
    Wout = (rng.standard_normal((att, C)) * 0.3).astype(np.float32)
    a = (rng.standard_normal(2 * att // h) * 0.5).astype(np.float32)
    with torch.no_grad():
        lay = blk.odefunc.multihead_att_layer
        lay.W.copy_(T(W))
        lay.Wout.copy_(T(Wout))
        lay.a.copy_(T(a).view(1, -1, 1, 1))
        blk.odefunc.alpha_train.fill_(0.5)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N)
    return blk, data, W, Wout, a


@pytest.mark.parametrize("name", ["gatmix_n0_h2", "gatmix_n1_h1_b3"])
def test_stage_fusion_in_constant_block(name):
    """rk4 (C = 12: the plain kernel of gnpde_linear_rhs_f32; C = 64, attention_dim 16: the
    split-bf16 one), replayed from captured graphs; dopri5: the adaptive stages through f +
    stage_apply."""
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    ei, x, N = d["edge_index"][:1], d["x"][:1], m["N"]
    ni = m["attention_norm_idx"]
    eo, _ = _prep_oracle(ei, N)
    blk, data, W, Wout, a = _block(gnpde.ConstantODEblock, m, ei, N, method='rk4', step_size=0.25)
    assert blk.odefunc.multihead_att_layer.mix
    f = lambda t, y: M.gat_mix_rhs(eo, y, None, W, Wout, a, m["heads"], ni, m["leaky_relu_slope"], 0.5,  # noqa: E731
                                   0.0)
    with torch.no_grad():
        z1 = blk(T(x), data)
        z2 = blk(T(x), data)  # the captured step graphs
    torch.cuda.synchronize()
    assert rel(z1, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL
    assert torch.equal(z1, z2)
    blk, data, W, Wout, a = _block(gnpde.ConstantODEblock, m, ei, N, method='dopri5')
    blk.rtol, blk.atol = 1e-3, 1e-4
    with torch.no_grad():
        z = blk(T(x), data)
    n_got = gi.odeint.last_n_steps
    want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
    assert n_got == n_want
    assert rel(z, want[-1] if np.ndim(want) == x.ndim + 1 else want) <= RTOL


def test_hard_attention_block_with_the_mix_function():
    d, m = _load(os.path.join(GOLDEN, "gatmix_n0_h2.npz"))
    ei, x, N = d["edge_index"], d["x"], m["N"]
    blk, data, W, Wout, a = _block(gnpde.HardAttODEblock, m, ei, N, block='hard_attention', att_samp_pct=0.5,
                                   method='rk4', step_size=0.25)
    assert not hasattr(blk, 'multihead_att_layer')
    with torch.no_grad():
        z = blk(T(x), data)
    eo, _ = _prep_oracle(ei, N)
    want_att = G.gat_attention(x, eo, W, a, m["heads"], 0, m["leaky_relu_slope"]).mean(axis=2)
    assert np.abs(blk.odefunc.attention_weights.double().cpu().numpy() - want_att).max() <= ATT_ATOL
    f = lambda t, y: M.gat_mix_rhs(eo, y, None, W, Wout, a, m["heads"], 0, m["leaky_relu_slope"], 0.5,  # noqa: E731
                                   0.0)
    assert rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL


def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e" % (name, err, tol))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_gat_mix_grad_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    names = ("x", "alpha_train", "beta_train", "W", "a", "Wout")
    scale = max(float(np.abs(d["g_" + k]).max()) for k in names)
    _check("x", x.grad, d["g_x"], scale)
    _check("alpha_train", func.alpha_train.grad, d["g_alpha_train"], scale)
    _check("beta_train", func.beta_train.grad, d["g_beta_train"], scale)
    _check("W", lay.W.grad, d["g_W"], scale)
    _check("a", lay.a.grad, d["g_a"], scale)
    _check("Wout", lay.Wout.grad, d["g_Wout"], scale)


def test_layer_wx_is_differentiable():
    """The layer's second output under autograd: d <g, x W> = (g W^T, x^T g)."""
    d, m = _load(os.path.join(GOLDEN, "gatmixgrad_n0_h2.npz"))
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    _, wx = lay(x, func.edge_index)
    g = np.random.default_rng(2).standard_normal(d["wx"].shape).astype(np.float32)
    (wx * T(g)).sum().backward()
    gd, xd, Wd = g.astype(np.float64), d["x"].astype(np.float64), d["W"].astype(np.float64)
    assert rel(x.grad, gd @ Wd.T) <= RTOL
    assert rel(lay.W.grad, np.einsum('bnc,bna->ca', xd, gd)) <= RTOL


def test_mix_features_off_leaves_wout_without_gradient():
    d, m = _load(os.path.join(GOLDEN, "gatmixgrad_n0_h2.npz"))
    func = _make(d, m, mix=False)
    lay = func.multihead_att_layer
    assert not lay.mix
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    want = G.gat_rhs(d["edge_index"], d["x"], d["x0"], d["W"], d["a"], m["heads"], m["attention_norm_idx"],
                     m["leaky_relu_slope"], float(d["alpha_train"]), float(d["beta_train"]),
                     add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"])
    assert rel(f, want) <= RTOL
    (f * T(d["gout"])).sum().backward()
    assert lay.Wout.grad is None or not bool(lay.Wout.grad.any())
    assert lay.W.grad is not None and bool(lay.W.grad.any())
