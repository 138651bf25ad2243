"""GPU: the GAT attention ODE function (gnpde.function_GAT_attention) against the
reference's own float64 run (tests/golden/gat/gat_*.npz, gatgrad_*.npz) and the fp64
restatement tests/gat_oracle.py.

Bars: attention <= 2e-5 absolute, f <= 1e-5 relative (RTOL of test_gpu_parity.py);
``gat_n1_wide`` (|pre-activation| up to ~30): max(1e-5, the deviation of the fixture's
own fp32 reference run from its fp64 run) — measured from the fixture: 1.4e-7, so the
bar is 1e-5 there too.  Gradients under the rule of test_gpu_grad_golden.py.  The
fused K1 (gnpde_attn_gat_rhs_f32) equals the weights pass + the plain K1 bit for bit."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gat_oracle as G
import gnpde
import gnpde.integrator as gi
import gnpde_oracle as O
from conftest import GOLDEN as _GOLDEN
from gnpde import ops
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "gat")
ATT_ATOL = 2e-5
GRAD_RTOL = 1e-4
BF16_GATE = 2e-2
FWD = sorted(glob.glob(os.path.join(GOLDEN, "gat_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "gatgrad_*.npz")))


def _load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, **kw):
    return dict(OPT, hidden_dim=m["C"], heads=m["heads"], attention_dim=m["attention_dim"], function='GAT',
                attention_norm_idx=m["attention_norm_idx"], add_source=m["add_source"],
                no_alpha_sigmoid=m["no_alpha_sigmoid"], leaky_relu_slope=m["leaky_relu_slope"], gnpde_gat=True, **kw)


def _make(d, m):
    C = m["C"]
    func = gnpde.set_function(_opt(m))(C, C, _opt(m), DEV).to(DEV)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
        lay.W.copy_(T(d["W"]))
        lay.a.copy_(T(d["a"]).view(1, -1, 1, 1))
    func.edge_index = T(d["edge_index"])
    func.x0 = T(d["x0"])
    return func


def _ns(d, m, g, x=None):
    return ops.gat_scores(g, T(d["x"]) if x is None else x, T(d["W"]), T(d["a"]), m["heads"], m["leaky_relu_slope"])


@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_gat_rhs_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    assert isinstance(func, gnpde.ODEFuncAtt)
    with torch.no_grad():
        att, values = func.multihead_att_layer(T(d["x"]), func.edge_index)
        f = func(torch.tensor(0.0), T(d["x"]))
        ax = func.multiply_attention(T(d["x"]), att)
    assert values is None and att.shape == d["attention"].shape and func.nfe == 1
    e_att = float(np.abs(att.double().cpu().numpy() - d["attention"]).max())
    e_f = rel(f, d["f"])
    bar = max(RTOL, float(np.abs(d["f_ref32"] - d["f"]).max() / np.abs(d["f"]).max()))
    print("%s: attention err %.3e, f rel err %.3e (bar %.3e)" % (os.path.basename(path), e_att, e_f, bar))
    assert e_att <= ATT_ATOL
    assert e_f <= (bar if os.path.basename(path) == "gat_n1_wide.npz" else RTOL)
    want_ax = O.aggregate(d["edge_index"], d["attention"].mean(axis=2), d["x"])
    assert rel(ax, want_ax) <= RTOL


def test_gat_max_nfe():
    d, m = _load(os.path.join(GOLDEN, "gat_n0_h2.npz"))
    func = _make(d, m)
    func.opt = dict(func.opt, max_nfe=1)
    with torch.no_grad():
        func(torch.tensor(0.0), T(d["x"]))
        func(torch.tensor(0.0), T(d["x"]))
        with pytest.raises(gnpde.MaxNFEException):
            func(torch.tensor(0.0), T(d["x"]))


@pytest.mark.parametrize("name", ["gat_n1_c128", "gat_n0_c128_h4"])
def test_fused_equals_unfused_bitwise(name):
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    g = ops.GraphCSR(T(d["edge_index"]), m["N"])
    x = T(d["x"])
    ns = _ns(d, m, g)
    a = torch.tensor(0.3, device=DEV)
    ni = m["attention_norm_idx"]
    fused = ops.attn_rhs(g, ns, None, None, ni, x, alpha=a, fuse=True)
    unfused = ops.attn_rhs(g, ns, None, None, ni, x, alpha=a, fuse=False)
    torch.cuda.synchronize()
    assert torch.equal(fused, unfused)
    for _ in range(2):
        assert torch.equal(ops.attn_rhs(g, _ns(d, m, g), None, None, ni, x, alpha=a, fuse=True), fused)
    want = G.gat_rhs(d["edge_index"], d["x"], None, d["W"], d["a"], m["heads"], ni, m["leaky_relu_slope"], 0.3, 0.0)
    assert rel(fused, want) <= RTOL


def test_unsupported_head_count_takes_the_unfused_path():
    """Head counts outside the fused kernel return GNPDE_EUNSUPPORTED at the ABI."""
    from gnpde import _lib
    vp = _lib.ctypes.c_void_p
    rc = _lib.call_rc("gnpde_attn_gat_rhs_f32", vp(0), 0, vp(0), 0, vp(0), vp(0), vp(0), vp(0), 0, 9, 0.2, 4, vp(16), 4,
                      vp(0), 0, vp(0), vp(0), 0, vp(64), 4, vp(0), 0, None, vp(0))
    assert rc == _lib.EUNSUPPORTED


@pytest.mark.parametrize("norm_idx", [0, 1])
@pytest.mark.parametrize("C", [16, 128])
def test_hub_and_long_groups(C, norm_idx):
    """N = 64 with one source of 1,100 out-edges and one destination of 1,100 in-edges
    (duplicates allowed) + 300 more edges (100 from one source, 100 into one destination, 100
    random; every other endpoint random): K1 splits rows at 16 edges below 50,000
    rows (hub combines), the statistics plan has hub chunks (> 512 edges) and long items
    (65..512)."""
    N, h, att = 64, 2, 16
    rng = np.random.default_rng(7 + C + norm_idx)
    ei = rng.integers(0, N, size=(1, 2, 2500))
    ei[0, 0, :1100] = 3
    ei[0, 1, 1100:2200] = 5
    ei[0, 0, 2200:2300] = 9    # a source and a destination of 100+ edges among the random ones:
    ei[0, 1, 2300:2400] = 11   # long items of the statistics plan in either grouping
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    W = (rng.standard_normal((C, att)) * 0.3 / np.sqrt(C / 12.0)).astype(np.float32)
    a = (rng.standard_normal(2 * att // h) * 0.5).astype(np.float32)
    g = ops.GraphCSR(T(ei), N)
    al = torch.tensor(0.3, device=DEV)
    ns = ops.gat_scores(g, T(x), T(W), T(a), h, 0.2)
    fused = ops.attn_rhs(g, ns, None, None, norm_idx, T(x), alpha=al, fuse=True)
    unfused = ops.attn_rhs(g, ns, None, None, norm_idx, T(x), alpha=al, fuse=False)
    torch.cuda.synchronize()
    want = G.gat_rhs(ei, x, None, W, a, h, norm_idx, 0.2, 0.3, 0.0)
    assert rel(fused, want) <= RTOL
    assert torch.equal(fused, unfused)
    for _ in range(2):
        ns2 = ops.gat_scores(g, T(x), T(W), T(a), h, 0.2)
        assert torch.equal(ops.attn_rhs(g, ns2, None, None, norm_idx, T(x), alpha=al, fuse=True), fused)
    att_g = ops.edge_attention(g, ns, *ops.softmax_stats(g, ns, norm_idx), norm_idx)
    assert np.abs(att_g.double().cpu().numpy() - G.gat_attention(x, ei, W, a, h, norm_idx, 0.2)).max() <= ATT_ATOL
    # the per-group statistics kernels (gnpde_softmax_stats_f32) take the score mode too: the same
    # max; 1/sum within the fp32 rounding of summing <= 1,200 positive terms in another order
    # (about sqrt(n) * 2^-24 * a few: 1e-5 bounds it with room)
    m1, rl1 = ops.softmax_stats(g, ns, norm_idx)
    m2, rl2 = ops.softmax_stats(g, ns, norm_idx, seg=False)
    nz = torch.from_numpy(np.bincount(ei[0, norm_idx], minlength=N) > 0).to(DEV)
    assert torch.equal(m1[nz], m2[nz]) and torch.allclose(rl1[nz], rl2[nz], rtol=1e-5, atol=0)
    torch.cuda.synchronize()
    grouped = g.csr if norm_idx == 0 else g.csc
    plans = [p for p in grouped._seg_plans.values() if p.n_hub or p.n_long]
    assert plans and all(p.n_hub >= 2 and p.n_long >= 1 and p.n_chunk == 0 for p in plans)
    assert g.csr.plan.n_heavy >= 1
    for p in plans + [g.csr.plan]:
        assert int(p.heavy.view(-1, 4)[:p.n_heavy, 3].abs().sum()) == 0  # every ticket back at 0


def _block(cls, m, ei, N, **kw):
    opt = _opt(m, max_nfe=10 ** 6, **kw)
    blk = cls(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    rng = np.random.default_rng(11)
    C, att, h = m["C"], m["attention_dim"], m["heads"]
    W = (rng.standard_normal((C, att)) * 0.3).astype(np.float32)
    a = (rng.standard_normal(2 * att // h) * 0.5).astype(np.float32)
    with torch.no_grad():
        lay = blk.odefunc.multihead_att_layer
        lay.W.copy_(T(W))
        lay.a.copy_(T(a).view(1, -1, 1, 1))
        blk.odefunc.alpha_train.fill_(0.5)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N)
    return blk, data, W, a


def test_stage_fusion_in_constant_block():
    d, m = _load(os.path.join(GOLDEN, "gat_n0_h2.npz"))
    ei, x, N = d["edge_index"], d["x"], m["N"]
    eo, _ = _prep_oracle(ei, N)
    blk, data, W, a = _block(gnpde.ConstantODEblock, m, ei, N, method='rk4', step_size=0.25)
    f = lambda t, y: G.gat_rhs(eo, y, None, W, a, m["heads"], 0, m["leaky_relu_slope"], 0.5, 0.0)  # noqa: E731
    with torch.no_grad():
        z1 = blk(T(x), data)
        z2 = blk(T(x), data)  # the captured step graphs
    torch.cuda.synchronize()
    assert rel(z1, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL
    assert torch.equal(z1, z2)
    blk, data, W, a = _block(gnpde.ConstantODEblock, m, ei, N, method='dopri5')
    blk.rtol, blk.atol = 1e-3, 1e-4
    with torch.no_grad():
        z = blk(T(x), data)
    n_got = gi.odeint.last_n_steps
    want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
    assert n_got == n_want
    assert rel(z, want[-1] if np.ndim(want) == x.ndim + 1 else want) <= RTOL


def test_hard_attention_block_with_gat_function():
    """The branch of HardAttODEblock that names GAT: the attention comes once from
    odefunc.multihead_att_layer, the integrated RHS is then GAT."""
    d, m = _load(os.path.join(GOLDEN, "gat_n0_h2.npz"))
    ei, x, N = d["edge_index"], d["x"], m["N"]
    blk, data, W, a = _block(gnpde.HardAttODEblock, m, ei, N, block='hard_attention', att_samp_pct=0.5,
                             method='rk4', step_size=0.25)
    assert not hasattr(blk, 'multihead_att_layer')
    with torch.no_grad():
        z = blk(T(x), data)
    eo, _ = _prep_oracle(ei, N)
    want_att = G.gat_attention(x, eo, W, a, m["heads"], 0, m["leaky_relu_slope"]).mean(axis=2)
    assert np.abs(blk.odefunc.attention_weights.double().cpu().numpy() - want_att).max() <= ATT_ATOL
    f = lambda t, y: G.gat_rhs(eo, y, None, W, a, m["heads"], 0, m["leaky_relu_slope"], 0.5, 0.0)  # noqa: E731
    assert rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL


def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e" % (name, err, tol))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_gat_grad_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    names = ("x", "alpha_train", "beta_train", "W", "a")
    scale = max(float(np.abs(d["g_" + k]).max()) for k in names)
    _check("x", x.grad, d["g_x"], scale)
    _check("alpha_train", func.alpha_train.grad, d["g_alpha_train"], scale)
    _check("beta_train", func.beta_train.grad, d["g_beta_train"], scale)
    _check("W", lay.W.grad, d["g_W"], scale)
    _check("a", lay.a.grad, d["g_a"], scale)
    assert lay.Wout.grad is None or not bool(lay.Wout.grad.any())


def test_bf16_state():
    d, m = _load(os.path.join(GOLDEN, "gat_n1_c128.npz"))
    func = _make(d, m)
    with torch.no_grad():
        f32 = func(torch.tensor(0.0), T(d["x"]))
        fb = func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))
    assert fb.dtype == torch.bfloat16
    scale = float(f32.abs().max())
    assert float((fb.float() - f32).abs().max()) <= BF16_GATE * scale
