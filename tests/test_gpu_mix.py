"""GPU: transformer mix_features — the per-head aggregation gnpde_head_aggregate_f32
(ops.head_aggregate), the output product with a bias gnpde_linear_rhs_bias_f32
(ops.linear_rhs(bias=...)) and the ODE function against the reference's own pieces in
float64 (tests/golden/mix/mix_*.npz, mixgrad_*.npz) and the fp64 restatement
tests/mix_oracle.py.

Bars (the project's own): f and z <= RTOL = 1e-5 as max error over max reference, or for f
the deviation of the fixture's own fp32 reference run where that is larger (the rule of
test_gpu_gat_mix.py); attention <= 2e-5 absolute; v and the plain product <= 2e-6; gradients
under the rule of test_gpu_grad_golden.py.  A 256-edge fp32 chain is a few 1e-7 from
float64; a dropped edge is about 1e-2."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import gnpde.integrator as gi
import gnpde_oracle as O
import mix_oracle as M
from conftest import GOLDEN as _GOLDEN
from gnpde import _lib, ops
from test_gpu_long_items import CHUNK, ORDERS, Host, build_graph
from test_gpu_parity import DEV, OPT, RTOL, T, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "mix")
PROD_RTOL = 2e-6
ATT_ATOL = 2e-5
GRAD_RTOL = 1e-4
FWD = sorted(glob.glob(os.path.join(GOLDEN, "mix_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "mixgrad_*.npz")))
PARAMS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wout", "bout")
# (heads, dk): the fast path at att/4 = 4 .. 64 lanes, then the plain kernel — heads = 3, dk % 4 != 0 (twice)
# and att = 512 beyond the 64 lanes of a wavefront
HEAD_SHAPES = [(1, 16), (2, 8), (2, 64), (8, 16), (4, 32), (8, 32), (3, 4), (2, 5), (4, 6), (8, 64)]
ROW_LENGTHS = (0, 1, 2, 15, 16, 17, 40)


# --------------------------------------------------------------------------- the aggregation kernel
def _small_graph(B, seed):
    """Rows of 0, 1, 2, 15, 16, 17 and 40 edges (several of each, shuffled), duplicates and
    self loops, on a graph small enough for the automatic 16-edge items: a 17-edge row is two
    chunks, a 40-edge row three."""
    rng = np.random.default_rng(seed)
    lens = np.repeat(np.array(ROW_LENGTHS), 5)
    lens = lens[rng.permutation(lens.size)]
    N = lens.size
    eis = []
    for _ in range(B):
        src = np.repeat(np.arange(N), lens)
        dst = rng.integers(0, N, size=src.size)
        first = np.cumsum(lens) - lens
        dst[first[lens > 0]] = np.arange(N)[lens > 0]                       # self loops
        two = first[lens >= 2]
        dst[two + 1] = dst[two]                                             # a duplicate edge in every longer row
        p = rng.permutation(src.size)
        eis.append(np.stack([src[p], dst[p]]))
    return np.stack(eis), N, lens


def _z_want(ei, wh_coo, v):
    return M.head_aggregate(ei, wh_coo, v)


@pytest.mark.parametrize("heads,dk", HEAD_SHAPES)
@pytest.mark.parametrize("B", [1, 2])
def test_head_aggregate_vs_fp64(B, heads, dk):
    ei, N, lens = _small_graph(B, 31 * heads + dk)
    g = ops.GraphCSR(T(ei), N)
    assert g.chunk == 16 and g.csr.plan.n_heavy == B * int((lens > 16).sum())
    assert bool(_lib.fn("gnpde_head_aggregate_fast")(heads, dk)) == ((heads, dk) in HEAD_SHAPES[:6])
    rng = np.random.default_rng(heads + dk)
    att = heads * dk
    v = rng.standard_normal((B, N, att)).astype(np.float32)
    w = rng.uniform(0.05, 1.0, size=(B, ei.shape[2], heads)).astype(np.float32)
    want = _z_want(ei, w, v)
    z = ops.head_aggregate(g, T(w), T(v), coo=True)
    assert tuple(z.shape) == (B, N, dk)
    e = rel(z, want)
    print("B=%d heads=%d dk=%d: z err %.3e" % (B, heads, dk, e))
    assert e <= RTOL
    assert not bool(z.view(B, N, dk)[:, lens == 0].any())                   # rows without edges
    # the same weights in aggregation-CSR order [nnz, heads]
    w_csr = T(w).view(-1, heads)[g.csr.perm.long()].contiguous()
    z2 = ops.head_aggregate(g, w_csr, T(v))
    assert torch.equal(z2, z)
    for _ in range(3):                                                      # repeated launches: the same bits
        assert torch.equal(ops.head_aggregate(g, T(w), T(v), coo=True), z)
    torch.cuda.synchronize()


_HOST = []


def _host():
    if not _HOST:
        _HOST.append(Host())
    return _HOST[0]


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("heads,dk", [(2, 64), (8, 16)])
def test_head_aggregate_at_production_item_length(heads, dk, order):
    """The graph of test_gpu_long_items.py (rows of 0 .. 700 edges, 255 / 256 / 257 among them)
    with chunk = 256 under both plan orders."""
    host = _host()
    g = build_graph(host.ei, host.N, order)
    assert g.chunk == CHUNK and g.csr.plan.n_heavy > 0
    rng = np.random.default_rng(5 + heads)
    v = rng.standard_normal((1, host.N, heads * dk)).astype(np.float32)
    w = (rng.uniform(0.1, 1.0, size=(1, host.E, heads)) / 8.0).astype(np.float32)
    z = ops.head_aggregate(g, T(w), T(v), coo=True)
    e = rel(z, _z_want(host.ei, w, v))
    print("order=%s heads=%d dk=%d: z err %.3e" % (order, heads, dk, e))
    assert e <= RTOL
    for _ in range(2):
        assert torch.equal(ops.head_aggregate(g, T(w), T(v), coo=True), z)


@pytest.mark.parametrize("heads,dk", [(2, 8), (8, 16), (3, 4)])
def test_equal_heads_fold_to_the_plain_k1(heads, dk):
    """With the same weight in every head, z is the plain K1 over v folded over the heads."""
    ei, N, _ = _small_graph(1, 77)
    g = ops.GraphCSR(T(ei), N)
    rng = np.random.default_rng(9)
    v = rng.standard_normal((1, N, heads * dk)).astype(np.float32)
    w = rng.uniform(0.05, 1.0, size=(1, ei.shape[2])).astype(np.float32)
    wh = np.repeat(w[:, :, None], heads, axis=2)
    z = ops.head_aggregate(g, T(wh), T(v), coo=True)
    full = ops.spmm_rhs(g, g.gather_weights(T(w)), T(v), rhs=False)
    fold = full.double().view(1, N, heads, dk).mean(dim=2).cpu().numpy()
    assert rel(z, fold) <= RTOL


@pytest.mark.parametrize("mode,norm_idx", [("reference", 0), ("reference", 1), ("per_edge", 0), ("per_edge", 1)])
def test_head_mean_of_the_head_weights_is_attn_weights(mode, norm_idx):
    N, E, C, h, att = 200, 1500, 32, 4, 32
    rng = np.random.default_rng(13 + norm_idx)
    ei = rng.integers(0, N, size=(1, 2, E))
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    Wq, Wk = [(rng.standard_normal((att, C)) * 0.1).astype(np.float32) for _ in range(2)]
    bq, bk = [(rng.standard_normal(att) * 0.1).astype(np.float32) for _ in range(2)]
    g = ops.GraphCSR(T(ei), N)
    ns = ops.node_scores(g, T(x), T(Wq), T(bq), T(Wk), T(bk), h, 'scaled_dot', mode)
    m, rl = ops.softmax_stats(g, ns, norm_idx)
    wh = ops.head_weights(g, ns, m, rl, norm_idx)
    assert tuple(wh.shape) == (g.nnz, h)
    w = ops.attn_weights(g, ns, m, rl, norm_idx)
    assert rel(w[:g.nnz], wh.double().mean(dim=1).cpu().numpy()) <= 1e-6
    # the CSR-order output is the layer's attention at perm, bit for bit
    att = ops.edge_attention(g, ns, m, rl, norm_idx)
    assert torch.equal(att.view(-1, h)[g.csr.perm.long()], wh)


# --------------------------------------------------------------------------- the output product with a bias
BIAS_SHAPES = [(16, 64), (64, 128), (4, 12), (20, 80), (16, 162)]


def _operands(R, K, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((R, K)).astype(np.float32)
    Wt = (rng.standard_normal((C, K)) * 0.3).astype(np.float32)
    bias = (rng.standard_normal(C) * 0.3).astype(np.float32)
    x = rng.standard_normal((R, C)).astype(np.float32)
    x0 = rng.standard_normal((R, C)).astype(np.float32)
    return z, Wt, bias, x, x0


def _want(z, Wt, bias, x, x0, alpha, beta, sigmoid):
    ax = z.astype(np.float64) @ Wt.astype(np.float64).T + bias.astype(np.float64)
    a = 1.0 / (1.0 + np.exp(-alpha)) if sigmoid else alpha
    f = a * (ax - x)
    return ax, (f + beta * x0 if x0 is not None else f)


@pytest.mark.parametrize("K,C", BIAS_SHAPES)
@pytest.mark.parametrize("R", [1, 33, 100])
def test_linear_rhs_bias_vs_fp64(R, K, C):
    z, Wt, bias, x, x0 = _operands(R, K, C, 100 * R + K + C)
    al, be = torch.tensor(0.4, device=DEV), torch.tensor(-0.7, device=DEV)
    ax_want, _ = _want(z, Wt, bias, x, None, 0.4, 0.0, True)
    ax = ops.linear_rhs(T(z), T(Wt), None, rhs=False, bias=T(bias))
    e = rel(ax, ax_want)
    print("R=%d K=%d C=%d: product err %.3e" % (R, K, C, e))
    assert e <= PROD_RTOL
    for with_x0 in (False, True):
        for sigmoid in (True, False):
            f = ops.linear_rhs(T(z), T(Wt), T(x), x0=T(x0) if with_x0 else None, alpha=al, beta=be,
                               alpha_sigmoid=sigmoid, add_source=with_x0, bias=T(bias))
            _, want = _want(z, Wt, bias, x, x0 if with_x0 else None, 0.4, -0.7, sigmoid)
            assert rel(f, want) <= RTOL
    # bias=None is the old entry, bit for bit — and the new entry with a NULL bias as well
    kw = dict(x0=T(x0), alpha=al, beta=be, add_source=True)
    old = ops.linear_rhs(T(z), T(Wt), T(x), **kw)
    out = torch.empty(R, C, device=DEV)
    vp = _lib.ctypes.c_void_p
    zt, Wtt, xt, x0t = T(z), T(Wt), T(x), T(x0)
    for name, extra in (("gnpde_linear_rhs_f32", ()), ("gnpde_linear_rhs_bias_f32", (vp(0),))):
        out.zero_()
        _lib.call(name, vp(zt.data_ptr()), R, K, K, vp(Wtt.data_ptr()), C, *extra, vp(xt.data_ptr()), C,
                  vp(x0t.data_ptr()), C, vp(al.reshape(1).data_ptr()), vp(be.reshape(1).data_ptr()),
                  ops._flags(True, True, True), vp(out.data_ptr()), C, None,
                  vp(torch.cuda.current_stream().cuda_stream))
        assert torch.equal(out, old)
    torch.cuda.synchronize()


@pytest.mark.parametrize("R,K,C", [(100, 64, 128), (33, 16, 64), (100, 20, 80), (33, 16, 162)])
def test_fused_stage_with_bias_equals_f_then_stage_apply(R, K, C):
    z, Wt, bias, x, x0 = _operands(R, K, C, R + K + C)
    zt, Wtt, bt, xt, x0t = T(z), T(Wt), T(bias), T(x), T(x0)
    kw = dict(x0=x0t, alpha=torch.tensor(0.4, device=DEV), beta=torch.tensor(-0.7, device=DEV), add_source=True,
              bias=bt)
    f = ops.linear_rhs(zt, Wtt, xt, **kw)
    runs = []
    for fused in (True, False, True):
        b = {k: T(np.random.default_rng(17).standard_normal((R, C)).astype(np.float32) + i)
             for i, k in enumerate(("y0", "k1", "k2", "o0", "o1", "fo"))}
        st = ops.Stage(f_out=b["fo"], outs=[(b["o0"], b["y0"], 1.0, 0.375, [(b["k1"], 0.75), (b["k2"], -1.5)]),
                                            (b["o1"], xt, 0.5, -0.25, [(b["k2"], 2.0)])])
        assert not st.wide
        if fused:
            assert ops.linear_rhs(zt, Wtt, xt, stage=st, **kw) is None
        else:
            ops.stage_apply(st, f, xt, xt)
        runs.append([b[k].clone() for k in ("fo", "o0", "o1")])
    for got in (runs[0], runs[2]):
        for u, w in zip(got, runs[1]):
            assert torch.equal(u, w)
    assert torch.equal(runs[0][0], f)
    _, fw = _want(z, Wt, bias, x, x0, 0.4, -0.7, True)
    assert rel(runs[0][0], fw) <= RTOL


# --------------------------------------------------------------------------- the ODE function
def _load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, mix=True, **kw):
    o = dict(OPT, hidden_dim=m["C"], heads=m["heads"], attention_dim=m["attention_dim"], function='transformer',
             attention_norm_idx=m["attention_norm_idx"], attention_type=m["attention_type"],
             attention_score_mode=m["score_mode"], add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"],
             mix_features=mix, gnpde_mix_features=True, **kw)
    if m["square_plus"]:
        o.update(square_plus=True, gnpde_square_plus=True)
    return o


def _make(d, m, mix=True, **kw):
    C = m["C"]
    func = gnpde.ODEFuncTransformerAtt(C, C, _opt(m, mix, **kw), DEV).to(DEV)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
        for n, p in _params(lay).items():
            p.copy_(T(d[n]))
        if m["attention_type"] == "exp_kernel":
            lay.output_var.fill_(m["output_var"])
            lay.lengthscale.fill_(m["lengthscale"])
    func.edge_index = T(d["edge_index"])
    func.x0 = T(d["x0"])
    return func


def _params(lay):
    return dict(Wq=lay.Q.weight, bq=lay.Q.bias, Wk=lay.K.weight, bk=lay.K.bias, Wv=lay.V.weight, bv=lay.V.bias,
                Wout=lay.Wout.weight, bout=lay.Wout.bias)


@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_mix_rhs_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    H, dk = m["heads"], m["attention_dim"] // m["heads"]
    with torch.no_grad():
        att, (v, prods) = func.multihead_att_layer(T(d["x"]), func.edge_index)
        f = func(torch.tensor(0.0), T(d["x"]))
        ax = func.multiply_attention(T(d["x"]), T(d["attention"], torch.float32),
                                     T(M.layer_values(d["v"], H), torch.float32))
        ax2 = func.multiply_attention(T(d["x"]), att, v)
        ax3 = func.multiply_attention(T(d["x"]), att)
    assert prods is None and func.nfe == 1
    assert att.shape == d["attention"].shape and tuple(v.shape) == (m["B"], m["N"], dk, H)
    e_att = float(np.abs(att.double().cpu().numpy() - d["attention"]).max())
    e_v = rel(v, M.layer_values(d["v"], H))
    e_f = rel(f, d["f"])
    bar = max(RTOL, float(np.abs(d["f_ref32"] - d["f"]).max() / np.abs(d["f"]).max()))
    print("%s: attention err %.3e, v rel err %.3e, f rel err %.3e (bar %.3e)" % (os.path.basename(path), e_att, e_v,
                                                                                e_f, bar))
    assert e_att <= ATT_ATOL
    assert e_v <= PROD_RTOL
    assert e_f <= bar
    want_ax = M.multiply_attention(d["edge_index"], d["attention"], d["v"], d["Wout"], d["bout"])
    assert rel(ax, want_ax) <= RTOL
    assert rel(ax2, want_ax) <= RTOL
    assert torch.equal(ax2, ax3)
    with torch.no_grad():  # repeated evaluations: the same bits
        assert torch.equal(func(torch.tensor(0.0), T(d["x"])), f)


def test_bf16_state_raises():
    d, m = _load(os.path.join(GOLDEN, "mix_sd_n0_h2.npz"))
    func = _make(d, m)
    with torch.no_grad(), pytest.raises(NotImplementedError, match="fp32"):
        func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))


def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e" % (name, err, tol))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_mix_grad_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    scale = max(float(np.abs(d[k]).max()) for k in d.files if k.startswith("g_") and d[k].size)
    _check("x", x.grad, d["g_x"], scale)
    _check("alpha_train", func.alpha_train.grad, d["g_alpha_train"], scale)
    _check("beta_train", func.beta_train.grad, d["g_beta_train"], scale)
    for n, p in _params(lay).items():
        _check(n, p.grad, d["g_" + n], scale)
    if m["attention_type"] == "exp_kernel":
        _check("output_var", lay.output_var.grad, d["g_output_var"], scale)
        _check("lengthscale", lay.lengthscale.grad, d["g_lengthscale"], scale)


def test_layer_values_are_differentiable():
    """The layer's second output under autograd: d <g, V(x)> = (g Wv, g^T x, sum g)."""
    d, m = _load(os.path.join(GOLDEN, "mixgrad_sd_n1_h2.npz"))
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    _, (v, _) = lay(x, func.edge_index)
    g = np.random.default_rng(2).standard_normal(d["v"].shape).astype(np.float32)
    (v * T(M.layer_values(g, m["heads"]), torch.float32)).sum().backward()
    gd, xd, Wd = g.astype(np.float64), d["x"].astype(np.float64), d["Wv"].astype(np.float64)
    assert rel(x.grad, gd @ Wd) <= RTOL
    assert rel(lay.V.weight.grad, np.einsum('bna,bnc->ac', gd, xd)) <= RTOL
    assert rel(lay.V.bias.grad, gd.sum(axis=(0, 1))) <= RTOL


def test_mix_features_off_leaves_v_and_wout_without_gradient():
    d, m = _load(os.path.join(GOLDEN, "mixgrad_sd_n1_h2.npz"))
    func = _make(d, m, mix=False)
    lay = func.multihead_att_layer
    assert not lay.mix
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    want = O.transformer_rhs(d["edge_index"], d["x"], d["x0"], d["Wq"], d["bq"], d["Wk"], d["bk"], m["heads"],
                             m["attention_norm_idx"], float(d["alpha_train"]), float(d["beta_train"]),
                             add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"])
    assert rel(f, want) <= RTOL
    (f * T(d["gout"])).sum().backward()
    for p in (lay.V.weight, lay.V.bias, lay.Wout.weight, lay.Wout.bias):
        assert p.grad is None or not bool(p.grad.any())
    assert lay.Q.weight.grad is not None and bool(lay.Q.weight.grad.any())


# mix_pe_n1_h2_dk64 (C = 128, dk = 64: the split-bf16 output product under the stage route) takes the
# rk4 part only: with its N(0, 0.3^2) Wout over 64 columns and alpha = 0.8 the system expands (the fp64
# dopri5 solve takes 108 steps and grows 40-fold over [0, 1]), so the accepted-step count of an fp32 run
# is not comparable with the fp64 one; the other fixtures' solves take 2-3 steps.
@pytest.mark.parametrize("name,adaptive", [("mix_sd_n0_h2", True), ("mix_pe_n1_h2_dk64", False),
                                           ("mix_sp_n1_h2", True), ("mix_pearson_n1_h4", True)])
def test_solves_against_the_restatement(name, adaptive):
    """A 3-step rk4 (the stage route; eager, then captured step graphs replayed) and a dopri5
    solve on a fixture graph; then Wout changed in place: the cached operands follow."""
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    x = d["x"]
    f = lambda t, y: M.fixture_rhs(d, y)[0]  # noqa: E731
    func = _make(d, m, max_nfe=10 ** 6)
    t3 = torch.tensor([0.0, 0.75], device=DEV)
    outs = []
    with torch.no_grad():
        for graph in (False, True, True):
            outs.append(gnpde.odeint(func, T(x), t3, method='rk4',
                                     options={'step_size': 0.25, 'gnpde_graph': graph})[-1])
    torch.cuda.synchronize()
    assert rel(outs[0], O.odeint_fixed(f, x, 0.0, 0.75, 'rk4', 0.25)) <= RTOL
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])
    if adaptive:
        with torch.no_grad():
            z = gnpde.odeint(func, T(x), torch.tensor([0.0, 1.0], device=DEV), rtol=1e-3, atol=1e-4,
                             method='dopri5')[-1]
        n_got = gi.odeint.last_n_steps
        want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
        assert n_got == n_want
        assert rel(z, want[-1] if np.ndim(want) == x.ndim + 1 else want) <= RTOL
    # Wout and its bias edited in place between two solves: the result moves with them
    with torch.no_grad():
        func.multihead_att_layer.Wout.weight.mul_(0.5)
        func.multihead_att_layer.Wout.bias.add_(0.25)
        z2 = gnpde.odeint(func, T(x), t3, method='rk4', options={'step_size': 0.25, 'gnpde_graph': True})[-1]
    d2 = dict((k, d[k]) for k in d.files)
    d2["Wout"], d2["bout"] = d["Wout"] * np.float32(0.5), d["bout"] + np.float32(0.25)
    f2 = lambda t, y: M.fixture_rhs(d2, y)[0]  # noqa: E731
    assert not torch.equal(z2, outs[0])
    assert rel(z2, O.odeint_fixed(f2, x, 0.0, 0.75, 'rk4', 0.25)) <= RTOL
