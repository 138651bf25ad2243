"""GPU: the squareplus attention normalisation (opt['square_plus'] + opt['gnpde_square_plus'])
against the fixtures of tests/golden/squareplus/ (the reference's own prods, utils.squareplus
and multiply_attention in float64) and the oracle (oracle/gnpde_oracle.py, square_plus=True).

Bars: those of test_gpu_gat.py — attention <= 2e-5 absolute, f <= 1e-5 relative (RTOL of
test_gpu_parity.py) on every forward fixture, the wide-range case (node scores of std 50,
where the literal fp32 formula carries 3.9e-4) and B = 3 included; gradients under the rule
of test_gpu_grad_golden.py (1e-4); a bf16 state within the project's 2e-2 gate of fp32.  The
fused K1 (gnpde_attn_sp_rhs_f32) equals the weights pass + the plain K1 bit for bit."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import gnpde.integrator as gi
import gnpde_oracle as O
from conftest import GOLDEN as _GOLDEN
from gnpde import ops
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, _set_qk, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "squareplus")
ATT_ATOL = 2e-5
GRAD_RTOL = 1e-4
BF16_GATE = 2e-2
FWD = sorted(glob.glob(os.path.join(GOLDEN, "sp_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "spgrad_*.npz")))
SP = dict(square_plus=True, gnpde_square_plus=True)


def _load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, **kw):
    return dict(OPT, hidden_dim=m["C"], heads=m["heads"], attention_dim=m["attention_dim"],
                attention_norm_idx=m["attention_norm_idx"], attention_type=m["attention_type"],
                add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"], function='transformer',
                attention_score_mode=m["score_mode"], **dict(SP, **kw))


def _make(d, m, **kw):
    C = m["C"]
    func = gnpde.ODEFuncTransformerAtt(C, C, _opt(m, **kw), DEV).to(DEV)
    lay = func.multihead_att_layer
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
        lay.Q.weight.copy_(T(d["Wq"]))
        lay.Q.bias.copy_(T(d["bq"]))
        lay.K.weight.copy_(T(d["Wk"]))
        lay.K.bias.copy_(T(d["bk"]))
        if m["attention_type"] == "exp_kernel":
            lay.output_var.fill_(m["output_var"])
            lay.lengthscale.fill_(m["lengthscale"])
    func.edge_index = T(d["edge_index"])
    func.x0 = T(d["x0"])
    return func


def _okw(m):
    kw = dict(attention_type=m["attention_type"], score_mode=m["score_mode"], square_plus=True)
    if m["attention_type"] == "exp_kernel":
        kw.update(output_var=m["output_var"], lengthscale=m["lengthscale"])
    return kw


def _ns(d, m, g, x=None):
    kw = {}
    if m["attention_type"] == "exp_kernel":
        kw = dict(output_var=m["output_var"], lengthscale=m["lengthscale"])
    return ops.node_scores(g, T(d["x"]) if x is None else x, T(d["Wq"]), T(d["bq"]), T(d["Wk"]), T(d["bk"]),
                           m["heads"], m["attention_type"], m["score_mode"], **kw)


# ---------------------------------------------------------------- parity
@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_squareplus_rhs_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    with torch.no_grad():
        att, _ = func.multihead_att_layer(T(d["x"]), func.edge_index)
        f = func(torch.tensor(0.0), T(d["x"]))
        ax = func.multiply_attention(T(d["x"]), att)
    assert att.shape == d["attention"].shape and func.nfe == 1
    e_att = float(np.abs(att.double().cpu().numpy() - d["attention"]).max())
    e_f = rel(f, d["f"])
    print("%s: attention err %.3e, f rel err %.3e" % (os.path.basename(path), e_att, e_f))
    assert e_att <= ATT_ATOL
    assert e_f <= RTOL
    assert rel(ax, O.aggregate(d["edge_index"], d["attention"].mean(axis=2), d["x"])) <= RTOL


def test_global_max_is_per_batch_element_and_stays_on_the_device():
    d, m = _load(os.path.join(GOLDEN, "sp_sd_n1_h8_b3.npz"))
    g = ops.GraphCSR(T(d["edge_index"]), m["N"])
    ns = _ns(d, m, g)
    sq = ops.score_max(g, ns)
    M = sq.M.cpu().numpy()
    assert M.shape == (3,) and np.abs(M - np.asarray(m["M"])).max() <= 1e-9 * np.abs(m["M"]).max()
    # the arg-max position holds the maximum (reference scores: an out-edge of the arg-max node)
    s = O.attention_scores(d["x"], d["edge_index"], d["Wq"], d["bq"], d["Wk"], d["bk"], m["heads"])
    am = sq.amax.cpu().numpy()
    per = m["E"] * m["heads"]
    for b in range(3):
        assert b * per <= am[b] < (b + 1) * per
        assert abs(s.reshape(-1)[am[b]] - m["M"][b]) <= 1e-9 * abs(m["M"][b])
    for bad in (ops.uniform_scores(2), ops.NodeScores(ops._lib.SCORE_GAT, 2, 4, sp=sq.M, slope=0.2)):
        with pytest.raises(ValueError):
            ops.score_max(g, bad)
    rc = ops._lib.call_rc("gnpde_score_max_f32", None, None, None, None, 1, 4, 0, ops._lib.SCORE_UNIFORM, 2, 4, None,
                          None, None, 1, 1.0, 1.0, None, None, None, None, 0, None)
    assert rc == ops._lib.EUNSUPPORTED


@pytest.mark.parametrize("norm_idx", [0, 1])
def test_per_edge_scores_outside_the_team_geometry(norm_idx):
    """dk = 6 (no 16-byte slices): the score maximum takes the one-lane-per-edge kernel
    instead of the team kernel the fixtures' shapes (dk 4, 8, 16) run; B = 2."""
    B, N, E, C, h, att = 2, 50, 260, 16, 2, 12
    rng = np.random.default_rng(31 + norm_idx)
    ei = rng.integers(0, N, size=(B, 2, E))
    x = rng.standard_normal((B, N, C)).astype(np.float32)
    Wq, Wk = [(rng.standard_normal((att, C)) * 0.3).astype(np.float32) for _ in range(2)]
    bq, bk = [(rng.standard_normal(att) * 0.3).astype(np.float32) for _ in range(2)]
    g = ops.GraphCSR(T(ei), N)
    ns = ops.node_scores(g, T(x), T(Wq), T(bq), T(Wk), T(bk), h, 'scaled_dot', 'per_edge')
    sq = ops.score_max(g, ns)
    rl = ops.squareplus_stats(g, ns, sq, norm_idx)
    att_g = ops.squareplus_attention(g, ns, sq, rl, norm_idx)
    want = O.transformer_attention(x, ei, Wq, bq, Wk, bk, h, norm_idx, score_mode='per_edge', square_plus=True)
    assert np.abs(att_g.double().cpu().numpy() - want).max() <= ATT_ATOL
    f = ops.squareplus_rhs(g, ns, norm_idx, T(x), alpha=torch.tensor(0.3, device=DEV))
    assert rel(f, O.transformer_rhs(ei, x, None, Wq, bq, Wk, bk, h, norm_idx, 0.3, 0.0, score_mode='per_edge',
                                    square_plus=True)) <= RTOL


# ---------------------------------------------------------------- fused functor
@pytest.mark.parametrize("name", ["sp_sd_n1_c128", "sp_sd_n1_c162"])
def test_fused_equals_unfused_bitwise(name):
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    g = ops.GraphCSR(T(d["edge_index"]), m["N"])
    x = T(d["x"])
    ns = _ns(d, m, g)
    a = torch.tensor(0.3, device=DEV)
    fused = ops.squareplus_rhs(g, ns, 1, x, alpha=a, fuse=True)
    unfused = ops.squareplus_rhs(g, ns, 1, x, alpha=a, fuse=False)
    torch.cuda.synchronize()
    assert torch.equal(fused, unfused)
    for _ in range(2):
        assert torch.equal(ops.squareplus_rhs(g, _ns(d, m, g), 1, x, alpha=a, fuse=True), fused)
    # a fused Runge-Kutta stage: the same bits as the stage over the weights pass
    outs = []
    for fuse in (True, False):
        out = torch.empty_like(x)
        ops.squareplus_rhs(g, ns, 1, x, alpha=a, fuse=fuse, stage=ops.Stage(outs=[(out, x, 1.0, 0.5, [])]))
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    want = O.transformer_rhs(d["edge_index"], d["x"], None, d["Wq"], d["bq"], d["Wk"], d["bk"], m["heads"], 1, 0.3,
                             0.0, **_okw(m))
    assert rel(fused, want) <= RTOL


# ---------------------------------------------------------------- uniform case
def test_uniform_case_uses_the_cached_weights():
    d, m = _load(os.path.join(GOLDEN, "sp_sd_n0_h2.npz"))
    func = _make(d, m)
    lay = func.multihead_att_layer
    assert lay.is_uniform(0) and lay.square_plus
    with torch.no_grad():
        f = func(torch.tensor(0.0), T(d["x"]))
        att, _ = lay(T(d["x"]), func.edge_index)
    assert lay._uniform is not None and lay._sp_bufs is None  # no squareplus pass ran
    g = func.graph_for(T(d["x"]))
    assert lay.uniform_weights(g) is lay._uniform[4]
    deg = np.bincount(d["edge_index"][0, 0], minlength=m["N"])
    assert np.abs(att.double().cpu().numpy()[0] - (1.0 / deg[d["edge_index"][0, 0]])[:, None]).max() <= 1e-7
    assert rel(f, d["f"]) <= RTOL
    assert func.supports_feature_padding()


# ---------------------------------------------------------------- hub groups
def _hub_graph(seed):
    """~4000 nodes, 24,000 edges: one source and one destination of 100 edges (two chunk
    items of the 64-edge statistics plan) and one source and one destination of 1,100
    edges (18 chunks: beyond one wavefront pass of the statistics kernel, merged by the
    hub kernel; K1 splits the rows too)."""
    N = 4000
    rng = np.random.default_rng(seed)
    ei = rng.integers(0, N, size=(1, 2, 24000))
    ei[0, 0, :1100] = 3
    ei[0, 1, 1100:2200] = 5
    ei[0, 0, 2200:2300] = 9
    ei[0, 1, 2300:2400] = 11
    return N, ei


@pytest.mark.parametrize("score_mode", ["reference", "per_edge"])
@pytest.mark.parametrize("norm_idx", [0, 1])
def test_hub_groups(norm_idx, score_mode):
    N, ei = _hub_graph(17 + norm_idx)
    C, h, att = 16, 2, 16
    rng = np.random.default_rng(5)
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    scale = 0.02 if score_mode == "reference" else 0.3
    Wq, Wk = [(rng.standard_normal((att, C)) * scale).astype(np.float32) for _ in range(2)]
    bq, bk = [(rng.standard_normal(att) * scale).astype(np.float32) for _ in range(2)]
    g = ops.GraphCSR(T(ei), N)
    ns = ops.node_scores(g, T(x), T(Wq), T(bq), T(Wk), T(bk), h, 'scaled_dot', score_mode)
    sq = ops.score_max(g, ns)
    rl = ops.squareplus_stats(g, ns, sq, norm_idx)
    w = ops.squareplus_weights(g, ns, sq, rl, norm_idx)
    att_g = ops.squareplus_attention(g, ns, sq, rl, norm_idx)
    torch.cuda.synchronize()
    grouped = g.csr if norm_idx == 0 else g.csc
    assert grouped.stats_plan.n_heavy >= 2 and grouped.stats_plan.n_slots >= 20
    s = O.attention_scores(x, ei, Wq, bq, Wk, bk, h, 'scaled_dot', score_mode)
    assert abs(float(sq.M[0]) - s.max()) <= 1e-5 * max(1.0, abs(s.max()))
    want = O.squareplus(s, ei[:, norm_idx, :], N)
    # statistics: L = sum of p over the group.  p is an fp32 value of relative error ~1e-7 on a
    # score whose own fp32 error (~1e-6 absolute for |s| ~ 10) moves p by at most that much
    # relatively (|dp/dt| <= p / 2), and the sum is taken in fp64: 1e-5 relative bounds it with room
    t = s[0] - s.max()
    p = 2.0 / (np.sqrt(t * t + 4.0) - t)
    L = np.zeros((N, h))
    np.add.at(L, ei[0, norm_idx], p)
    live = np.bincount(ei[0, norm_idx], minlength=N) > 0
    got_L = 1.0 / rl.double().cpu().numpy() - 1e-16
    assert np.abs(got_L[live] / L[live] - 1.0).max() <= 1e-5
    assert np.abs(att_g.double().cpu().numpy() - want).max() <= ATT_ATOL
    wcoo = np.empty(ei.shape[2])
    wcoo[g.csr.perm.cpu().numpy()] = w.double().cpu().numpy()
    assert np.abs(wcoo - want[0].mean(axis=1)).max() <= ATT_ATOL
    # the whole RHS over the hub rows of K1, fused (reference scores, norm_idx 1) or not
    al = torch.tensor(0.3, device=DEV)
    f = ops.squareplus_rhs(g, ns, norm_idx, T(x), alpha=al)
    f2 = ops.squareplus_rhs(g, ns, norm_idx, T(x), alpha=al, fuse=False)
    assert torch.equal(f, f2)
    want_f = O.transformer_rhs(ei, x, None, Wq, bq, Wk, bk, h, norm_idx, 0.3, 0.0, score_mode=score_mode,
                               square_plus=True)
    assert rel(f, want_f) <= RTOL
    assert g.csr.plan.n_heavy >= 1


# ---------------------------------------------------------------- gradients
def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e" % (name, err, tol))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_squareplus_grad_golden(path):
    d, m = _load(path)
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    got = dict(x=x.grad, alpha_train=func.alpha_train.grad, beta_train=func.beta_train.grad, Wq=lay.Q.weight.grad,
               bq=lay.Q.bias.grad, Wk=lay.K.weight.grad, bk=lay.K.bias.grad)
    if m["attention_type"] == "exp_kernel":
        got.update(output_var=lay.output_var.grad, lengthscale=lay.lengthscale.grad)
    scale = max(float(np.abs(d["g_" + k]).max()) for k in got)
    for k, v in got.items():
        _check(k, v, d["g_" + k], scale)


def test_backward_without_the_max_term_misses_the_fixture():
    """The max term is part of the derivative: dropping it (the softmax-style group term
    alone) moves dL/ds by far more than the gradient bar."""
    d, m = _load(os.path.join(GOLDEN, "spgrad_pe_n1.npz"))
    g = ops.GraphCSR(T(d["edge_index"]), m["N"])
    ns = _ns(d, m, g)
    sq = ops.score_max(g, ns)
    rl = ops.squareplus_stats(g, ns, sq, 1)
    att = ops.squareplus_attention(g, ns, sq, rl, 1)
    gen = torch.Generator(device='cpu').manual_seed(1)
    ga = torch.randn(att.shape, generator=gen).to(DEV)
    gs = ops.squareplus_backward(g.csc, att, ga, rl, sq.amax)
    # fp64 restatement of the issue's formula
    a, gg, r = att.double().cpu().numpy(), ga.double().cpu().numpy(), rl.double().cpu().numpy()
    ei = d["edge_index"]
    want = np.empty_like(a)
    for b in range(m["B"]):
        grp = ei[b, 1] + b * m["N"]
        dsum = np.zeros((m["B"] * m["N"], m["heads"]))
        np.add.at(dsum, grp, a[b] * gg[b])
        p = a[b] / r[grp]
        want[b] = a[b] / (p + 1.0 / p) * (gg[b] - dsum[grp])
    nomax = want.copy()
    am = sq.amax.cpu().numpy()
    for b in range(m["B"]):
        want.reshape(-1)[am[b]] -= want[b].sum()
    got = gs.double().cpu().numpy()
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    assert np.abs(got - nomax).max() > 1e-2 * np.abs(want).max()


# ---------------------------------------------------------------- stage fusion and capture
def _const_block(m, d, **kw):
    opt = _opt(m, max_nfe=10 ** 6, **kw)
    blk = gnpde.ConstantODEblock(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    lay = blk.odefunc.multihead_att_layer
    with torch.no_grad():
        lay.Q.weight.copy_(T(d["Wq"]))
        lay.Q.bias.copy_(T(d["bq"]))
        lay.K.weight.copy_(T(d["Wk"]))
        lay.K.bias.copy_(T(d["bk"]))
        blk.odefunc.alpha_train.fill_(0.5)
    data = gnpde.GraphData()
    data.new_graph(T(d["edge_index"]), m["N"])
    return blk, data


@pytest.mark.parametrize("name", ["sp_sd_n1_h2", "sp_pe_n0_h2"])
def test_stage_fusion_in_constant_block(name):
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    ei, x, N = d["edge_index"], d["x"], m["N"]
    eo, _ = _prep_oracle(ei, N)
    ni = m["attention_norm_idx"]
    f = lambda t, y: O.transformer_rhs(eo, y, None, d["Wq"], d["bq"], d["Wk"], d["bk"], m["heads"], ni, 0.5, 0.0,  # noqa
                                       **_okw(m))
    blk, data = _const_block(m, d, method='rk4', step_size=0.25)
    with torch.no_grad():
        z1 = blk(T(x), data)
        z2 = blk(T(x), data)  # the captured step graphs
    torch.cuda.synchronize()
    assert rel(z1, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL
    assert torch.equal(z1, z2)
    # replayed step graphs against the eager loop, bit for bit
    outs = []
    for graph in (False, True):
        func = _make(d, m, max_nfe=10 ** 6)
        func.edge_index = T(eo)
        with torch.no_grad():
            z = gnpde.odeint(func, T(x), torch.tensor([0.0, 0.4, 1.0], device=DEV), method='rk4',
                             options={'step_size': 0.05, 'gnpde_graph': graph})
        torch.cuda.synchronize()
        outs.append((z, func.nfe))
    assert outs[0][1] == outs[1][1] == 80 and torch.equal(outs[0][0], outs[1][0])
    blk, data = _const_block(m, d, method='dopri5')
    blk.rtol, blk.atol = 1e-3, 1e-4
    with torch.no_grad():
        z = blk(T(x), data)
        zb = blk(T(x), data)
    n_got = gi.odeint.last_n_steps
    want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
    assert n_got == n_want
    assert rel(z, want[-1] if np.ndim(want) == x.ndim + 1 else want) <= RTOL
    assert torch.equal(z, zb)


@pytest.mark.parametrize("mode,norm_idx", [("per_edge", 0), ("reference", 1)])
def test_fixed_grid_solve_in_the_node_layout(mode, norm_idx):
    """A large graph's fixed-grid solve runs in the in-degree numbering (ops.NodeLayout,
    replayed step graphs): the squareplus operands follow it (per-node p in the internal
    numbering, stored scores in COO order, which the renumbering keeps; one maximum either
    way).  Bars of tests/test_gpu_layout.py::test_layout_attention_scores: 1e-5 for the
    solve against the user numbering, 1e-6 for one RHS; weights scaled as there."""
    from gnpde import synthetic
    from test_gpu_layout import _solve
    N, E, C, h, att = 60000, 450000, 128, 2, 32
    wscale = 1e-3 if mode == "reference" else 0.1
    ei, _ = synthetic.rw_graph(N, E, seed=32, device=DEV)
    opt = dict(OPT, hidden_dim=C, heads=h, attention_dim=att, attention_norm_idx=norm_idx,
               attention_score_mode=mode, function='transformer', max_nfe=10 ** 6, **SP)
    func = gnpde.ODEFuncTransformerAtt(C, C, opt, DEV).to(DEV).eval()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    with torch.no_grad():
        for lin in (func.multihead_att_layer.Q, func.multihead_att_layer.K):
            lin.weight.copy_(torch.randn(att, C, generator=gen, device=DEV) * wscale)
            lin.bias.copy_(torch.randn(att, generator=gen, device=DEV) * wscale)
        func.alpha_train.fill_(0.3)
    func.edge_index = ei
    x = synthetic.features(1, N, C, seed=8, device=DEV)
    lay = func.node_layout(x)
    assert lay is not None
    ref = _solve(func, x, "rk4", 7, 0.25, "none")
    got = _solve(func, x, "rk4", 7, 0.25, "degree")
    assert float((got - ref).abs().max() / ref.abs().max()) <= 1e-5
    assert torch.equal(_solve(func, x, "rk4", 7, 0.25, "degree"), got)  # the captured steps replay
    with torch.no_grad():
        f_user = func(None, x)
        func._layout = lay
        try:
            f_int = func(None, lay.to_internal(x))
        finally:
            func._layout = None
    assert float((lay.to_user(f_int) - f_user).abs().max() / f_user.abs().max()) <= 1e-6


# ---------------------------------------------------------------- blocks
def test_attention_block_cora_shaped_dopri5_vs_oracle():
    """Cora's best_params shape (block attention, heads 8, attention_dim 128, norm_idx 1,
    add_source, square_plus) on a 300-node graph: dopri5 against the oracle integrated
    with the oracle's squareplus weights."""
    N, E, C, h, att = 300, 1800, 80, 8, 128
    rng = np.random.default_rng(23)
    ei = rng.integers(0, N, size=(1, 2, E))
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    opt = dict(OPT, hidden_dim=C, heads=h, attention_dim=att, block='attention', attention_norm_idx=1,
               add_source=True, method='dopri5', max_nfe=10 ** 6, **SP)
    blk = gnpde.AttODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    Wq, bq, Wk, bk = _set_qk(blk.multihead_att_layer, rng, C, att, scale=0.03)
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.5)
        blk.odefunc.beta_train.fill_(0.25)
    blk.rtol, blk.atol = 1e-3, 1e-4
    data = gnpde.GraphData()
    data.new_graph(T(ei), N)
    blk.set_x0(T(x))
    with torch.no_grad():
        z = blk(T(x), data)
    n_got = gi.odeint.last_n_steps
    eo, wo = _prep_oracle(ei, N)
    attn = O.transformer_attention(x, eo, Wq, bq, Wk, bk, h, 1, square_plus=True)
    assert attn.std() > 0
    with torch.no_grad():
        att_gpu = blk.get_attention_weights(T(x)).double().cpu().numpy()
    assert np.abs(att_gpu - attn).max() <= ATT_ATOL
    f = lambda t, y: O.laplacian_rhs(eo, y, x, 0.5, 0.25, block='attention', attention_weights=attn,  # noqa: E731
                                     add_source=True)
    want, n_want = O.odeint_adaptive(f, x, [0.0, 1.0], 'dopri5', 1e-3, 1e-4)
    assert n_got == n_want
    assert rel(z, want[-1] if np.ndim(want) == x.ndim + 1 else want) <= RTOL


def test_best_params_blocks_run_a_forward():
    """Cora's, Citeseer's, Pubmed's and CoauthorCS's best_params settings (recorded from
    src/best_params.py) with gnpde_square_plus added: the block constructs and integrates
    (time shortened to 1) on a small graph."""
    with open(os.path.join(GOLDEN, "best_params_squareplus.json")) as fh:
        bp = json.load(fh)
    N, E = 300, 1800
    rng = np.random.default_rng(29)
    ei = rng.integers(0, N, size=(1, 2, E))
    data = gnpde.GraphData()
    data.new_graph(T(ei), N)
    for name in ("Cora", "Citeseer", "Pubmed", "CoauthorCS"):
        opt = dict(OPT, **bp[name])
        opt.update(time=1.0, gnpde_square_plus=True)
        C = opt['hidden_dim']
        blk = gnpde.set_block(opt)(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
        _set_qk(blk.multihead_att_layer, rng, C, opt['attention_dim'], scale=0.1)
        x = T(rng.standard_normal((1, N, C)).astype(np.float32))
        blk.set_x0(x)
        with torch.no_grad():
            z = blk(x, data)
            att = blk.get_attention_weights(x)
        assert z.shape == x.shape and torch.isfinite(z).all(), name
        # squareplus, not softmax: every destination / source group sums to 1 and no weight is exp-small
        assert att.shape[-1] == opt['heads'] and float(att.min()) > 0, name


@pytest.mark.parametrize("name", ["sp_sd_n1_c128", "sp_pe_n1_c128_h8"])
def test_bf16_state(name):
    d, m = _load(os.path.join(GOLDEN, name + ".npz"))
    func = _make(d, m)
    with torch.no_grad():
        f32 = func(torch.tensor(0.0), T(d["x"]))
        fb = func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))
    assert fb.dtype == torch.bfloat16
    scale = float(f32.abs().max())
    assert float((fb.float() - f32).abs().max()) <= BF16_GATE * scale


def test_hard_attention_compacted_graph_matches_masked(monkeypatch):
    """HardAttODEblock training forward under squareplus: the retained edges compacted inside
    the plan's items (the default) against the masked full graph (COMPACT_SAMPLED off) — bit
    for bit at C = 128, as the softmax test (test_hard_attention_compacted_graph_bit_equal) —
    and the sampled attention against the oracle's squareplus."""
    import gnpde.base_classes as bc
    N, E, C, h, att = 1200, 9000, 128, 2, 16
    rng = np.random.default_rng(73)
    ei = rng.integers(0, N, size=(1, 2, E))
    ei[0, 0, :400] = 7
    ei[0, 1, 400:800] = 11
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    opt = dict(OPT, hidden_dim=C, heads=h, attention_dim=att, block='hard_attention', attention_norm_idx=1,
               att_samp_pct=0.6, method='rk4', step_size=0.25, attention_score_mode='per_edge', **SP)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N)
    res = []
    for compact in (True, False):
        monkeypatch.setattr(bc, "COMPACT_SAMPLED", compact)
        blk = gnpde.HardAttODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0, 1.0])).to(DEV).train()
        Wq, bq, Wk, bk = _set_qk(blk.multihead_att_layer, np.random.default_rng(3), C, att, scale=0.05)
        with torch.no_grad():
            blk.odefunc.alpha_train.fill_(0.4)
        xt = T(x).requires_grad_(True)
        z = blk(xt, data)
        z.sum().backward()
        res.append((z.detach(), xt.grad, blk.odefunc.nfe, int(blk.retained)))
    (z0, g0, n0, r0), (z1, g1, n1, r1) = res
    assert torch.equal(z0, z1) and torch.equal(g0, g1) and n0 == n1 and r0 == r1 < ei.shape[2] + N
    eo, _ = _prep_oracle(ei, N)
    attn = O.transformer_attention(x, eo, Wq, bq, Wk, bk, h, 1, score_mode='per_edge', square_plus=True)
    with torch.no_grad():
        att_gpu = blk.get_attention_weights(T(x)).double().cpu().numpy()
    assert np.abs(att_gpu - attn).max() <= ATT_ATOL
