"""GPU: the beltrami exp_kernel attention (opt['beltrami'], attention_type 'exp_kernel',
opt['gnpde_beltrami_kernel']) against the fixtures of tests/golden/beltrami/ (the reference
layer's own Qx / Kx / Qp / Kp modules, utils.softmax / utils.squareplus, multiply_attention
and float64 autograd; the slice and the score from the formula) and the float64 oracle
(tests/beltrami_oracle.py).

Bars: the project's forward bar 1e-5 (attention absolute, as tests/test_gpu_squareplus.py
measures it, and f relative, RTOL of test_gpu_parity.py) on every fixture and through every
block; gradients under the rule of tests/test_gpu_grad_golden.py (1e-4), the four scalars
checked each on its own; a bf16 state within the project's 2e-2 of the float64 fixture.  The
new kernel alone (gnpde_score_grad_split_f32) against float64 at 1e-5 relative, both sides,
with a 300-edge row and an empty row, and bit-identical across two runs.  Every test prints
its measured figures (pytest -s)."""
import json
import os

import numpy as np
import pytest
import torch

import beltrami_oracle as BO
import gnpde
import gnpde_oracle as O
from conftest import GOLDEN as _GOLDEN
from gnpde import ops
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, rel

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(_GOLDEN, "beltrami")
with open(os.path.join(GOLDEN, "meta.json")) as _fh:
    META = json.load(_fh)
CASES = sorted(META["cases"])
GRAD_CASES = [n for n in CASES if META["cases"][n]["has_grad"]]
ATT_ATOL = 1e-5
GRAD_RTOL = 1e-4
KERNEL_RTOL = 1e-5
BF16_GATE = 2e-2
LINS = (("Qx", "Wqx", "bqx"), ("Kx", "Wkx", "bkx"), ("Qp", "Wqp", "bqp"), ("Kp", "Wkp", "bkp"))


def _load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def _opt(m, **kw):
    sp = dict(square_plus=True, gnpde_square_plus=True) if m["square_plus"] else {}
    opt = dict(OPT, hidden_dim=m["C"], feat_hidden_dim=m["F"], pos_enc_hidden_dim=m["P"], heads=m["heads"],
               attention_dim=m["attention_dim"], attention_norm_idx=m["attention_norm_idx"],
               attention_type='exp_kernel', beltrami=True, gnpde_beltrami_kernel=True, add_source=m["add_source"],
               no_alpha_sigmoid=m["no_alpha_sigmoid"], function='transformer', **sp)
    opt.update(kw)
    return opt


def _set_layer(lay, d, m):
    with torch.no_grad():
        for lin, w, b in LINS:
            getattr(lay, lin).weight.copy_(T(d[w]))
            getattr(lay, lin).bias.copy_(T(d[b]))
        for s in BO.SNAMES:
            getattr(lay, s).fill_(m[s])


def _make(d, m, **kw):
    C = m["C"]
    func = gnpde.ODEFuncTransformerAtt(C, C, _opt(m, **kw), DEV).to(DEV)
    with torch.no_grad():
        func.alpha_train.fill_(float(d["alpha_train"]))
        func.beta_train.fill_(float(d["beta_train"]))
    _set_layer(func.multihead_att_layer, d, m)
    func.edge_index = T(d["edge_index"])
    func.x0 = T(d["x0"])
    return func


# ---------------------------------------------------------------- forward
@pytest.mark.parametrize("name", CASES)
def test_rhs_golden(name):
    d, m = _load(name)
    func = _make(d, m)
    lay = func.multihead_att_layer
    with torch.no_grad():
        att, values = lay(T(d["x"]), func.edge_index)
        f = func(torch.tensor(0.0), T(d["x"]))
        ax = func.multiply_attention(T(d["x"]), att)
    assert values == (None, None) and att.shape == d["attention"].shape and func.nfe == 1
    e_att = float(np.abs(att.double().cpu().numpy() - d["attention"]).max())
    e_f = rel(f, d["f"])
    print("%s: attention err %.3e (bar %.0e), f rel err %.3e (bar %.0e)" % (name, e_att, ATT_ATOL, e_f, RTOL))
    assert e_att <= ATT_ATOL
    assert e_f <= RTOL
    assert rel(ax, O.aggregate(d["edge_index"], d["attention"].mean(axis=2), d["x"])) <= RTOL
    # the exp_kernel passes over the folded projection: heads h, dk' = 2 dk, p0 = ovx ovp, p1 = 1
    ns = lay.node_scores(func.graph_for(T(d["x"])), T(d["x"]))
    assert (ns.mode, ns.heads, ns.dk) == (ops._lib.SCORE_EXP_KERNEL, m["heads"], 2 * m["attention_dim"] // m["heads"])
    assert ns.p1 == 1.0 and abs(ns.p0 - m["output_var_x"] * m["output_var_p"]) <= 1e-6 * ns.p0
    _, kw = BO.fixture_args(d)
    q, k = BO.folded(d["x"], kw["W"], m["heads"], m["F"], m["P"], kw["lsx"], kw["lsp"])
    R = m["B"] * m["N"]
    assert rel(ns.q, q.reshape(R, -1)) <= RTOL and rel(ns.k, k.reshape(R, -1)) <= RTOL


def _block(block, d, m, **kw):
    """A block over the fixture's graph (self loops added by the data object), its layer set
    to the fixture's parameters -> (block, data, the oracle's edge list and weights)."""
    function = 'transformer' if block == 'constant' else 'laplacian'
    opt = _opt(m, block=block, function=function, max_nfe=10 ** 6, att_samp_pct=0.6, **kw)
    blk = gnpde.set_block(opt)(gnpde.set_function(opt), [], opt, DEV, t=torch.tensor([0, 1.0])).to(DEV)
    lay = blk.odefunc.multihead_att_layer if block == 'constant' else blk.multihead_att_layer
    assert lay.beltrami_kernel
    _set_layer(lay, d, m)
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.5)
    data = gnpde.GraphData()
    data.new_graph(T(d["edge_index"]), m["N"])
    eo, wo = _prep_oracle(d["edge_index"], m["N"])
    return blk, lay, data, eo, wo


def _oracle_attention(d, eo, x=None, **over):
    _, kw = BO.fixture_args(d, **over)
    a = {k: kw[k] for k in ("W", "heads", "F", "P", "ovx", "lsx", "ovp", "lsp", "norm_idx", "square_plus")}
    return BO.attention(d["x"] if x is None else x, eo, **a)


@pytest.mark.parametrize("block", ["attention", "mixed", "hard_attention", "constant"])
@pytest.mark.parametrize("name", ["team_n0", "team_n1"])
def test_blocks(name, block):
    d, m = _load(name)
    x = d["x"]
    blk, lay, data, eo, wo = _block(block, d, m, method='rk4', step_size=0.25)
    blk.eval()
    with torch.no_grad():
        if block == 'mixed':
            blk.gamma.fill_(-0.4)
        z = blk(T(x), data)
    if block == 'constant':
        _, kw = BO.fixture_args(d)
        kw.update(alpha_train=0.5, beta_train=0.0)
        f = lambda t, y: BO.rhs(eo, y, None, **kw)[0]  # noqa: E731
    else:
        attn = _oracle_attention(d, eo)
        with torch.no_grad():
            att_gpu = blk.get_attention_weights(T(x)).double().cpu().numpy()
        e_att = float(np.abs(att_gpu - attn).max())
        print("%s %s: attention err %.3e" % (name, block, e_att))
        assert e_att <= ATT_ATOL
        # what the oracle's Laplacian takes per block: [B,E,h] (it takes the head mean), the
        # mixed weights, the head mean
        w = {'attention': attn, 'mixed': O.mixed_attention(attn, wo, -0.4),
             'hard_attention': attn.mean(axis=2)}[block]
        f = lambda t, y: O.laplacian_rhs(eo, y, None, 0.5, 0.0, block=block, attention_weights=w)  # noqa: E731
    err = rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25))
    print("%s %s: z rel err %.3e" % (name, block, err))
    assert err <= RTOL


def test_hard_attention_training_runs():
    d, m = _load("team_n1")
    blk, lay, data, eo, wo = _block('hard_attention', d, m, method='rk4', step_size=0.5)
    blk.train()
    xt = T(d["x"]).requires_grad_(True)
    z = blk(xt, data)
    assert torch.isfinite(z).all() and int(blk.retained) < eo.shape[2]
    z.sum().backward()
    assert xt.grad is not None and torch.isfinite(xt.grad).all()


def test_rk4_solve_follows_parameter_versions():
    """8 rk4 steps in the constant block (fused stages; the second call replays the captured
    step graphs) against the oracle's rk4; after an in-place change of lengthscale_p the
    folded operand and the captured graphs are rebuilt: another result, again the oracle's."""
    d, m = _load("team_n1")
    x = d["x"]
    blk, lay, data, eo, wo = _block('constant', d, m, method='rk4', step_size=0.125)
    blk.eval()
    _, kw = BO.fixture_args(d)
    kw.update(alpha_train=0.5, beta_train=0.0)

    def want(**over):
        a = dict(kw, **over)
        return O.odeint_fixed(lambda t, y: BO.rhs(eo, y, None, **a)[0], x, 0.0, 1.0, 'rk4', 0.125)

    with torch.no_grad():
        z1 = blk(T(x), data)
        z2 = blk(T(x), data)
    torch.cuda.synchronize()
    w1 = want()
    print("rk4 x 8: rel err %.3e" % rel(z1, w1))
    assert rel(z1, w1) <= RTOL and torch.equal(z1, z2)
    with torch.no_grad():
        lay.lengthscale_p.mul_(0.5)
        z3 = blk(T(x), data)
        z4 = blk(T(x), data)
    torch.cuda.synchronize()
    w3 = want(lsp=0.5 * m["lengthscale_p"])
    moved = float(np.abs(w3 - w1).max() / np.abs(w1).max())
    print("after lengthscale_p *= 0.5: rel err %.3e, the oracle moved by %.3e" % (rel(z3, w3), moved))
    assert moved > 100 * RTOL
    assert rel(z3, w3) <= RTOL and torch.equal(z3, z4)
    assert rel(z3, w1) > 10 * RTOL
    # the amplitude is a host scalar of the launches: it follows too
    with torch.no_grad():
        lay.output_var_x.mul_(0.5)
        z5 = blk(T(x), data)
    assert rel(z5, want(lsp=0.5 * m["lengthscale_p"], ovx=0.5 * m["output_var_x"])) <= RTOL


def test_bf16_state():
    d, m = _load("wide")
    func = _make(d, m)
    with torch.no_grad():
        fb = func(torch.tensor(0.0), T(d["x"]).to(torch.bfloat16))
    assert fb.dtype == torch.bfloat16
    scale = float(np.abs(d["f"]).max())
    err = float(np.abs(fb.double().cpu().numpy() - d["f"]).max())
    print("bf16: max err %.3e of scale %.3e (gate %.0e)" % (err, scale, BF16_GATE))
    assert err <= BF16_GATE * scale


# ---------------------------------------------------------------- gradients
def _check(name, got, want, scale):
    got = np.zeros_like(want) if got is None else got.detach().double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    tol = max(GRAD_RTOL * (np.abs(want).max() if want.size else 0.0), 1e-6 * scale)
    print("%s: max err %.3e, tolerance %.3e (largest reference entry %.3e)" % (name, err, tol, np.abs(want).max()))
    assert err <= tol, "%s: max err %.3e, tolerance %.3e" % (name, err, tol)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_grad_golden(name):
    d, m = _load(name)
    func = _make(d, m)
    lay = func.multihead_att_layer
    x = T(d["x"]).requires_grad_(True)
    f = func(torch.tensor(0.0), x)
    assert rel(f, d["f"]) <= RTOL
    (f * T(d["gout"])).sum().backward()
    got = dict(x=x.grad, alpha_train=func.alpha_train.grad, beta_train=func.beta_train.grad)
    for lin, w, b in LINS:
        got[w], got[b] = getattr(lay, lin).weight.grad, getattr(lay, lin).bias.grad
    scale = max(float(np.abs(d["g_" + k]).max()) for k in list(got) + list(BO.SNAMES))
    for k, v in got.items():
        _check(name + " " + k, v, d["g_" + k], scale)
    for s in BO.SNAMES:  # each scalar on its own
        g = getattr(lay, s).grad
        assert g is not None and tuple(g.shape) == (1,)
        _check(name + " " + s, g, d["g_" + s], scale)
    for dead in (lay.Vx, lay.Vp, lay.Wout):
        assert dead.weight.grad is None and dead.bias.grad is None


# ---------------------------------------------------------------- the new kernel alone
KN, KE = 64, 700


def _kernel_graph():
    """64 nodes, 700 edges: node 5 is the source of 300 edges (a 300-edge CSR row), node 7 the
    destination of 300 others (a 300-edge CSC row), node 63 has no edge (an empty row on
    both sides)."""
    rng = np.random.default_rng(77)
    ei = rng.integers(0, KN - 1, size=(1, 2, KE))
    ei[0, 0, :300] = 5
    ei[0, 1, 300:600] = 7
    return ei[:, :, rng.permutation(KE)]


@pytest.mark.parametrize("H,dk,dks", [(2, 8, 4), (1, 12, 6), (8, 32, 16), (3, 10, 3)])
def test_score_grad_split_kernel(H, dk, dks):
    ei = _kernel_graph()
    g = ops.GraphCSR(T(ei), KN)
    rng = np.random.default_rng(1000 * H + dk)
    q, k = (rng.standard_normal((2, KN, H * dk)) * (1.5 / np.sqrt(dk))).astype(np.float32)
    # g_s > 0: the three sums then carry no cancellation, so 1e-5 relative measures the kernel's
    # per-edge terms and not the conditioning of a sum of mixed signs (the rows keep both signs
    # through own - oth)
    gs = (np.abs(rng.standard_normal((KE, H))) + 0.1).astype(np.float32)
    p0 = float(np.float32(2.4))
    want = BO.score_grad_split(ei[0], q, k, gs, H, dk, dks, p0)
    ns = ops.NodeScores(ops._lib.SCORE_EXP_KERNEL, H, dk, q=T(q), k=T(k), p0=p0, p1=1.0)
    tgs = T(gs).view(1, KE, H)
    for side, grouped in ((0, g.csr), (1, g.csc)):
        rows = np.diff(grouped.rowptr.cpu().numpy())
        assert rows.max() >= 300 and rows[KN - 1] == 0
        got = ops.score_grad_split(grouped, side, ns, tgs, dks, with_params=True)
        assert tuple(got[0].shape) == (KN, H * dk)
        err = rel(got[0], want[side])
        print("score_grad_split H=%d dk=%d split=%d side=%d: rows rel err %.3e" % (H, dk, dks, side, err))
        assert err <= KERNEL_RTOL
        assert not got[0][KN - 1].any()                      # the empty row: exact zeros
        for i, nm in enumerate(("S0", "S1", "S2")):
            e = abs(float(got[1 + i]) - want[2 + i]) / abs(want[2 + i])
            print("   %s: %.6e (float64 %.6e), rel err %.3e" % (nm, float(got[1 + i]), want[2 + i], e))
            assert e <= KERNEL_RTOL
        again = ops.score_grad_split(grouped, side, ns, tgs, dks, with_params=True)
        assert all(torch.equal(a, b) for a, b in zip(again, got))
        assert torch.equal(ops.score_grad_split(grouped, side, ns, tgs, dks), got[0])
    # the split is honoured: the whole-head sum is exp_kernel's own lengthscale term
    _, gov, gls = ops.score_grad(g.csr, 0, ns, tgs, with_params=True)
    _, S0, S1, S2 = ops.score_grad_split(g.csr, 0, ns, tgs, dks, with_params=True)
    assert abs(float(S0 - gov)) <= KERNEL_RTOL * abs(float(gov))
    assert abs(float(S1 + S2 - gls)) <= KERNEL_RTOL * max(abs(float(gls)), abs(float(S1)), abs(float(S2)))


def test_score_grad_split_refuses_bad_arguments():
    ei = _kernel_graph()
    g = ops.GraphCSR(T(ei), KN)
    q = torch.zeros(KN, 16, device=DEV)
    ns = ops.NodeScores(ops._lib.SCORE_EXP_KERNEL, 2, 8, q=q, k=q, p0=1.0, p1=1.0)
    gs = torch.zeros(1, KE, 2, device=DEV)
    with pytest.raises(ValueError, match="dk_split"):
        ops.score_grad_split(g.csr, 0, ns, gs, 9)
    with pytest.raises(ValueError, match="exp_kernel"):
        ops.score_grad_split(g.csr, 0, ops.NodeScores(ops._lib.SCORE_DOT, 2, 8, q=q, k=q), gs, 4)
    with pytest.raises(ValueError, match="nnz"):
        ops.score_grad_split(g.csr, 0, ns, gs[:, :10], 4)
    wide = torch.zeros(KN, 1025, device=DEV)
    with pytest.raises(ops._lib.GnpdeError, match="attention_dim"):
        ops.score_grad_split(g.csr, 0, ops.NodeScores(ops._lib.SCORE_EXP_KERNEL, 1, 1025, q=wide, k=wide),
                             torch.zeros(1, KE, 1, device=DEV), 4)
