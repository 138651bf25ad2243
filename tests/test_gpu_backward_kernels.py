"""The backward kernels one by one (csrc/backward.hip, csrc/score_backward.hip,
gnpde_gat_score_backward_f32, the fp64 reductions of csrc/solver.hip) against the
float64 references of tests/backward_oracle.py, at the widths training runs them
(Cora's heads 8 / attention_dim 128 / C 80, BLEND's C 162, C 128 and 256) and at the
edges of their lane, tile and loop geometry; then the whole-RHS gradients at those
widths against torch float64 autograd.

Bars: the project's forward bar RTOL (1e-5, max over max) for the SDDMM, its gradient
bar GTOL (1e-4, max over max) for the score gradients and the whole-RHS gradients;
the kernels that do fp64 math are held to bars derived from their arithmetic
(backward_oracle.*_bar), the pure selections (gather_head, the GAT LeakyReLU
backward) to exact equality.  Every kernel is also run twice and must give the same
bits.  Each test prints its measured error beside its bar (pytest -s).
tests/test_backward_oracle_host.py checks the references and that these inputs would
expose a dropped edge, swapped heads, a dropped column or a missing a_own term.
"""
import numpy as np
import pytest
import torch

import backward_oracle as BO
import gnpde
from gnpde import _lib, ops
from gnpde.ops import _ptr, _stream
from test_gpu_backward import BIAS_OF, GTOL, OPT, graph, qk_params, relerr, t_attention, t_rhs, t_softmax
from test_gpu_parity import DEV, RTOL, T, rel

pytestmark = pytest.mark.gpu

assert (RTOL, GTOL) == (BO.RTOL, BO.GTOL)   # the host test multiplies the same bars


def report(name, err, bar):
    print("%-58s err %.3e  bar %.3e" % (name, err, bar))


def npy(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def G():
    """(edge list, GraphCSR, {side: (grouped CSR, group id of every COO edge, COO ids in grouped order)})."""
    ei = BO.unit_graph()
    g = ops.GraphCSR(T(ei), BO.UNIT_N)
    sides = {}
    for side, grouped, nodes in ((0, g.csr, BO.SRC_NODES), (1, g.csc, BO.DST_NODES)):
        gidx = BO.groups_of(ei, BO.UNIT_N, side)
        rowptr = npy(grouped.rowptr).astype(np.int64)
        order = npy(grouped.perm)[:grouped.nnz].astype(np.int64)
        assert np.array_equal(np.diff(rowptr), np.bincount(gidx, minlength=g.R))
        assert np.array_equal(np.sort(order), np.arange(g.nnz)) and (np.diff(gidx[order]) >= 0).all()
        for b in range(BO.UNIT_B):   # the constructed groups of 0, 1, 63, 64, 65 and 200 edges
            assert tuple(np.diff(rowptr)[b * BO.UNIT_N + np.asarray(nodes)]) == BO.GROUP_SIZES
        sides[side] = (grouped, gidx, order)
    return ei, g, sides


# ============================================================================ sddmm
@pytest.mark.parametrize("alpha", BO.SDDMM_ALPHA)
@pytest.mark.parametrize("H,C", BO.SDDMM_CASES)
def test_sddmm(G, H, C, alpha):
    ei, g, _ = G
    gf, x = BO.sddmm_inputs(H, C)
    a = None if alpha is None else torch.tensor(BO.ALPHA_VALUE, device=DEV)
    tg, tx = T(gf), T(x)

    def call():
        return ops.sddmm(g, tg, tx, heads=H, alpha=a, alpha_sigmoid=alpha == "sigmoid")

    got = call()
    want = BO.sddmm(ei, gf, x, BO.alpha_scale(alpha), H)
    assert tuple(got.shape) == want.shape
    err = rel(got, want)
    report("sddmm heads=%d C=%d alpha=%s" % (H, C, alpha), err, RTOL)
    assert err <= RTOL
    assert torch.equal(call(), got)


def test_sddmm_refuses_65_heads_and_returns_on_no_edges(G):
    ei, g, _ = G
    gf, x = BO.sddmm_inputs(1, 12)
    with pytest.raises(_lib.GnpdeError, match="heads"):
        ops.sddmm(g, T(gf), T(x), heads=65)
    out = torch.full((8,), 7.0, device=DEV)
    _lib.call("gnpde_sddmm_f32", _ptr(None), _ptr(None), _ptr(None), 0, 12, _ptr(None), 12, _ptr(None), 12, _ptr(None),
              0, 1, _ptr(out), _stream(out.device))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ============================================================================ softmax backward, segment sums
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.SOFTMAX_HEADS)
def test_softmax_backward(G, side, H):
    ei, g, sides = G
    grouped, gidx, _ = sides[side]
    att, gg = BO.softmax_inputs(ei, side, H)
    ta, tg = T(att).view(g.B, g.E, H), T(gg).view(g.B, g.E, H)
    got = ops.softmax_backward(grouped, ta, tg)
    want = BO.softmax_backward(gidx, att, gg)
    ex = BO.exceed(npy(got).reshape(want.shape), want, BO.softmax_backward_bar(want, gg))
    report("softmax_backward side=%d H=%d (|err|/bar, elementwise)" % (side, H), ex, 1.0)
    assert ex <= 1.0
    assert torch.equal(ops.softmax_backward(grouped, ta, tg), got)


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.SEGSUM_HEADS)
def test_segment_sum(G, side, H):
    ei, g, sides = G
    grouped, gidx, _ = sides[side]
    v = BO.segsum_inputs(side, H)
    tv = T(v).view(g.B, g.E, H)
    got = ops.segment_sum(grouped, tv)
    want = BO.segment_sum(gidx, v, g.R)
    empty = np.bincount(gidx, minlength=g.R) == 0
    assert empty.sum() >= BO.UNIT_B                       # the constructed empty groups
    assert (npy(got)[empty] == 0.0).all()                 # exact zeros into a torch.empty output
    ex = BO.exceed(npy(got), want, BO.segment_sum_bar(gidx, v, g.R))
    report("segment_sum side=%d H=%d (|err|/bar, per row)" % (side, H), ex, 1.0)
    assert ex <= 1.0
    assert torch.equal(ops.segment_sum(grouped, tv), got)


# ============================================================================ weighted column sums
@pytest.mark.parametrize("B,N,C,H", BO.WCOLSUM_CASES)
def test_wcolsum(B, N, C, H):
    x, w = BO.wcolsum_inputs(B, N, C, H)
    tx, tw = T(x), T(w).view(B * N, H)
    got = ops.wcolsum(tx, B, N, tw)
    want = BO.wcolsum(x, w)
    assert tuple(got.shape) == want.shape == (B, H, C + 1)
    ex = BO.exceed(npy(got), want, BO.wcolsum_bar(x, w))
    report("wcolsum B=%d N=%d C=%d H=%d (|err|/bar, per output)" % (B, N, C, H), ex, 1.0)
    assert ex <= 1.0
    assert torch.equal(ops.wcolsum(tx, B, N, tw), got)


def test_wcolsum_refuses_a_row_past_the_lds():
    C = BO.WCOLSUM_REFUSED_C
    x = torch.zeros(1, 2, C, device=DEV)
    w = torch.ones(2, 1, dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.GnpdeError, match="C too large"):
        ops.wcolsum(x, 1, 2, w)


# ============================================================================ node-score input gradient
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("B,N,C,H", BO.SIG_CASES)
def test_score_input_grad(B, N, C, H, accumulate):
    gcs, U, deg, gxbar, gx0 = BO.sig_inputs(B, N, C, H)
    tg, tU, td, tb = T(gcs).view(B * N, H), T(U), T(deg).view(-1), T(gxbar)

    def call():
        out = T(gx0).view(B * N, C).clone() if accumulate else None
        res = ops.score_input_grad(tg, tU, td, tb, B, N, C, out=out)
        assert out is None or res is out
        return res

    got = call()
    want = BO.score_input_grad(gcs, U, deg, gxbar, gx0 if accumulate else None)
    ex = BO.exceed(npy(got).reshape(want.shape), want, BO.score_input_grad_bar(want))
    report("score_input_grad B=%d N=%d C=%d H=%d acc=%d (|err|/bar)" % (B, N, C, H, accumulate), ex, 1.0)
    assert ex <= 1.0
    assert torch.equal(call(), got)


# ============================================================================ head gather
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.GATHER_HEADS)
def test_gather_head(G, side, H):
    ei, g, sides = G
    grouped, _, order = sides[side]
    w = BO.gather_inputs(H)
    tw = T(w).view(g.B, g.E, H)
    for scale in (1.0, 1.0 / BO.GATHER_DK ** 0.5):
        for h in range(H):
            got = ops.gather_head(grouped, tw, h, scale)
            assert np.array_equal(npy(got)[:g.nnz], BO.gather_head(order, w, h, scale)), (h, scale)
            assert torch.equal(ops.gather_head(grouped, tw, h, scale), got)
    with pytest.raises(_lib.GnpdeError, match="bad head"):
        ops.gather_head(grouped, tw, H)


# ============================================================================ per-edge score gradient
@pytest.mark.parametrize("mode,H,dk", BO.SCORE_CASES)
def test_score_grad(G, mode, H, dk):
    ei, g, sides = G
    q, k, gs, p0, p1 = BO.score_inputs(mode, H, dk)
    s = BO.score_values(ei, BO.UNIT_N, q, k, mode, H, dk, p0, p1)
    print("score_grad %s H=%d dk=%d: s in [%.3e, %.3e], smallest head norm %.3e"
          % (mode, H, dk, s.min(), s.max(), BO.min_head_norm(q, k, mode, H, dk)))
    want = BO.score_grad(ei, q, k, gs, mode, H, dk, p0, p1)
    ns = ops.NodeScores(BO.MODES[mode], H, dk, q=T(q), k=T(k), p0=p0, p1=p1)
    tgs = T(gs).view(g.B, g.E, H)
    for side in (0, 1):
        grouped = sides[side][0]
        got = ops.score_grad(grouped, side, ns, tgs)
        assert tuple(got.shape) == (g.R, H * dk)
        err = rel(got, want[side])
        report("score_grad %s H=%d dk=%d side=%d" % (mode, H, dk, side), err, GTOL)
        assert err <= GTOL
        assert torch.equal(ops.score_grad(grouped, side, ns, tgs), got)
    if mode == "exp_kernel":
        got, gov, gls = ops.score_grad(sides[0][0], 0, ns, tgs, with_params=True)
        assert rel(got, want[0]) <= GTOL
        for name, gp, wp in (("output_var", gov, want[2]), ("lengthscale", gls, want[3])):
            err = abs(float(gp) - wp) / abs(wp)
            report("score_grad exp_kernel H=%d dk=%d d/d%s" % (H, dk, name), err, GTOL)
            assert err <= GTOL
        again = ops.score_grad(sides[0][0], 0, ns, tgs, with_params=True)
        assert all(torch.equal(a, b) for a, b in zip(again, (got, gov, gls)))


def test_score_grad_refuses_attention_dim_1025(G):
    ei, g, sides = G
    q = torch.zeros(g.R, 1025, device=DEV)
    ns = ops.NodeScores(BO.MODES["scaled_dot"], 1, 1025, q=q, k=q)
    with pytest.raises(_lib.GnpdeError, match="attention_dim"):
        ops.score_grad(sides[0][0], 0, ns, torch.zeros(g.B, g.E, 1, device=DEV))


# ============================================================================ GAT LeakyReLU backward
@pytest.mark.parametrize("H", BO.GAT_HEADS)
def test_gat_score_backward(G, H):
    ei, g, _ = G
    sp, gs = BO.gat_inputs(ei, H)
    ns = ops.NodeScores(_lib.SCORE_GAT, H, 1, sp=T(sp), slope=BO.GAT_SLOPE)
    tgs = T(gs).view(g.B, g.E, H)
    got = ops.gat_score_backward(g, ns, tgs)
    assert np.array_equal(npy(got).reshape(-1, H), BO.gat_score_backward(ei, sp, BO.GAT_SLOPE, gs))
    assert torch.equal(ops.gat_score_backward(g, ns, tgs), got)


def test_gat_score_backward_refuses_9_heads(G):
    ei, g, _ = G
    ns = ops.NodeScores(_lib.SCORE_GAT, 9, 1, sp=torch.zeros(g.R, 18, dtype=torch.float64, device=DEV), slope=0.2)
    with pytest.raises(_lib.GnpdeError, match="gat_score_backward"):
        ops.gat_score_backward(g, ns, torch.zeros(g.B, g.E, 9, device=DEV))


# ============================================================================ fp64 reductions
def exact_sum(v):
    return float(np.sum(np.asarray(v, np.float64).astype(np.longdouble)))


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("n", BO.SUM_NS)
def test_sum_f64(n, accumulate):
    v = BO.sum_inputs(n)
    tv = T(v)

    def call():
        return ops.sum_f64(tv, out=torch.full((), 3.25, dtype=torch.float64, device=DEV), accumulate=accumulate)

    got = call()
    want = exact_sum(v) + (3.25 if accumulate else 0.0)
    # accumulating adds one term, the value already in ``out``, to the sum the bound is about
    err, bar = abs(float(got) - want), BO.sum_bar(np.append(v, 3.25) if accumulate else v)
    report("sum_f64 n=%d acc=%d (absolute)" % (n, accumulate), err, bar)
    assert err <= bar
    assert torch.equal(call(), got)
    if not accumulate:
        assert torch.equal(ops.sum_f64(tv), got)          # a fresh output: the same sum


@pytest.mark.parametrize("nseg,ln", BO.SEGSUMS_CASES)
def test_segment_sums(nseg, ln):
    v = BO.segsums_inputs(nseg, ln)
    tv = T(v)
    outs = []
    for _ in range(2):
        out = torch.full((nseg,), -1.0, dtype=torch.float64, device=DEV)
        ops.segment_sums(tv, out)
        outs.append(out)
    got = npy(outs[0])
    worst = 0.0
    for s in range(nseg):
        err, bar = abs(got[s] - exact_sum(v[s])), BO.sum_bar(v[s])
        worst = max(worst, err / bar if bar > 0 else float(err > 0))
        assert err <= bar, (s, err, bar)
    report("segment_sums nseg=%d len=%d (|err|/bar, worst row)" % (nseg, ln), worst, 1.0)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("with_f1", [False, True])
@pytest.mark.parametrize("n", BO.SQ_NS)
def test_scaled_sq_sums(n, with_f1):
    y0, f0, f1 = BO.sq_inputs(n)
    ty, tf0, tf1 = T(y0), T(f0), (T(f1) if with_f1 else None)
    outs = []
    for _ in range(2):
        out = torch.full((2,), -1.0, dtype=torch.float64, device=DEV)
        ops.scaled_sq_sums(ty, tf0, tf1, BO.SQ_ATOL, BO.SQ_RTOL, out)
        outs.append(out)
    got = npy(outs[0])
    want = BO.scaled_sq_sums(y0, f0, f1 if with_f1 else None, BO.SQ_ATOL, BO.SQ_RTOL)
    pairs = [(got[0], want)] if with_f1 else list(zip(got, want))
    for j, (a, b) in enumerate(pairs):
        err = abs(a - b) / b
        report("scaled_sq_sums n=%d f1=%d out[%d] (relative)" % (n, with_f1, j), err, 1e-6)
        assert err <= 1e-6
    assert torch.equal(outs[0], outs[1])


# ============================================================================ whole-RHS gradients at the trained widths
RHS_B, RHS_N, RHS_E = 2, 300, 2500     # graph(): a hub source group and a hub destination group of 400 edges


def t_attention_typed(x, ei, Wq, bq, Wk, bk, H, norm_idx, atype, ov=None, ls=None):
    """t_attention for the per-edge score types (function_transformer_attention.py:230-266)."""
    B, N, _ = x.shape
    dk = Wq.shape[0] // H
    q = (x @ Wq.t() + bq).view(B, N, H, dk).transpose(2, 3)
    k = (x @ Wk.t() + bk).view(B, N, H, dk).transpose(2, 3)
    outs = []
    for b in range(B):
        s = BO.edge_scores(q[b][ei[b, 0]], k[b][ei[b, 1]], atype, dk, ov, ls)     # [E,H]
        outs.append(t_softmax(s, ei[b, norm_idx], N))
    return torch.stack(outs)


@pytest.mark.parametrize("atype,mode,norm_idx", [
    ("scaled_dot", "reference", 1), ("scaled_dot", "per_edge", 0), ("scaled_dot", "per_edge", 1),
    ("exp_kernel", "per_edge", 1), ("cosine_sim", "per_edge", 1), ("pearson", "per_edge", 1)])
def test_transformer_rhs_gradients_at_cora_width(atype, mode, norm_idx):
    """ODEFuncTransformerAtt at Cora's best_params widths: heads 8, attention_dim 128, C 80."""
    B, N, E, C, H, att = RHS_B, RHS_N, RHS_E, 80, 8, 128
    ei = graph(21, N, E, B=B)
    torch.manual_seed(21)
    x = torch.randn(B, N, C, device=DEV)
    x0 = torch.randn(B, N, C, device=DEV)
    R = torch.randn(B, N, C, device=DEV)
    # scores of a few units: q, k entries of deviation scale * sqrt(C); the reference mode sums E keys
    Wq, bq, Wk, bk = qk_params(22, C, att, scale=0.02 if mode == "reference" else 0.15)
    opt = dict(OPT, hidden_dim=C, heads=H, attention_dim=att, function='transformer', attention_norm_idx=norm_idx,
               attention_score_mode=mode, attention_type=atype, add_source=True)
    func = gnpde.ODEFuncTransformerAtt(C, C, opt, DEV).to(DEV)
    lay = func.multihead_att_layer
    OV, LS = 1.2, 6.0        # |q - k|^2 is about 58 per head: exponents near -0.8
    with torch.no_grad():
        for p, v in ((lay.Q.weight, Wq), (lay.Q.bias, bq), (lay.K.weight, Wk), (lay.K.bias, bk)):
            p.copy_(v)
        func.alpha_train.fill_(0.3)
        func.beta_train.fill_(0.6)
        if atype == "exp_kernel":
            lay.output_var.fill_(OV)
            lay.lengthscale.fill_(LS)
    func.edge_index, func.x0 = ei, x0

    def run():
        for p in func.parameters():
            p.grad = None
        xt = x.clone().requires_grad_(True)
        (func(0, xt) * R).sum().backward()
        res = [xt.grad, lay.Q.weight.grad, lay.Q.bias.grad, lay.K.weight.grad, lay.K.bias.grad, func.alpha_train.grad]
        return res + ([lay.output_var.grad, lay.lengthscale.grad] if atype == "exp_kernel" else [])

    got = run()
    assert all(torch.equal(a, b) for a, b in zip(run(), got))

    p64 = [t.double().requires_grad_(True) for t in (x, Wq, bq, Wk, bk)]
    a64 = torch.tensor(0.3, dtype=torch.float64, device=DEV, requires_grad=True)
    e64 = [torch.tensor([v], dtype=torch.float64, device=DEV, requires_grad=True) for v in (OV, LS)]
    if atype == "scaled_dot":
        attn = t_attention(p64[0], ei, *p64[1:], H, norm_idx, mode)
    else:
        attn = t_attention_typed(p64[0], ei, *p64[1:], H, norm_idx, atype, *e64)
    (t_rhs(p64[0], ei, attn.mean(2), a64, 0.6, x0.double()) * R.double()).sum().backward()
    names = ["x", "Wq", "bq", "Wk", "bk", "alpha"]
    want = [p.grad for p in p64] + [a64.grad]
    if atype == "exp_kernel":
        names += ["output_var", "lengthscale"]
        want += [p.grad for p in e64]
    errs = []
    for name, gg, ww in zip(names, got, want):
        floor = float(want[BIAS_OF[name]].abs().max()) if name in BIAS_OF else 1e-30
        errs.append((name, relerr(gg, ww, floor)))
        report("transformer %s %s norm_idx=%d d/d%s" % (atype, mode, norm_idx, name), errs[-1][1], GTOL)
    for name, err in errs:
        assert err <= GTOL, (name, err)


@pytest.mark.parametrize("C", [162, 256])
def test_laplacian_edge_weight_gradient_at_wide_rows(C):
    """BLEND's C = 162 (scalar SDDMM, three trips) and C = 256 (64 lanes of float4)."""
    B, N, E = RHS_B, RHS_N, RHS_E
    ei = graph(23, N, E, B=B)
    torch.manual_seed(23)
    x = torch.randn(B, N, C, device=DEV)
    w = torch.rand(B, E, device=DEV)
    R = torch.randn(B, N, C, device=DEV)
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C), DEV).to(DEV)
    with torch.no_grad():
        func.alpha_train.fill_(0.4)
    func.edge_index = ei

    def run():
        func.alpha_train.grad = None
        wt = w.clone().requires_grad_(True)
        xt = x.clone().requires_grad_(True)
        func.edge_weight = wt
        (func(0, xt) * R).sum().backward()
        return wt, xt, func.alpha_train.grad

    wt, xt, ga = run()
    again = run()
    assert torch.equal(again[0].grad, wt.grad) and torch.equal(again[1].grad, xt.grad) and torch.equal(again[2], ga)
    w64 = w.double().requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    a64 = torch.tensor(0.4, dtype=torch.float64, device=DEV, requires_grad=True)
    (t_rhs(x64, ei, w64, a64) * R.double()).sum().backward()
    errs = [("w", relerr(wt.grad, w64.grad)), ("x", relerr(xt.grad, x64.grad)),
            ("alpha", relerr(ga, a64.grad))]
    for name, err in errs:
        report("laplacian C=%d d/d%s" % (C, name), err, GTOL)
    for name, err in errs:
        assert err <= GTOL, (name, err)


def test_laplacian_attention_mean_gradient_at_8_heads():
    """block='attention' at H = 8, C = 128: the SDDMM writes its value to every head / H."""
    B, N, E, C, H = RHS_B, RHS_N, RHS_E, 128, 8
    ei = graph(24, N, E, B=B)
    torch.manual_seed(24)
    x = torch.randn(B, N, C, device=DEV)
    att = torch.rand(B, E, H, device=DEV)
    R = torch.randn(B, N, C, device=DEV)
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C, block='attention'), DEV).to(DEV)
    func.edge_index = ei

    def run():
        at = att.clone().requires_grad_(True)
        func.attention_weights = at
        (func(0, x) * R).sum().backward()
        return at

    at = run()
    assert torch.equal(run().grad, at.grad)
    a64 = att.double().requires_grad_(True)
    (t_rhs(x.double(), ei, a64.mean(2), torch.tensor(0.0, dtype=torch.float64, device=DEV)) * R.double()).sum() \
        .backward()
    err = relerr(at.grad, a64.grad)
    report("laplacian attention mean H=8 C=128 d/datt", err, GTOL)
    assert err <= GTOL
