"""Host checks of tests/backward_oracle.py (no GPU).

1. The closed-form references (softmax backward, SDDMM, weighted column sums,
   node-score input gradient, and the closed form of the per-edge score gradient)
   against torch float64 autograd of the forward they differentiate: 1e-12 relative.
2. The inputs of tests/test_gpu_backward_kernels.py discriminate: a kernel that
   dropped the last edge of the longest group, swapped two heads, dropped the last
   column, or forgot the a_own term would move the reference by at least 10x the bar
   the GPU test applies to that kernel, for every input set.  This is a condition on
   the inputs: where a draw fails it the draw changes, never the factor.
   Mutations that are the identity by construction are not listed: two heads of an
   SDDMM hold the same value, a sum over heads (exp_kernel's parameter gradients)
   does not see a swap, and scaled_dot has no a_own term.
"""
import numpy as np
import pytest
import torch

import backward_oracle as BO

F = 10.0          # the mutation must move the reference by F bars
ATOL12 = 1e-12


@pytest.fixture(scope="module")
def ei():
    return BO.unit_graph()


def t64(a, grad=False):
    t = torch.from_numpy(np.array(a, np.float64))
    return t.requires_grad_(True) if grad else t


def swap_heads(a, axis=-1):
    """Heads 0 and H-1 exchanged (H >= 2)."""
    a = np.array(a)
    idx = np.arange(a.shape[axis])
    idx[0], idx[-1] = idx[-1], idx[0]
    return np.take(a, idx, axis=axis)


# ============================================================================ the unit graph
def test_unit_graph_has_the_constructed_groups(ei):
    assert ei.shape == (BO.UNIT_B, 2, BO.UNIT_E) and ei.min() >= 0 and ei.max() < BO.UNIT_N
    for side, nodes in ((0, BO.SRC_NODES), (1, BO.DST_NODES)):
        cnt = np.bincount(BO.groups_of(ei, BO.UNIT_N, side), minlength=BO.UNIT_B * BO.UNIT_N)
        for b in range(BO.UNIT_B):
            assert tuple(cnt[b * BO.UNIT_N + np.asarray(nodes)]) == BO.GROUP_SIZES
        assert cnt.max() == 200      # the longest group is the constructed one


# ============================================================================ 1. references against autograd
@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.SOFTMAX_HEADS)
def test_softmax_backward_reference_is_the_softmax_gradient(ei, side, H):
    gidx = BO.groups_of(ei, BO.UNIT_N, side)
    _, g = BO.softmax_inputs(ei, side, H)
    rng = np.random.default_rng(H)
    s = t64(rng.standard_normal((gidx.size, H)) * 2.0, grad=True)
    gi = torch.from_numpy(gidx)
    R = BO.UNIT_B * BO.UNIT_N
    e = torch.exp(s - s.detach().max())
    att = e / torch.zeros(R, H, dtype=torch.float64).index_add(0, gi, e)[gi]
    (att * t64(g)).sum().backward()
    assert BO.rel(BO.softmax_backward(gidx, att.detach().numpy(), g), s.grad.numpy()) <= ATOL12


@pytest.mark.parametrize("H,C", [(1, 5), (8, 12), (1, 162)])
@pytest.mark.parametrize("alpha", BO.SDDMM_ALPHA)
def test_sddmm_reference_is_the_weight_gradient(ei, H, C, alpha):
    """f = a (A(w) x - x), w the head mean of wh [B,E,H]; L = <gf, f>."""
    gf, x = BO.sddmm_inputs(H, C)
    a = BO.alpha_scale(alpha)
    B, N, E = BO.UNIT_B, BO.UNIT_N, BO.UNIT_E
    wh = t64(np.random.default_rng(3).uniform(0.1, 1.0, (B, E, H)), grad=True)
    w = wh.mean(2)
    x64, L = t64(x), 0.0
    for b in range(B):
        ax = torch.zeros(N, C, dtype=torch.float64).index_add(0, torch.from_numpy(ei[b, 0]),
                                                              w[b][:, None] * x64[b][ei[b, 1]])
        L = L + (t64(gf)[b] * (a * (ax - x64[b]))).sum()
    L.backward()
    want = wh.grad.numpy()
    got = BO.sddmm(ei, gf, x, a, H)
    assert BO.rel(got.reshape(want.shape), want) <= ATOL12


@pytest.mark.parametrize("B,N,C,H", [(3, 257, 162, 1), (2, 300, 5, 2)])
def test_wcolsum_and_score_input_grad_references_are_the_node_score_gradients(B, N, C, H):
    """cs[b,n,h] = x[b,n,:] . U[b,:,h] + v[b,h]  and  xbar[b,:] = sum_n deg[b,n] x[b,n,:];
    L = <gcs, cs> + <gxbar, xbar>:  dL/dU, dL/dv = wcolsum(x, gcs);  dL/dx = score_input_grad."""
    x, gcs = BO.wcolsum_inputs(B, N, C, H)
    rng = np.random.default_rng(7)
    U, v = t64(rng.standard_normal((B, C, H)), grad=True), t64(rng.standard_normal((B, H)), grad=True)
    deg = rng.integers(0, 40, size=(B, N))
    gxbar = rng.standard_normal((B, C))
    xt = t64(x, grad=True)
    cs = torch.einsum('bnc,bch->bnh', xt, U) + v[:, None, :]
    xbar = (t64(deg)[:, :, None] * xt).sum(1)
    ((t64(gcs) * cs).sum() + (t64(gxbar) * xbar).sum()).backward()
    y = BO.wcolsum(x, gcs)
    assert BO.rel(y[:, :, :C], U.grad.numpy().transpose(0, 2, 1)) <= ATOL12
    assert BO.rel(y[:, :, C], v.grad.numpy()) <= ATOL12
    gx = BO.score_input_grad(gcs, U.detach().numpy(), deg, gxbar, dtype=np.float64)
    assert BO.rel(gx, xt.grad.numpy()) <= ATOL12


@pytest.mark.parametrize("mode,H,dk", BO.SCORE_CASES)
def test_score_grad_closed_form_is_the_autograd_gradient(ei, mode, H, dk):
    q, k, gs, p0, p1 = BO.score_inputs(mode, H, dk)
    gq, gk, _, _ = BO.score_grad(ei, q, k, gs, mode, H, dk, p0, p1)
    assert BO.rel(BO.score_grad_closed(ei, q, k, gs, mode, H, dk, 0, p0, p1), gq) <= ATOL12
    assert BO.rel(BO.score_grad_closed(ei, q, k, gs, mode, H, dk, 1, p0, p1), gk) <= ATOL12


def test_exp_kernel_parameter_gradients_match_the_header_formulas(ei):
    """ds/dov = 2 s / ov, ds/dls = s |q-k|^2 / ls^3, summed over edges and heads."""
    mode, H, dk = "exp_kernel", 8, 16
    q, k, gs, p0, p1 = BO.score_inputs(mode, H, dk)
    _, _, gov, gls = BO.score_grad(ei, q, k, gs, mode, H, dk, p0, p1)
    s = BO.score_values(ei, BO.UNIT_N, q, k, mode, H, dk, p0, p1)
    d2 = -2.0 * p1 ** 2 * np.log(s / p0 ** 2)
    g64 = np.asarray(gs, np.float64)
    assert abs((g64 * 2 * s / p0).sum() - gov) <= 1e-11 * abs(gov)
    assert abs((g64 * s * d2 / p1 ** 3).sum() - gls) <= 1e-11 * abs(gls)


# ============================================================================ 2. the inputs discriminate
def moved(ref, mut, bar):
    """The largest move of the reference in units of the elementwise bar."""
    return BO.exceed(mut, ref, bar)


@pytest.mark.parametrize("H,C", BO.SDDMM_CASES)
def test_sddmm_inputs_see_a_dropped_column(ei, H, C):
    gf, x = BO.sddmm_inputs(H, C)
    ref = BO.sddmm(ei, gf, x, 1.0, H)
    xm = x.copy()
    xm[..., C - 1] = 0.0
    assert BO.rel(BO.sddmm(ei, gf, xm, 1.0, H), ref) >= F * BO.RTOL


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.SOFTMAX_HEADS)
def test_softmax_backward_inputs_see_a_dropped_edge_and_swapped_heads(ei, side, H):
    gidx = BO.groups_of(ei, BO.UNIT_N, side)
    att, g = BO.softmax_inputs(ei, side, H)
    ref = BO.softmax_backward(gidx, att, g)
    bar = BO.softmax_backward_bar(ref, g)
    r, e = BO.longest_group_last_edge(gidx)
    keep = np.delete(np.arange(gidx.size), e)
    mut = BO.softmax_backward(gidx[keep], att[keep], g[keep])
    rows = gidx[keep] == r
    assert moved(ref[keep][rows], mut[rows], bar[keep][rows]) >= F
    if H > 1:
        assert moved(ref, BO.softmax_backward(gidx, att, swap_heads(g)), bar) >= F


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("H", BO.SEGSUM_HEADS)
def test_segment_sum_inputs_see_a_dropped_edge_and_swapped_heads(ei, side, H):
    gidx = BO.groups_of(ei, BO.UNIT_N, side)
    R = BO.UNIT_B * BO.UNIT_N
    v = BO.segsum_inputs(side, H)
    ref, bar = BO.segment_sum(gidx, v, R), BO.segment_sum_bar(gidx, v, R)
    r, e = BO.longest_group_last_edge(gidx)
    keep = np.delete(np.arange(gidx.size), e)
    assert moved(ref[r], BO.segment_sum(gidx[keep], v[keep], R)[r], bar[r]) >= F
    if H > 1:
        assert moved(ref, BO.segment_sum(gidx, swap_heads(v), R), bar) >= F


@pytest.mark.parametrize("B,N,C,H", BO.WCOLSUM_CASES)
def test_wcolsum_inputs_see_a_dropped_column_and_swapped_heads(B, N, C, H):
    x, w = BO.wcolsum_inputs(B, N, C, H)
    ref, bar = BO.wcolsum(x, w), BO.wcolsum_bar(x, w)
    xm = x.copy()
    xm[..., C - 1] = 0.0
    assert moved(ref, BO.wcolsum(xm, w), bar) >= F
    if H > 1:
        assert moved(ref, BO.wcolsum(x, swap_heads(w)), bar) >= F


@pytest.mark.parametrize("B,N,C,H", BO.SIG_CASES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_score_input_grad_inputs_see_a_dropped_column_and_swapped_heads(B, N, C, H, accumulate):
    gcs, U, deg, gxbar, gx0 = BO.sig_inputs(B, N, C, H)
    g0 = gx0 if accumulate else None
    ref = BO.score_input_grad(gcs, U, deg, gxbar, g0)
    bar = BO.score_input_grad_bar(ref)
    gm = gcs.copy()
    gm[..., H - 1] = 0.0                     # the head loop one trip short
    assert moved(ref, BO.score_input_grad(gm, U, deg, gxbar, g0), bar) >= F
    if H > 1:
        assert moved(ref, BO.score_input_grad(swap_heads(gcs), U, deg, gxbar, g0), bar) >= F


def test_gather_head_and_gat_inputs_see_swapped_heads(ei):
    """Both kernels are held to exact equality: any move counts."""
    for H in BO.GATHER_HEADS:
        if H > 1:
            w = BO.gather_inputs(H)
            assert (w[:, 0] != w[:, H - 1]).all()
    for H in BO.GAT_HEADS:
        sp, gs = BO.gat_inputs(ei, H)
        ref = BO.gat_score_backward(ei, sp, BO.GAT_SLOPE, gs)
        assert ((ref == gs) | (ref == gs * np.float32(BO.GAT_SLOPE))).all()
        assert (ref == gs).any() and (ref != gs).any()        # both branches of the LeakyReLU
        if H > 1:
            spm = np.concatenate([swap_heads(sp[:, :H]), sp[:, H:]], 1)
            assert (BO.gat_score_backward(ei, spm, BO.GAT_SLOPE, gs) != ref).any()


@pytest.mark.parametrize("mode,H,dk", BO.SCORE_CASES)
def test_score_grad_inputs_discriminate(ei, mode, H, dk):
    q, k, gs, p0, p1 = BO.score_inputs(mode, H, dk)
    s = BO.score_values(ei, BO.UNIT_N, q, k, mode, H, dk, p0, p1)
    # scores neither saturate nor vanish; the cosine's eps clamp is inactive
    if mode == "scaled_dot":
        assert 1.0 < np.abs(s).max() < 8.0
    elif mode == "exp_kernel":
        assert 0.01 * p0 ** 2 < s.min() and 0.3 * p0 ** 2 < np.median(s) < 0.9 * p0 ** 2
    else:
        assert np.abs(s).max() < 1.0 - 1e-6 and np.abs(s).max() > 0.2
    assert BO.min_head_norm(q, k, mode, H, dk) > 1e-2
    ref = BO.score_grad(ei, q, k, gs, mode, H, dk, p0, p1)
    att = H * dk
    last = np.arange(dk - 1, att, dk)                          # the last element of every head
    for side in (0, 1):
        gidx = BO.groups_of(ei, BO.UNIT_N, side)
        _, e = BO.longest_group_last_edge(gidx)
        gm = gs.copy()
        gm[e] = 0.0                                            # L = sum gs s: the edge drops out
        assert BO.rel(BO.score_grad(ei, q, k, gm, mode, H, dk, p0, p1)[side], ref[side]) >= F * BO.GTOL
        if H > 1:
            mut = BO.score_grad(ei, q, k, swap_heads(gs), mode, H, dk, p0, p1)[side]
            assert BO.rel(mut, ref[side]) >= F * BO.GTOL
        # the other operand's last element of every head left out of the sums
        qm, km = q.copy(), k.copy()
        (km if side == 0 else qm)[:, last] = 0.0
        mut = BO.score_grad(ei, qm, km, gs, mode, H, dk, p0, p1)
        assert BO.rel(mut[side], ref[side]) >= F * BO.GTOL
        if mode == "exp_kernel":
            for j in (2, 3):
                assert abs(mut[j] - ref[j]) >= F * BO.GTOL * abs(ref[j])
        if mode != "scaled_dot":
            mut = BO.score_grad_closed(ei, q, k, gs, mode, H, dk, side, p0, p1, drop_own=True)
            assert BO.rel(mut, ref[side]) >= F * BO.GTOL


@pytest.mark.parametrize("n", [n for n in BO.SUM_NS if n > 1])
def test_reduction_inputs_see_a_dropped_last_element(n):
    v = BO.sum_inputs(n)
    assert abs(v[-1]) >= F * BO.sum_bar(v)
    y0, f0, f1 = BO.sq_inputs(n)
    a, b = BO.scaled_sq_sums(y0, f0, None, BO.SQ_ATOL, BO.SQ_RTOL)
    a1, b1 = BO.scaled_sq_sums(y0[:-1], f0[:-1], None, BO.SQ_ATOL, BO.SQ_RTOL)
    c, c1 = (BO.scaled_sq_sums(y0[:m], f0[:m], f1[:m], BO.SQ_ATOL, BO.SQ_RTOL) for m in (n, n - 1))
    if n <= 4096:        # one term of a million is below 10 x 1e-6 of the sum: the small sizes carry this
        assert a - a1 >= F * 1e-6 * a and b - b1 >= F * 1e-6 * b and c - c1 >= F * 1e-6 * c
