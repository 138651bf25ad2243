"""Host: the GDC rewiring's oracle, its schedules, its torch restatement (ops.gdc_torch,
ops.topk_cols_torch) and the gnpde.graph_rewiring plumbing on CPU tensors (no GPU: the driver
is injected), plus the host-side validation of gnpde_topk_cols_f32."""
import numpy as np
import pytest
import torch

import gdc_oracle as KO
from gnpde import GraphData, _lib, apply_gdc, graph_rewiring, ops

FIXTURES = [(n, "ppr", a) for n in KO.SHAPES for a in KO.ALPHAS] + [(n, "heat", KO.HEAT_T) for n in KO.SHAPES]


def _opt(**kw):
    opt = {'gdc_method': 'ppr', 'gdc_sparsification': 'topk', 'gdc_k': 16, 'gdc_threshold': 0.01, 'ppr_alpha': 0.05,
           'heat_time': 3.0, 'self_loop_weight': 1, 'exact': True, 'pos_enc_orientation': 'row'}
    opt.update(kw)
    return opt


def _data(ei, N, w=None, batched=False):
    d = GraphData()
    e = torch.tensor(np.ascontiguousarray(ei))
    d.new_graph(e.unsqueeze(0) if batched else e, N, None if w is None else torch.tensor(w))
    return d


def _kw(method, p):
    return dict(method=method, alpha=p) if method == "ppr" else dict(method=method, t=p)


def test_closed_form_complete_graph():
    """K5 with w_self = 1: T = J / 5, so S = alpha I + (1 - alpha) J / 5 (ppr)."""
    n, a = 5, 0.15
    ei = np.array([(i, j) for i in range(n) for j in range(n) if i != j]).T
    T = KO.transition(KO.dense_m(ei, None, n, 1.0))
    assert np.allclose(T, np.full((n, n), 0.2), atol=1e-15)
    want = a * np.eye(n) + (1 - a) * np.full((n, n), 0.2)
    assert np.allclose(KO.diffusion(T, "ppr", alpha=a), want, atol=1e-14)
    S = ops.gdc_torch(torch.tensor(ei), None, n, method='ppr', alpha=a, dense=True)
    assert np.abs(S.numpy() - want / want.sum(0)).max() <= 1e-6
    ei2, w2 = ops.gdc_torch(torch.tensor(ei), None, n, method='ppr', alpha=a, k=5)
    assert np.array_equal(ei2.numpy(), np.array([(i, j) for i in range(n) for j in range(n)]).T)
    assert np.abs(w2.numpy().reshape(n, n) - want).max() <= 1e-6     # the columns of `want` already sum to 1


def test_decided_share_small():
    for a in KO.ALPHAS:
        res = KO.fixture("small", "ppr", a)[3]
        print("small alpha=%g: decided share %.3f" % (a, KO.decided_share(res)))
        assert KO.decided_share(res) >= 0.9


@pytest.mark.parametrize("method,p", [("ppr", 0.05), ("ppr", 0.15), ("heat", 3.0)])
def test_schedule_bounds_float64(method, p):
    """The float64 iterates of the schedules meet their stated 2-norm bounds."""
    ei, N, k, res = KO.fixture("small", method, p)
    T = KO.transition(KO.dense_m(ei, None, N, 1.0))
    sched = ops.diffusion_schedule(**_kw(method, p))
    if method == "ppr":
        # x_m costs m - 1 products; m is the first index with 2 rho^m <= tol alpha (55 / 29 here,
        # against about 290 / 90 terms of the plain series)
        m = sched.products + 1
        rho = (np.sqrt((2 - p) / p) - 1) / (np.sqrt((2 - p) / p) + 1)
        assert 2 * rho ** m <= 1e-6 * p < 2 * rho ** (m - 1) and m == {0.05: 55, 0.15: 29}[p]
    E = np.eye(N)
    cur, prev = sched.init * E, None
    for cb, cf, ce in sched.steps:
        nxt = cf * (T @ cur) + ce * E + (cb * prev if (sched.two_term and prev is not None) else 0.0)
        prev, cur = cur, nxt
    err = np.linalg.norm(cur - res.S, axis=0).max()
    print("%s %g: %d products, max column 2-norm error %.3e, bound %.3e" % (method, p, sched.products, err,
                                                                          sched.bound))
    assert err <= sched.bound + 1e-13
    scale = p if method == "ppr" else np.exp(-p)
    assert sched.bound <= 1e-6 * scale
    blk = ops.diffusion_block_torch(torch.tensor(T), 128, 100, sched, dtype=torch.float64).numpy()
    assert np.abs(blk - cur[:, 128:228]).max() <= 1e-14


@pytest.mark.parametrize("name,method,p", FIXTURES)
def test_gdc_torch_vs_oracle(name, method, p):
    ei, N, k, res = KO.fixture(name, method, p)
    e, w = ops.gdc_torch(torch.tensor(ei), None, N, k=k, **_kw(method, p))
    assert e.dtype == torch.int64 and w.dtype == torch.float32 and tuple(e.shape) == (2, N * k)
    key = e[0].numpy() * N + e[1].numpy()
    assert (np.diff(key) > 0).all()                       # sorted by (row, col), unique
    KO.check_edges(res, e.numpy(), w.numpy(), N, k)


def test_topk_cols_torch_total_order():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((150, 20)).astype(np.float32)
    y[rng.random(y.shape) < 0.3] = 0.5                    # exact duplicates
    y[rng.random(y.shape) < 0.1] = 0.0
    y[3, 0], y[1, 0] = -0.0, 0.0
    idx, val, wn = ops.topk_cols_torch(torch.tensor(y), 40)
    want, wv = KO.topk(y.astype(np.float64), 40)
    assert np.array_equal(idx.numpy(), want) and np.array_equal(val.numpy(), wv.astype(np.float32))
    s = np.zeros(20, np.float32)
    for i in range(40):
        s = s + val.numpy()[:, i]
    assert np.array_equal(wn.numpy(), val.numpy() / s[:, None])
    with pytest.raises(ValueError, match="exceeds"):
        ops.topk_cols_torch(torch.tensor(y), 151)


def test_isolated_node_pads_with_zero_weight_edges():
    N, k = 12, 4
    ring = np.arange(11)
    ei = np.stack([np.concatenate([ring, (ring + 1) % 11]), np.concatenate([(ring + 1) % 11, ring])])
    e, w = ops.gdc_torch(torch.tensor(ei), None, N, k=k)           # node 11 is isolated
    assert e.shape[1] == N * k
    col = e[1].numpy() == 11
    rows, wc = e[0].numpy()[col], w.numpy()[col]
    assert sorted(rows.tolist()) == [0, 1, 2, 11]
    assert wc[rows == 11] == 1.0 and (wc[rows != 11] == 0.0).all()
    assert np.abs(np.bincount(e[1].numpy(), w.numpy().astype(np.float64)) - 1).max() <= 1e-6


def test_existing_self_loop_summed_or_kept():
    ei, N = KO.graph(40, 4, seed=1)
    ei = np.concatenate([ei, [[7], [7]]], 1)
    w = np.ones(ei.shape[1], np.float32)
    w[-1] = 2.5
    a = 0.15
    # combined: PyG's add_self_loops then coalesce: the loop of node 7 weighs 2.5 + 1
    M = KO.dense_m(ei, w, N, 1.0)
    assert M[7, 7] == 3.5
    res = KO.reference(ei, w, N, 8, "ppr", alpha=a)
    e, wn = ops.gdc_torch(torch.tensor(ei), torch.tensor(w), N, alpha=a, k=8)
    KO.check_edges(res, e.numpy(), wn.numpy(), N, 8)
    # pos_encoding: add_remaining_self_loops keeps the loop's own weight
    Mr = KO.dense_m(ei, w, N, 1.0, remaining=True)
    assert Mr[7, 7] == 2.5 and Mr[6, 6] == 1.0
    S = KO.diffusion(KO.transition(Mr), "ppr", alpha=a)
    d = _data(ei, N, w)
    P = apply_gdc(d, _opt(ppr_alpha=a), type='pos_encoding', gdc=ops.gdc_torch)
    assert np.abs(P.numpy() - S / S.sum(0)).max() <= 1e-5 * (S / S.sum(0)).max()


def test_apply_gdc_option_mapping():
    ei, N, k, res = KO.fixture("small", "ppr", 0.05)
    for batched in (False, True):
        d = apply_gdc(_data(ei, N, batched=batched), _opt(gdc_k=k), gdc=ops.gdc_torch)
        assert d.edge_index.dtype == torch.int64
        assert tuple(d.edge_index.shape) == ((1, 2, N * k) if batched else (2, N * k))
        assert tuple(d.edge_attr.shape) == ((1, N * k) if batched else (N * k,))
        KO.check_edges(res, d.edge_index.reshape(2, -1).numpy(), d.edge_attr.reshape(-1).numpy(), N, k)
    # heat fallback: any other gdc_method
    hres = KO.fixture("small", "heat", KO.HEAT_T)[3]
    d = apply_gdc(_data(ei, N), _opt(gdc_k=k, gdc_method='coeff'), gdc=ops.gdc_torch)
    KO.check_edges(hres, d.edge_index.numpy(), d.edge_attr.numpy(), N, k)
    # self_loop_weight = 0: no self loops
    r0 = KO.reference(ei, None, N, k, "ppr", alpha=0.05, w_self=0.0)
    d = apply_gdc(_data(ei, N), _opt(gdc_k=k, self_loop_weight=0), gdc=ops.gdc_torch)
    KO.check_edges(r0, d.edge_index.numpy(), d.edge_attr.numpy(), N, k)
    # threshold
    thr = 0.01
    d = apply_gdc(_data(ei, N), _opt(gdc_sparsification='threshold', gdc_threshold=thr), gdc=ops.gdc_torch)
    _check_threshold(res, d.edge_index.numpy(), d.edge_attr.numpy(), thr)
    # orientation: col is the transpose of row
    Pr = apply_gdc(_data(ei, N), _opt(), type='pos_encoding', gdc=ops.gdc_torch)
    Pc = apply_gdc(_data(ei, N), _opt(pos_enc_orientation='col'), type='pos_encoding', gdc=ops.gdc_torch)
    assert torch.equal(Pr.T, Pc)
    Sn = res.S / res.S.sum(0)
    assert np.abs(Pr.numpy() - Sn).max(0).max() <= 1e-5 * Sn.max()
    assert np.abs(Pr.numpy().astype(np.float64).sum(0) - 1).max() <= 1e-6


def _check_threshold(res, ei, w, thr):
    """The oracle's edge set, outside the entries within tau_j of the threshold."""
    S, tau = res.S, res.tau
    N = S.shape[0]
    got = np.zeros((N, N), bool)
    got[ei[0], ei[1]] = True
    assert got.sum() == ei.shape[1] and (np.diff(ei[0] * N + ei[1]) > 0).all()
    assert not (got & (S < thr - tau[None, :])).any() and not (~got & (S >= thr + tau[None, :])).any()
    kept = np.where(got, S, 0.0)
    want = kept / kept.sum(0)
    assert np.abs(w - want[ei[0], ei[1]]).max() <= 1e-5 * want.max()


def test_errors():
    ei, N, k, _ = KO.fixture("small", "ppr", 0.05)
    e = torch.tensor(ei)
    with pytest.raises(ValueError, match="to_undirected"):
        ops.gdc_torch(e[:, :-1], None, N, k=4)                       # one direction of an edge missing
    wa = np.ones(ei.shape[1], np.float32)
    wa[0] = 2.0                                                     # same pattern, asymmetric weights
    with pytest.raises(ValueError, match="to_undirected"):
        ops.gdc_torch(e, torch.tensor(wa), N, k=4)
    with pytest.raises(ValueError, match="exceeds"):
        ops.gdc_torch(e, None, N, k=N + 1)
    with pytest.raises(NotImplementedError):
        ops.gdc_torch(torch.stack([e, e]), None, N, k=4)
    with pytest.raises(NotImplementedError):
        apply_gdc(_data(np.stack([ei, ei]), N), _opt(), gdc=ops.gdc_torch)
    with pytest.raises(ValueError, match="self_loop_weight"):
        apply_gdc(_data(ei, N), _opt(exact=False, self_loop_weight=2), gdc=ops.gdc_torch)
    apply_gdc(_data(ei, N), _opt(exact=False, self_loop_weight=1, gdc_k=4), gdc=ops.gdc_torch)   # accepted
    with pytest.raises(ValueError, match="max_bytes"):
        ops.gdc_torch(e, None, N, dense=True, max_bytes=4 * N * N - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        graph_rewiring.GDCWrapper(1, diffusion_kwargs=dict(method='ppr', alpha=0.05), gdc=ops.gdc_torch,
                                  max_bytes=1000).position_encoding(_data(ei, N))


def test_abi_host_validation():
    """gnpde_topk_cols_f32 validates on the host before any launch: no device is touched."""
    fn = lambda N, ncols, ld, k: _lib.call_rc("gnpde_topk_cols_f32", None, N, ncols, ld, k, None, None, None, 0, None,
                                              0, None)     # noqa: E731
    assert fn(1000, 128, 128, 129) == _lib.EUNSUPPORTED
    assert fn(10, 8, 8, 11) == _lib.EINVAL
    assert b"exceeds" in _lib.load().gnpde_last_error()
    assert fn(1000, 128, 64, 16) == _lib.EINVAL
    assert fn(1000, 128, 128, 0) == _lib.EINVAL
    assert fn(1000, 128, 128, 16) == _lib.EINVAL            # NULL arrays
    assert _lib.fn("gnpde_topk_cols_workspace_bytes")(5000, 128, 64, 1024) == 5 * 128 * 64 * 8
    assert _lib.fn("gnpde_topk_cols_workspace_bytes")(300, 128, 64, 0) == 16
