"""GPU: the positional-encoding distance kernels (csrc/posdist.hip through ops.pos_knn,
ops.pair_select / pair_quantile, ops.pair_threshold_edges) and gnpde.apply_pos_dist_rewire on the
device, against the float64 oracle of tests/posdist_oracle.py.

Acceptance (posdist_oracle.check_knn / check_edges): the index and edge sets match the oracle
outside the band of entries whose float64 u lies within tau of the oracle's k-th or threshold
value; every emitted edge has u <= u_thr (1 + tau); every oracle edge below the band is
present; the band holds at most 1 % of the kept entries (a condition: a fixture over the limit
fails).  Shapes: M = 1; one partial tile with odd C; HYPS16's width over three row tiles; two
column chunks (a short one, DW64's two whole ones); norms up to 0.95 with one row outside the
ball (the eps clamp) and one at the origin.  Bitwise: ties on an exact lattice, ranks above 2^32
(closed form, no oracle matrix), determinism, Euclidean pos_knn against ops.knn."""
import numpy as np
import pytest
import torch

import posdist_oracle as PO
from gnpde import GraphData, apply_pos_dist_rewire, ops
from test_gpu_parity import T

pytestmark = pytest.mark.gpu

CASES = [(n, m) for n in PO.SHAPES for m in PO.METRICS]


@pytest.mark.parametrize("name,metric", CASES)
def test_pos_knn_vs_oracle(name, metric):
    x, u, tm = PO.fixture(name, metric)
    N, C, k, _ = PO.SHAPES[name]
    idx, dist, n_valid = ops.pos_knn(T(x), k, metric, return_dist=True)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1, N, k) and n_valid.tolist() == [N]
    got = idx[0].cpu().numpy().astype(np.int64)
    PO.check_knn(u, tm, k, got, "%s %s" % (name, metric))
    assert (got[:, 0] == np.arange(N)).all()                         # u_ii = 0 and no duplicate points
    ug, tg = np.take_along_axis(u, got, 1), np.take_along_axis(tm, got, 1)
    Dg = PO.dist_from_u(ug, metric)
    # |dD / D| <= |du / u| for both metrics; 8 e for sqrtf / log1pf and the fp32 steps between them
    assert (np.abs(dist[0].double().cpu().numpy() - Dg) <= (tg + 8 * PO.E32) * Dg).all()
    idx2, _ = ops.pos_knn(T(x), k, metric)                           # dist_out = NULL
    assert torch.equal(idx, idx2)


@pytest.mark.parametrize("name,metric", CASES)
def test_pair_threshold_vs_oracle(name, metric):
    x, u, tm = PO.fixture(name, metric)
    N = len(x)
    tx = T(x)
    tmax = tm[np.isfinite(tm)].max()
    for q in PO.QUANTS[name]:
        what = "%s %s q=%g" % (name, metric, q)
        thr_o, u_lo_o = PO.quantile_threshold(u, q, metric)
        thr, u_lo, cnt = ops.pair_quantile(tx, q, metric)
        assert thr.dtype == torch.float64 and thr.is_cuda and u_lo.dtype == torch.float32 and cnt.dtype == torch.int64
        print("%s: u_lo %.9g (oracle %.9g), thr %.9g (oracle %.9g), count_le %d" % (
            what, float(u_lo), u_lo_o, float(thr), thr_o, int(cnt)))
        assert abs(float(u_lo) - u_lo_o) <= tmax * u_lo_o
        assert abs(float(thr) - thr_o) <= (tmax + 8 * PO.E32) * thr_o or not np.isfinite(thr_o)
        ei = ops.pair_threshold_edges(tx, q, metric)
        assert ei.dtype == torch.int64 and ei.is_cuda and int(cnt) == ei.shape[1]
        e = ei.cpu().numpy()
        PO.check_edges(u, tm, u_lo_o, e, what)
        if q == 0.0:                                                  # exactly the N self loops (no duplicate points)
            assert np.array_equal(e, np.stack([np.arange(N), np.arange(N)]))
        if q == 1.0 and np.isfinite(u).all():                         # all N^2 pairs in numpy.where order
            assert np.array_equal(e, np.stack(np.where(np.ones((N, N), bool))))


@pytest.mark.parametrize("quant", [0.0, 0.02, 0.3, 0.5])
def test_ties_bitwise(quant):
    """Duplicated points on an exact lattice, Euclidean: every fp32 u is exact, tied u straddle
    rank lo; all tied entries are kept and count_le equals the oracle's count exactly."""
    x = PO.ties_points()
    N = len(x)
    u = PO.rank_values(x, 'euclid')
    assert np.array_equal(u, u.astype(np.float32).astype(np.float64))
    lo = ops.pair_rank(N, quant)[0]
    su = np.sort(u.reshape(-1))
    u_lo = su[lo]
    assert su[lo + 1] == u_lo and (quant == 0.0 or su[lo - 1] == u_lo)    # ties on both sides of the rank
    thr, gu, cnt = ops.pair_quantile(T(x), quant, 'euclid')
    assert float(gu) == u_lo and int(cnt) == int((u <= u_lo).sum())
    assert abs(float(thr) - np.quantile(np.sqrt(u), quant)) <= 1e-15 * float(thr)
    ei = ops.pair_threshold_edges(T(x), quant, 'euclid')
    assert np.array_equal(ei.cpu().numpy(), np.stack(np.where(u <= u_lo)))
    if quant == 0.0:
        assert ei.shape[1] > N                                        # the self loops plus the duplicates
    # the kNN on the same lattice: the (u, j) order to the bit
    idx, dist, _ = ops.pos_knn(T(x), 16, 'euclid', return_dist=True)
    assert np.array_equal(idx[0].cpu().numpy().astype(np.int64), PO.knn(u, 16))
    assert np.array_equal(dist[0].cpu().numpy(), np.sqrt(np.sort(u, 1)[:, :16]).astype(np.float32))


def test_rank_above_2_pow_32():
    """N = 66,000 points on a line, x_i = i: N^2 > 2^32.  u = (i - j)^2, small ones exact; the
    pairs with |i - j| <= m number N + 2 sum_{t <= m} (N - t).  A rank inside m = 2 must give
    u = 4, that count, and exactly the edges {|i - j| <= 2}; the first digit's bins already hold
    more than 2^32 entries there.  The select is also run at ranks beyond 2^32 (just past it,
    and among the largest u), where the residual rank and the running count exceed 32 bits too.
    Any count held in 32 bits fails."""
    N = 66000
    x = torch.arange(N, dtype=torch.float32, device="cuda").reshape(N, 1)
    M = N * N
    assert M > 1 << 32
    count = lambda m: N + 2 * m * N - m * (m + 1)                    # noqa: E731  (N + 2 sum_{t <= m} (N - t))
    lo = (count(1) + count(2)) // 2
    quant = (lo + 0.5) / (M - 1)
    assert ops.pair_rank(N, quant)[0] == lo and count(1) <= lo < count(2)
    thr, u_lo, cnt = ops.pair_quantile(x, quant, 'euclid')
    assert float(u_lo) == 4.0 and int(cnt) == count(2) and float(thr) == 2.0
    ei = ops.pair_threshold_edges(x, quant, 'euclid').cpu().numpy()
    i = np.repeat(np.arange(N), 5)
    j = i + np.tile(np.arange(-2, 3), N)
    ok = (j >= 0) & (j < N)
    assert np.array_equal(ei, np.stack([i[ok], j[ok]]))
    # ranks past 2^32: the residual ranks and the running count exceed 32 bits
    big = M - 4                                                        # |i - j| = N - 1 holds ranks M-2, M-1; N - 2 holds M-6 .. M-3
    u_big, c_big = ops.pair_select(x, big, 'euclid')
    assert float(u_big) == float(np.float32(N - 2) ** 2) and int(c_big) == M - 2
    u_top, c_top = ops.pair_select(x, M - 1, 'euclid')
    assert float(u_top) == float(np.float32(N - 1) ** 2) and int(c_top) == M
    mid = (1 << 32) + 12345                                            # a rank just past 2^32
    # |i - j| = t has 2 (N - t) pairs: the rank's t from the closed form; u = fl32(t^2), distinct for distinct t
    t = next(t for t in range(N) if count(t) > mid)
    u_mid, c_mid = ops.pair_select(x, mid, 'euclid')
    assert float(u_mid) == float(np.float32(t) * np.float32(t)) and int(c_mid) == count(t)


def test_determinism():
    x, _u, _tm = PO.fixture("dw64", "poincare")
    tx = T(x)
    a = ops.pos_knn(tx, 64, 'poincare', return_dist=True)
    b = ops.pos_knn(tx, 64, 'poincare', return_dist=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    qa, qb = ops.pair_quantile(tx, 0.3, 'poincare'), ops.pair_quantile(tx, 0.3, 'poincare')
    assert all(torch.equal(p, q) for p, q in zip(qa, qb))
    ea, eb = ops.pair_threshold_edges(tx, 0.3, 'poincare'), ops.pair_threshold_edges(tx, 0.3, 'poincare')
    assert torch.equal(ea, eb) and ea.shape[1] == int(qa[2])


@pytest.mark.parametrize("name", ["partial", "hyps16", "dw64"])
def test_euclid_pos_knn_equals_knn(name):
    """No zero row in these fixtures: Euclidean pos_knn selects on the same bits as ops.knn."""
    x = PO.points(name)
    k = PO.SHAPES[name][2]
    assert not (x == 0).all(1).any()
    i1, d1, _ = ops.pos_knn(T(x), k, 'euclid', return_dist=True)
    i0, d0, _ = ops.knn(T(x), k, return_dist=True)
    assert torch.equal(i1, i0) and np.array_equal(d1.cpu().numpy(), np.sqrt(d0.cpu().numpy()))


def test_masked_rows_and_batch():
    x = np.stack([PO.points("hyps16"), PO.points("rim")]).copy()
    x[0, 5, 2] = np.nan
    idx, n_valid = ops.pos_knn(T(x), 8, 'poincare')
    assert n_valid.tolist() == [164, 165]
    got = idx.cpu().numpy()
    assert (got[0, 5] == 5).all() and not (got[0, np.arange(165) != 5] == 5).any()
    assert (got[1] == 100).any() and got[1, 100, 0] == 100             # the origin is a point like any other
    assert torch.equal(ops.pos_knn(T(x[1]), 8, 'poincare')[0][0], idx[1])   # no leakage across graphs
    with pytest.raises(ValueError, match="non-finite"):
        ops.pair_threshold_edges(T(x[0]), 0.5, 'poincare')
    with pytest.raises(ValueError, match="range"):
        ops.pos_knn(T(x), 65, 'poincare')


def test_poincare_dist_of_huge_u():
    """Two rows outside the ball (both clamped, r = 2^52): their u ~ 2^104 d stays inside fp32 but
    u (u + 1) does not; the reported distance is still arccosh(1 + 2u), about 74, not inf.  k = N, so
    every pair's distance comes back: small u, u ~ 2^52 (one clamped row) and u ~ 2^104."""
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.4, 0.4, size=(8, 3)).astype(np.float32)
    x[1] *= np.float32(1.25 / np.linalg.norm(x[1]))
    x[5] *= np.float32(1.5 / np.linalg.norm(x[5]))
    u = PO.rank_values(x, 'poincare')
    assert 1e30 < u[1, 5] < 3e38 and 1e12 < u[1, 0] < 1e19 and u[0, 2] < 10
    idx, dist, _ = ops.pos_knn(T(x), 8, 'poincare', return_dist=True)
    got = idx[0].cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(got, 1), np.tile(np.arange(8), (8, 1)))
    Dg = PO.dist_from_u(np.take_along_axis(u, got, 1), 'poincare')
    tg = np.take_along_axis(PO.tau_matrix(x, 'poincare'), got, 1)
    d = dist[0].double().cpu().numpy()
    assert np.isfinite(d).all() and (np.abs(d - Dg) <= (tg + 8 * PO.E32) * Dg).all()
    assert got[1, 7] == 5 and 70.0 < d[1, 7] < 80.0


def test_edge_limit_raises_before_allocation(monkeypatch):
    """E at or above the limit raises after the count pass, before the edge list exists."""
    x = T(PO.points("hyps16"))
    E = ops.pair_threshold_edges(x, 0.25, 'euclid').shape[1]
    monkeypatch.setattr(ops, "POSDIST_MAX_EDGES", E)
    real_empty = torch.empty

    def no_edge_list(*size, **kw):
        assert not (len(size) == 2 and size[0] == 2 and kw.get("dtype") == torch.int64), "the edge list was allocated"
        return real_empty(*size, **kw)
    monkeypatch.setattr(torch, "empty", no_edge_list)
    with pytest.raises(ValueError, match="limit"):
        ops.pair_threshold_edges(x, 0.25, 'euclid')
    monkeypatch.setattr(ops, "POSDIST_MAX_EDGES", E + 1)
    monkeypatch.setattr(torch, "empty", real_empty)
    assert ops.pair_threshold_edges(x, 0.25, 'euclid').shape[1] == E


def _opt(**kw):
    opt = {'pos_enc_type': 'HYPS16', 'gdc_sparsification': 'topk', 'gdc_k': 16, 'pos_dist_quantile': 0.01}
    opt.update(kw)
    return opt


def _data(N, dev):
    d = GraphData()
    d.new_graph(torch.zeros(2, 5, dtype=torch.int64, device=dev), N, torch.ones(5, device=dev))
    return d


@pytest.mark.parametrize("name", ["hyps16", "rim"])
@pytest.mark.parametrize("typ", ["HYPS16", "DW64"])
def test_apply_pos_dist_rewire_end_to_end(name, typ):
    """The HIP backend against the torch backend on the fixtures, outside the band (each is
    checked against the oracle; where the band is empty the two are equal)."""
    x = PO.points(name)
    N, C, k, _ = PO.SHAPES[name]
    metric = 'poincare' if typ.startswith("HYP") else 'euclid'
    _, u, tm = PO.fixture(name, metric)
    tx = T(x)
    d = apply_pos_dist_rewire(_data(N, tx.device), _opt(pos_enc_type=typ), tx)
    t = apply_pos_dist_rewire(_data(N, "cpu"), _opt(pos_enc_type=typ), torch.tensor(x), backend=ops.POSDIST_TORCH)
    assert d.edge_index.is_cuda and d.edge_index.dtype == torch.int64 and tuple(d.edge_index.shape) == (2, N * k)
    band = PO.check_knn(u, tm, k, d.edge_index[1].reshape(N, k).cpu().numpy(), "rewire topk")
    PO.check_knn(u, tm, k, t.edge_index[1].reshape(N, k).numpy(), "rewire topk (torch)")
    if band == 0:
        assert np.array_equal(np.sort(d.edge_index[1].reshape(N, k).cpu().numpy(), 1),
                              np.sort(t.edge_index[1].reshape(N, k).numpy(), 1))
    for q in (0.01, 0.25):
        o = _opt(pos_enc_type=typ, gdc_sparsification='threshold', pos_dist_quantile=q)
        d = apply_pos_dist_rewire(_data(N, tx.device), o, tx)
        t = apply_pos_dist_rewire(_data(N, "cpu"), o, torch.tensor(x), backend=ops.POSDIST_TORCH)
        qq = q if metric == 'poincare' else 0.001                     # DW: apply_dist_threshold's default
        u_lo = PO.quantile_threshold(u, qq, metric)[1]
        band = PO.check_edges(u, tm, u_lo, d.edge_index.cpu().numpy(), "rewire thr")
        PO.check_edges(u, tm, u_lo, t.edge_index.numpy(), "rewire thr (torch)")
        if band == 0:
            assert np.array_equal(d.edge_index.cpu().numpy(), t.edge_index.numpy())
    with pytest.raises(NotImplementedError):
        apply_pos_dist_rewire(_data(N, tx.device), _opt(gdc_sparsification='threshold'), torch.stack([tx, tx]))
