"""Host: the positional-encoding distance rewiring's oracle against its golden fixtures, the
torch restatements (ops.pos_knn_torch, ops.pair_quantile_torch, ops.pair_threshold_edges_torch)
against the oracle, ops.pair_rank against numpy, the set identity the threshold kernels rest
on, the host-side validation and workspace bounds of the new entry points, and
gnpde.apply_pos_dist_rewire on CPU tensors with the torch backend injected."""
import json
import os

import numpy as np
import pytest
import torch

import posdist_oracle as PO
from conftest import GOLDEN
from gnpde import (GraphData, _lib, apply_dist_KNN, apply_dist_threshold, apply_feat_KNN, apply_pos_dist_rewire,
                   hyperbolize, ops)

GDIR = os.path.join(GOLDEN, "posdist")
CASES = [(n, m) for n in PO.SHAPES for m in PO.METRICS]
BE = ops.POSDIST_TORCH


def _golden_names():
    with open(os.path.join(GDIR, "MANIFEST.json")) as fh:
        return json.load(fh)


def test_manifest_lists_the_fixtures():
    assert sorted(f for f in os.listdir(GDIR) if f.endswith(".npz")) == _golden_names()
    assert len(_golden_names()) == 6


@pytest.mark.parametrize("fn", ["partial_poincare", "partial_euclid", "hyps16_poincare", "hyps16_euclid",
                                "rim_poincare", "rim_euclid"])
def test_oracle_vs_golden(fn):
    """scipy / sklearn / numpy composed as the reference's lines intend, against the oracle."""
    g = np.load(os.path.join(GDIR, fn + ".npz"))
    name, metric = fn.rsplit("_", 1)
    x, u, tm = PO.fixture(name, metric)
    assert np.array_equal(g["x"], x)
    D = PO.dist_from_u(u, metric)
    # arccosh(1 + 2u) as scipy's composition evaluates it cancels below u ~ 1e-8; these D are O(0.1) and above
    off = ~np.eye(len(x), dtype=bool)
    assert np.abs(D - g["D"])[off].max() <= 1e-9 * D.max() and (np.diag(g["D"]) == 0).all() and (np.diag(D) == 0).all()
    # sklearn breaks ties in no fixed order: sets, on the rows whose k + 1 smallest are distinct
    k = PO.SHAPES[name][2]
    idx = PO.knn(u, k)
    su = np.sort(u, axis=1)[:, :k + 1]
    strict = (np.diff(su, axis=1) > 1e-9 * su[:, 1:]).all(axis=1)
    assert strict.mean() >= 0.9
    assert np.array_equal(np.sort(idx[strict], 1), np.sort(g["knn"][strict].astype(np.int64), 1))
    for i, q in enumerate(g["quants"]):
        thr, u_lo = PO.quantile_threshold(u, q, metric)
        assert abs(thr - g["thr"][i]) <= 1e-9 * max(thr, 1e-300)
        want = g["edges_%d" % i].astype(np.int64)
        assert np.array_equal(PO.threshold_edges(u, q, metric), want)
        assert np.array_equal(np.stack(np.where(u <= u_lo)), want)      # the set identity on a golden


@pytest.mark.parametrize("N,quant", [(63, .001), (165, .01), (165, .5), (40, 0.0), (40, 1.0), (63, 0.25), (165, 0.25)])
def test_set_identity(N, quant):
    """{D <= numpy.quantile(D)} = {u <= u_(lo)} with lo from ops.pair_rank: equal sets, both metrics."""
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((N, 5)) * 0.3).astype(np.float32)
    x[N // 2] = x[1]                                                 # a duplicate: ties at u = 0
    for metric in PO.METRICS:
        u = PO.rank_values(x, metric)
        lo, hi, frac = ops.pair_rank(N, quant)
        assert (lo, hi) == PO.pair_rank(N, quant)[:2]
        u_lo = np.sort(u.reshape(-1))[lo]
        a = PO.threshold_edges(u, quant, metric)
        b = np.stack(np.where(u <= u_lo))
        assert np.array_equal(a, b)
        if quant == 0.0:
            assert a.shape[1] == N + 2                               # the diagonal and the duplicate pair
        if quant == 1.0:
            assert a.shape[1] == N * N


def test_pair_rank_vs_numpy():
    try:    # numpy's own index arithmetic, where this numpy still keeps it there (a private path)
        from numpy.lib._function_base_impl import _QuantileMethods
        virtual = _QuantileMethods['linear']['get_virtual_index']
    except (ImportError, KeyError, AttributeError):
        virtual = None
    rng = np.random.default_rng(0)
    quants = [0.0, 1.0, 0.001, 0.5, 0.25, 1 / 3, 0.999999] + rng.random(40).tolist()
    for N in (1, 2, 63, 165, 2708, 19717, 169343, 1 << 20):
        M = N * N
        for q in quants:
            lo, hi, frac = ops.pair_rank(N, q)
            assert 0 <= lo <= hi == min(lo + 1, M - 1) and 0.0 <= frac < 1.0
            if virtual is not None:
                v = float(virtual(M, np.float64(q)))
                assert lo == min(int(np.floor(v)), M - 1)
                assert frac == (v - np.floor(v) if hi > lo else 0.0)
            # and the exact position q (M - 1): within an ulp of the index
            elo, _ehi, efrac = PO.pair_rank(N, q)
            assert abs((lo + frac) - (elo + efrac)) <= 4 * np.spacing(float(M))
    # small N: the quantile of 0..M-1 IS the position
    for N in (3, 17, 40):
        M = N * N
        for q in quants:
            lo, hi, frac = ops.pair_rank(N, q)
            a = np.arange(M, dtype=np.float64)
            assert np.quantile(a, q) == ops._quantile_lerp(a[lo], a[hi], frac)
    assert ops.pair_rank(169343, 0.001)[0] == 28677051                # floor(0.001 (169343^2 - 1))
    for bad in (-1e-9, 1.0000001, float("nan")):
        with pytest.raises(ValueError, match="outside"):
            ops.pair_rank(10, bad)


@pytest.mark.parametrize("name,metric", CASES)
def test_pos_knn_torch_vs_oracle(name, metric):
    x, u, tm = PO.fixture(name, metric)
    N, C, k, _ = PO.SHAPES[name]
    idx, dist, n_valid = ops.pos_knn_torch(torch.tensor(x), k, metric, return_dist=True)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1, N, k) and n_valid.tolist() == [N]
    PO.check_knn(u, tm, k, idx[0].numpy(), "%s %s" % (name, metric))
    ug = np.take_along_axis(u, idx[0].numpy().astype(np.int64), 1)
    tg = np.take_along_axis(tm, idx[0].numpy().astype(np.int64), 1)
    Dg = PO.dist_from_u(ug, metric)
    # D(u) has |dD/D| <= |du/u| for both metrics (sqrt halves it; arccosh(1 + 2u) is concave in log u)
    assert (np.abs(dist[0].double().numpy() - Dg) <= (tg + 4 * PO.E32) * Dg).all()
    assert (idx[0, :, 0].numpy() == np.arange(N)).all()              # the self index first: u_ii = 0, no duplicates here


@pytest.mark.parametrize("name,metric", CASES)
def test_pair_torch_vs_oracle(name, metric):
    x, u, tm = PO.fixture(name, metric)
    N = len(x)
    for q in PO.QUANTS[name]:
        thr_o, u_lo_o = PO.quantile_threshold(u, q, metric)
        thr, u_lo, cnt = ops.pair_quantile_torch(torch.tensor(x), q, metric)
        assert thr.dtype == torch.float64 and cnt.dtype == torch.int64
        tmax = tm[np.isfinite(tm)].max()
        assert abs(float(u_lo) - u_lo_o) <= tmax * u_lo_o
        assert abs(float(thr) - thr_o) <= (tmax + 4 * PO.E32) * thr_o or not np.isfinite(thr_o)
        ei = ops.pair_threshold_edges_torch(torch.tensor(x), q, metric)
        assert ei.dtype == torch.int64 and int(cnt) == ei.shape[1]
        PO.check_edges(u, tm, u_lo_o, ei.numpy(), "%s %s q=%g" % (name, metric, q))
        if q == 0.0:
            assert ei.shape[1] == N and (ei[0] == ei[1]).all()
        if q == 1.0:
            assert np.array_equal(ei.numpy(), np.stack(np.where(np.ones((N, N), bool))))


def test_torch_backends_raise():
    x = torch.tensor(PO.points("partial"))
    with pytest.raises(ValueError, match="max_bytes"):
        ops.pair_quantile_torch(x, 0.5, 'euclid', max_bytes=4 * 63 * 63 - 1)
    with pytest.raises(ValueError, match="max_bytes"):
        ops.pair_threshold_edges_torch(x, 0.5, 'euclid', max_bytes=100)
    with pytest.raises(ValueError, match="max_bytes"):
        hyperbolize(x, max_bytes=100)
    with pytest.raises(ValueError, match="metric"):
        ops.pos_knn_torch(x, 3, 'cosine')
    with pytest.raises(ValueError, match="exceeds"):
        ops.pos_knn_torch(x, 64, 'euclid')
    with pytest.raises(NotImplementedError):
        ops.pair_quantile_torch(torch.stack([x, x]), 0.5, 'euclid')
    with pytest.raises(TypeError, match="float32"):
        ops.pos_knn(x.double(), 3, 'euclid')
    with pytest.raises(RuntimeError, match="device"):                 # the product path takes device tensors only
        ops.pos_knn(x, 3, 'euclid')


def test_hyperbolize_and_masked_rows():
    x = PO.points("rim")
    D = hyperbolize(torch.tensor(x))
    want = PO.distances(x, 'poincare')
    assert D.dtype == torch.float32 and tuple(D.shape) == (1, 165, 165)
    fin = np.isfinite(want)
    assert (np.abs(D[0].double().numpy() - want)[fin] <= 1e-5 * np.maximum(want[fin], 1e-3)).all()
    # a non-finite row is masked: never a neighbour, returns itself; the origin is a candidate
    y = x.copy()
    y[5, 2] = np.nan
    idx, n_valid = ops.pos_knn_torch(torch.tensor(y), 4, 'poincare')
    assert n_valid.tolist() == [164] and (idx[0, 5] == 5).all() and not (idx[0, np.arange(165) != 5] == 5).any()
    assert (idx[0] == 100).any() and idx[0, 100, 0] == 100             # the all-zero row


def _opt(**kw):
    opt = {'pos_enc_type': 'HYPS16', 'gdc_sparsification': 'topk', 'gdc_k': 16, 'pos_dist_quantile': 0.01,
           'dataset': 'Cora', 'rewiring': 'pos_enc_knn'}
    opt.update(kw)
    return opt


def _data(N, batched=False):
    d = GraphData()
    ei = torch.zeros(2, 5, dtype=torch.int64)
    d.new_graph(ei.unsqueeze(0) if batched else ei, N, torch.ones(1, 5) if batched else torch.ones(5))
    return d


def test_apply_pos_dist_rewire_torch_backend():
    x = PO.points("hyps16")
    N, C, k, _ = PO.SHAPES["hyps16"]
    tx = torch.tensor(x)
    for typ, metric in (("HYPS16", "poincare"), ("DW64", "euclid")):
        _, u, tm = PO.fixture("hyps16", metric)
        for batched in (False, True):
            d = apply_pos_dist_rewire(_data(N, batched), _opt(pos_enc_type=typ), tx.unsqueeze(0) if batched else tx,
                                      backend=BE)
            assert d.edge_index.dtype == torch.int64 and d.edge_attr is None
            assert tuple(d.edge_index.shape) == ((1, 2, N * k) if batched else (2, N * k))
            ei = d.edge_index.reshape(2, -1).numpy()
            assert np.array_equal(ei[0], np.repeat(np.arange(N), k))
            PO.check_knn(u, tm, k, ei[1].reshape(N, k), "rewire topk %s" % typ)
        # threshold: HYP reads pos_dist_quantile, DW takes apply_dist_threshold's default of 1/1000
        d = apply_pos_dist_rewire(_data(N), _opt(pos_enc_type=typ, gdc_sparsification='threshold'), tx, backend=BE)
        q = 0.01 if metric == "poincare" else 0.001
        want = PO.threshold_edges(u, q, metric)
        PO.check_edges(u, tm, PO.quantile_threshold(u, q, metric)[1], d.edge_index.numpy(), "rewire thr %s" % typ)
        assert d.edge_index.shape[1] == want.shape[1] and (metric == "poincare" or want.shape[1] == N)
    # the helpers: [B, 2, E], src = row
    e = apply_feat_KNN(tx, 5, backend=BE)
    assert tuple(e.shape) == (1, 2, N * 5) and np.array_equal(e[0, 0].numpy(), np.repeat(np.arange(N), 5))
    assert torch.equal(e, apply_dist_KNN(tx, 5, 'euclid', backend=BE))
    e2 = apply_dist_KNN(torch.stack([tx, tx.flip(0)]), 5, backend=BE)
    assert tuple(e2.shape) == (2, 2, N * 5)
    t = apply_dist_threshold(tx, backend=BE)
    assert tuple(t.shape) == (1, 2, N) and (t[0, 0] == t[0, 1]).all()    # 1/1000 of 165^2 lies inside the diagonal


def test_apply_pos_dist_rewire_raises():
    x = torch.tensor(PO.points("hyps16"))
    N = 165
    with pytest.raises(ValueError, match="pos_enc_type"):
        apply_pos_dist_rewire(_data(N), _opt(pos_enc_type='GDC'), x, backend=BE)
    with pytest.raises(ValueError, match="gdc_sparsification"):
        apply_pos_dist_rewire(_data(N), _opt(gdc_sparsification='none'), x, backend=BE)
    with pytest.raises(ValueError, match="gdc_k"):
        apply_pos_dist_rewire(_data(N), _opt(gdc_k=65), x, backend=BE)
    with pytest.raises(ValueError, match="gdc_k"):
        apply_pos_dist_rewire(_data(N), _opt(gdc_k=0), x, backend=BE)
    with pytest.raises(ValueError, match="exceeds"):
        apply_pos_dist_rewire(_data(N), _opt(gdc_k=64), x[:40], backend=BE)
    with pytest.raises(NotImplementedError):
        apply_pos_dist_rewire(_data(N, True), _opt(gdc_sparsification='threshold'), torch.stack([x, x]), backend=BE)
    for q in (-0.1, 1.5):
        with pytest.raises(ValueError, match="outside"):
            apply_pos_dist_rewire(_data(N), _opt(gdc_sparsification='threshold', pos_dist_quantile=q), x, backend=BE)
    bad = x.clone()
    bad[3, 1] = float("inf")
    with pytest.raises(ValueError, match="non-finite"):
        apply_pos_dist_rewire(_data(N), _opt(), bad, backend=BE)
    with pytest.raises(ValueError, match="non-finite"):
        apply_pos_dist_rewire(_data(N), _opt(gdc_sparsification='threshold'), bad, backend=BE)
    with pytest.raises(ValueError, match="unbatched"):
        apply_pos_dist_rewire(_data(N), _opt(), torch.stack([x, x]), backend=BE)


def test_edge_limit_constant():
    """E >= 2^31 * 16 is refused (tests/test_gpu_posdist.py lowers the limit to see it raise before the fill)."""
    assert ops.POSDIST_MAX_EDGES == (1 << 31) * 16


def test_abi_host_validation():
    """Every new entry point validates on the host before any launch: no device is touched."""
    vp = None
    E, P = _lib.METRIC_EUCLID, _lib.METRIC_POINCARE
    knn = lambda B, N, C, ld, k, m: _lib.call_rc("gnpde_pos_knn_f32", vp, B, N, C, ld, k, m, vp, vp, vp, vp, vp)  # noqa: E731
    assert knn(1, 100, 8, 8, 0, E) == _lib.EINVAL and b"k=0" in _lib.load().gnpde_last_error()
    assert knn(1, 100, 0, 8, 4, E) == _lib.EINVAL
    assert knn(1, 100, 9, 8, 4, P) == _lib.EINVAL
    assert knn(1, 100, 8, 8, 4, 2) == _lib.EINVAL and b"metric" in _lib.load().gnpde_last_error()
    assert knn(1, 100, 8, 8, 4, P) == _lib.EINVAL and b"NULL" in _lib.load().gnpde_last_error()
    assert knn(70000, 100, 8, 8, 4, P) == _lib.EINVAL
    assert knn(0, 100, 8, 8, 4, P) == _lib.OK                            # no rows: nothing to do
    sel = lambda N, C, ld, m, rank: _lib.call_rc("gnpde_pair_select_f32", vp, N, C, ld, m, rank, vp, vp, vp, 0, vp)  # noqa: E731
    assert sel(100, 8, 8, E, 5) == _lib.EINVAL and b"NULL" in _lib.load().gnpde_last_error()
    assert sel(100, 9, 8, E, 5) == _lib.EINVAL
    assert sel(100, 8, 8, 7, 5) == _lib.EINVAL and b"metric" in _lib.load().gnpde_last_error()
    assert sel((1 << 24) + 1, 8, 8, E, 5) == _lib.EUNSUPPORTED and b"range" in _lib.load().gnpde_last_error()
    assert sel(0, 8, 8, E, 0) == _lib.EINVAL                             # no entries: no rank to select
    assert sel(-1, 8, 8, E, 0) == _lib.EINVAL
    import ctypes
    buf = ctypes.create_string_buffer(1 << 16)                           # host memory: validation only, nothing launched
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert _lib.call_rc("gnpde_pos_knn_f32", p, 1, 100, 8, 8, 65, P, p, p, p, p, vp) == _lib.EUNSUPPORTED
    assert b"k=65" in _lib.load().gnpde_last_error()
    sel2 = lambda N, rank, ws: _lib.call_rc("gnpde_pair_select_f32", p, N, 8, 8, E, rank, p, p, p, ws, vp)  # noqa: E731
    assert sel2(100, 10000, 1 << 15) == _lib.EINVAL and b"rank" in _lib.load().gnpde_last_error()
    assert sel2(100, -1, 1 << 15) == _lib.EINVAL
    assert sel2(100, 5, 64) == _lib.EINVAL and b"workspace" in _lib.load().gnpde_last_error()
    cnt = lambda N, C, ld, m: _lib.call_rc("gnpde_pair_threshold_count_f32", vp, N, C, ld, m, vp, vp, vp, 0, vp)  # noqa: E731
    assert cnt(100, 8, 8, P) == _lib.EINVAL and cnt(100, 0, 8, P) == _lib.EINVAL and cnt(100, 8, 8, 3) == _lib.EINVAL
    assert cnt((1 << 24) + 1, 8, 8, P) == _lib.EUNSUPPORTED
    assert cnt(0, 8, 8, P) == _lib.OK
    fill = lambda N, C, ld, m, E_: _lib.call_rc("gnpde_pair_threshold_fill_f32", vp, N, C, ld, m, vp, vp, E_, vp, vp, 0,  # noqa: E731
                                                vp)
    assert fill(100, 8, 8, P, 10) == _lib.EINVAL and fill(100, 8, 4, P, 10) == _lib.EINVAL
    assert fill(0, 8, 8, P, 0) == _lib.OK
    fill2 = lambda E_: _lib.call_rc("gnpde_pair_threshold_fill_f32", p, 100, 8, 8, P, p, p, E_, p, p, 1 << 15, vp)  # noqa: E731
    assert fill2(10001) == _lib.EINVAL and b"E=" in _lib.load().gnpde_last_error()
    assert fill2(-1) == _lib.EINVAL
    assert fill2(0) == _lib.OK                                           # no edges: nothing launched


@pytest.mark.parametrize("N", [169343, 1 << 20])
def test_workspace_is_linear_in_n(N):
    """At most 64 bytes per row plus 1 MiB; nothing of size N^2 / tile."""
    bound = 64 * N + (1 << 20)
    pair = _lib.fn("gnpde_pair_workspace_bytes")(N)
    knn = _lib.fn("gnpde_pos_knn_workspace_bytes")(1, N)
    assert 4 * N <= pair <= bound and 5 * N <= knn <= bound
    assert _lib.fn("gnpde_pos_knn_workspace_bytes")(3, N) <= 3 * bound
    assert _lib.fn("gnpde_pos_knn_workspace_bytes")(0, N) == 16
