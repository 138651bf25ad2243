"""GDC rewiring on the GPU: the column top-k kernel (csrc/topk_cols.hip) against numpy, the
diffusion blocks on K1 and the whole driver against the float64 oracle (tests/gdc_oracle.py),
and the rewired graph through the existing ODE block.

Bounds.  Values: 1e-5 of the column's maximum (the project's parity bar at the column's
scale); the schedules truncate at 1e-6 alpha (ppr) / 1e-6 e^-t (heat) of it.  Selection: the
boundary rule of gdc_oracle.check on every column, the exact set on the decided ones."""
import numpy as np
import pytest
import torch

import gdc_oracle as KO
import gnpde
import gnpde_oracle as O
from gnpde import ops
from test_gdc_host import FIXTURES, _check_threshold, _data, _kw, _opt
from test_gpu_parity import OPT as BASE_OPT, RTOL, T, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _block(N, ncols, ld, seed):
    """Finite values of either sign, zeros, and 30 % exact duplicates."""
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((N, ld)).astype(np.float32)
    y[rng.random(y.shape) < 0.1] = 0.0
    dup = rng.random(y.shape) < 0.3
    y[dup] = rng.choice(np.array([-1.5, -0.25, 0.0, 0.5, 0.75, 2.0], np.float32), size=int(dup.sum()))
    return y


def _want(y, ncols, k):
    idx, val = KO.topk(y[:, :ncols].astype(np.float64), k)
    val = val.astype(np.float32)
    s = np.zeros(ncols, np.float32)
    for i in range(k):
        s = s + val[:, i]                                  # sequential, rank order, fp32
    with np.errstate(divide="ignore", invalid="ignore"):
        wn = np.where(s[:, None] == 0, np.float32(0), val / s[:, None])
    return idx, val, wn.astype(np.float32)


@pytest.mark.parametrize("N,ncols,k,ld,rows", [(100, 100, 100, 100, None), (777, 9, 1, 128, None),
                                               (777, 128, 128, 128, None), (777, 128, 128, 128, 64),
                                               (5000, 128, 64, 128, None), (5000, 128, 64, 128, 448),
                                               (5000, 128, 64, 128, 1024)])
def test_topk_cols_vs_numpy(N, ncols, k, ld, rows):
    y = _block(N, ncols, ld, 7)
    idx, val, wn = ops.topk_cols(T(y), k, ncols=ncols, rows_per_wg=rows)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (ncols, k)
    widx, wval, wwn = _want(y, ncols, k)
    assert np.array_equal(idx.cpu().numpy(), widx)         # ties: (value desc, row asc)
    assert np.array_equal(val.cpu().numpy(), wval)
    assert np.array_equal(wn.cpu().numpy().view(np.int32), wwn.view(np.int32))
    idx2, val2, wn2 = ops.topk_cols(T(y), k, ncols=ncols, rows_per_wg=rows)
    assert torch.equal(idx, idx2) and torch.equal(val, val2) and torch.equal(wn, wn2)
    ti, tv, tw = ops.topk_cols_torch(T(y), k, ncols=ncols)
    assert torch.equal(idx, ti) and torch.equal(val, tv)
    assert bool(((wn - tw).abs() <= 2.0 ** -23 * wn.abs()).all())     # (the device's division may round otherwise)


def test_topk_cols_partition_independent():
    y = T(_block(5000, 128, 128, 11))
    a = ops.topk_cols(y, 64, rows_per_wg=None)
    for rows in (64, 1024, 5000):
        b = ops.topk_cols(y, 64, rows_per_wg=rows)
        assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_topk_cols_errors():
    y = T(_block(100, 16, 16, 3))
    with pytest.raises(ValueError, match="exceeds"):
        ops.topk_cols(y, 101)
    with pytest.raises(ops._lib.GnpdeError, match="range"):
        ops.topk_cols(T(_block(200, 16, 16, 3)), 129)
    with pytest.raises(RuntimeError):
        ops.topk_cols(y.cpu(), 4)


def _prepared(name):
    ei, N, k, _ = KO.fixture(name, "ppr", 0.05)
    row, col, val = ops.gdc_matrix(T(ei), None, N, 1.0)
    e = torch.stack([row, col]).unsqueeze(0).contiguous()
    tw = ops.norm_weights(e, val.unsqueeze(0).contiguous(), N, ops._lib.NORM_GCN)
    g = ops.GraphCSR(e, N)
    return g, g.gather_weights(tw), N


@pytest.mark.parametrize("name,blocks,seeds", [("small", [(0, 128), (256, 44)], ("operand", "diagonal")),
                                               ("wide", [(256, 128), (768, 9)], ("operand",))])
@pytest.mark.parametrize("method,p", [("ppr", 0.05), ("ppr", 0.15), ("heat", 3.0)])
def test_diffusion_block_vs_oracle(name, blocks, seeds, method, p):
    g, w, N = _prepared(name)
    S = KO.fixture(name, method, p)[3].S
    sched = ops.diffusion_schedule(**_kw(method, p))
    for j0, nc in blocks:
        for seed in seeds:
            Y = ops.diffusion_block(g, w, j0, nc, sched, seed=seed)
            assert tuple(Y.shape) == (N, nc)
            want = S[:, j0:j0 + nc]
            err = (np.abs(Y.double().cpu().numpy() - want) / want.max(0)).max()
            print("diffusion_block %s %s %g [%d, +%d) %s: max err / column max %.3e" % (name, method, p, j0, nc,
                                                                                       seed, err))
            assert err <= KO.BAR


@pytest.mark.parametrize("name,method,p", FIXTURES)
def test_gdc_vs_oracle(name, method, p):
    ei, N, k, res = KO.fixture(name, method, p)
    e, w = ops.gdc(T(ei), None, N, k=k, **_kw(method, p))
    assert e.dtype == torch.int64 and w.dtype == torch.float32 and tuple(e.shape) == (2, N * k)
    assert (np.diff(e[0].cpu().numpy() * N + e[1].cpu().numpy()) > 0).all()
    KO.check_edges(res, e.cpu().numpy(), w.cpu().numpy(), N, k)
    e2, w2 = ops.gdc(T(ei), None, N, k=k, **_kw(method, p))
    assert torch.equal(e, e2) and torch.equal(w, w2)                      # the same bits on every call


def _column_values(res, e, w, N, k):
    """The kept values of a rewired edge list as a dense [N, N] array (NaN where not kept): the
    column normalisation undone with the oracle's kept sum of the list's own index set."""
    idx, wn = KO.edges_to_columns(e.cpu().numpy(), w.cpu().numpy(), N, k)
    cols = np.arange(N)[:, None]
    V = np.full((N, N), np.nan)
    V[idx, cols] = wn.astype(np.float64) * res.S[idx, cols].sum(1, keepdims=True)
    return V


@pytest.mark.parametrize("name,method,p", FIXTURES)
def test_gdc_vs_gdc_torch_on_device(name, method, p):
    """ops.gdc against its torch restatement on the same device, within the value bar tau_j =
    1e-5 max_i S[i, j] itself: every entry of the unsparsified matrix (dense=True), and every
    entry both top-k lists keep; an entry only one of them keeps is held to the boundary rule,
    and on decided columns both keep the oracle's set (check_edges)."""
    ei, N, k, res = KO.fixture(name, method, p)
    Pg = ops.gdc(T(ei), None, N, dense=True, **_kw(method, p)).double().cpu().numpy()
    Pt = ops.gdc_torch(T(ei), None, N, dense=True, **_kw(method, p)).double().cpu().numpy()
    err = np.abs(Pg - Pt) * res.S.sum(0) / res.tau
    print("gdc vs gdc_torch %s %s %g: dense max |diff| / tau = %.3f" % (name, method, p, err.max()))
    assert err.max() <= 1.0
    e, w = ops.gdc(T(ei), None, N, k=k, **_kw(method, p))
    et, wt = ops.gdc_torch(T(ei), None, N, k=k, **_kw(method, p))
    KO.check_edges(res, e.cpu().numpy(), w.cpu().numpy(), N, k)
    KO.check_edges(res, et.cpu().numpy(), wt.cpu().numpy(), N, k)
    A, B = _column_values(res, e, w, N, k), _column_values(res, et, wt, N, k)
    both = ~np.isnan(A) & ~np.isnan(B)
    err = np.where(both, np.abs(A - B), 0.0) / res.tau
    print("gdc vs gdc_torch %s %s %g: top-k max |diff| / tau = %.3f on %d shared of %d entries" % (
        name, method, p, err.max(), both.sum(), N * k))
    assert err.max() <= 1.0
    d = res.decided
    assert np.array_equal(np.isnan(A)[:, d], np.isnan(B)[:, d])


def _device_data(ei, N, batched=False):
    d = _data(ei, N, batched=batched)
    d.edge_index = d.edge_index.to(DEV)
    return d


@pytest.mark.parametrize("name,method,p", FIXTURES)
def test_apply_gdc_on_device(name, method, p):
    """apply_gdc with the device driver on every fixture: the option mapping (ppr_alpha, the heat
    fallback of any other gdc_method, gdc_k up to 128) into the kernels."""
    ei, N, k, res = KO.fixture(name, method, p)
    opt = _opt(gdc_k=k, ppr_alpha=p) if method == "ppr" else _opt(gdc_k=k, gdc_method='coeff', heat_time=p)
    for batched in (False, True):
        d = gnpde.apply_gdc(_device_data(ei, N, batched), opt)
        assert d.edge_index.is_cuda and tuple(d.edge_index.shape) == ((1, 2, N * k) if batched else (2, N * k))
        assert tuple(d.edge_attr.shape) == ((1, N * k) if batched else (N * k,))
        KO.check_edges(res, d.edge_index.reshape(2, -1).cpu().numpy(), d.edge_attr.reshape(-1).cpu().numpy(), N, k)


def test_gdc_errors_on_device():
    ei, N, k, _ = KO.fixture("small", "ppr", 0.05)
    with pytest.raises(ValueError, match="to_undirected"):
        ops.gdc(T(ei[:, :-1]), None, N, k=4)
    with pytest.raises(ValueError, match="range"):
        ops.gdc(T(KO.fixture("k128")[0]), None, 200, k=129)


@pytest.mark.parametrize("method,p", [("ppr", 0.05), ("heat", 3.0)])
def test_gdc_default_seed_of_large_graphs(method, p, monkeypatch):
    """From GDC_DIAGONAL_MIN_ROWS rows on the driver's default adds the seed term to the block's
    diagonal; with the limit lowered the same default path runs end to end on a fixture."""
    ei, N, k, res = KO.fixture("wide", method, p)
    a = ops.gdc(T(ei), None, N, k=k, seed='diagonal', **_kw(method, p))
    monkeypatch.setattr(ops, "GDC_DIAGONAL_MIN_ROWS", N)
    e, w = ops.gdc(T(ei), None, N, k=k, **_kw(method, p))
    KO.check_edges(res, e.cpu().numpy(), w.cpu().numpy(), N, k)
    assert torch.equal(e, a[0]) and torch.equal(w, a[1])                 # the default took the diagonal path
    monkeypatch.setattr(ops, "GDC_DIAGONAL_MIN_ROWS", N + 1)
    b = ops.gdc(T(ei), None, N, k=k, **_kw(method, p))
    c = ops.gdc(T(ei), None, N, k=k, seed='operand', **_kw(method, p))
    assert torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])          # below the limit: the operand path


@pytest.mark.parametrize("method,p,thr", [("ppr", 0.05, 0.01), ("heat", 3.0, 0.02)])
def test_gdc_threshold(method, p, thr):
    ei, N, k, res = KO.fixture("small", method, p)
    e, w = ops.gdc(T(ei), None, N, sparsification='threshold', threshold=thr, **_kw(method, p))
    _check_threshold(res, e.cpu().numpy(), w.cpu().numpy(), thr)
    e2, w2 = ops.gdc(T(ei), None, N, sparsification='threshold', threshold=thr, **_kw(method, p))
    assert torch.equal(e, e2) and torch.equal(w, w2)


def test_pos_encoding_on_device():
    ei, N, k, res = KO.fixture("small", "ppr", 0.05)
    Sn = res.S / res.S.sum(0)
    enc = {}
    for o in ("row", "col"):
        d = _data(ei, N)
        d.edge_index = d.edge_index.to(DEV)
        enc[o] = gnpde.apply_gdc(d, _opt(pos_enc_orientation=o), type='pos_encoding')
        assert tuple(enc[o].shape) == (N, N) and enc[o].dtype == torch.float32
    assert torch.equal(enc["row"].T, enc["col"])
    err = np.abs(enc["row"].double().cpu().numpy() - Sn) / Sn.max(0)
    assert err.max() <= KO.BAR
    with pytest.raises(ValueError, match="max_bytes"):
        ops.gdc(T(ei), None, N, dense=True, max_bytes=1000)


def test_rewired_graph_through_the_ode_block():
    """The rewired graph, with its weights, is a graph the rest of the stack accepts."""
    ei, N, k, _ = KO.fixture("small", "ppr", 0.05)
    C = 16
    e, w = ops.gdc(T(ei), None, N, k=k)
    x = np.random.default_rng(5).standard_normal((1, N, C)).astype(np.float32)
    opt = dict(BASE_OPT, hidden_dim=C, method='rk4', step_size=0.25, data_norm='rw', self_loop_weight=1.0)
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.6)
    data = gnpde.GraphData()
    data.new_graph(e.unsqueeze(0), N, edge_attr=w.unsqueeze(0))
    with torch.no_grad():
        z = blk(T(x), data)
    en, wn = e.unsqueeze(0).cpu().numpy(), w.unsqueeze(0).cpu().numpy()
    eis, ws = O.get_rw_adj(en, edge_weight=wn, norm_dim=1, fill_value=1.0, num_nodes=N)
    eo, wo = np.stack(eis, 0), np.stack(ws, 0)
    f = lambda t, y: O.laplacian_rhs(eo, y, None, 0.6, 0.0, edge_weight=wo)  # noqa: E731
    assert rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.25)) <= RTOL
