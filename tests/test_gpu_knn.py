"""GPU: the exact top-k kernel (csrc/knn.hip through ops.knn) and the kNN rewiring on the
device, against the float64 oracle of tests/knn_oracle.py.

Acceptance (knn_oracle.check): (a) distinct, in-range, unmasked indices; (b) position by
position |D[j_m] - D_(m)| <= tau D_(m) with tau = 2 (C + 3) 2^-24 (two fp32 difference-form
distances compared, each within (C + 3) 2^-24 of the exact value); (c) exact indices on
the oracle's strict rows, on the fixtures whose strict share the test itself finds >= 0.9.
The shapes are the smallest at which the kernel can go wrong: k = N inside one partial
tile, tile tails and odd C, k = 1, more than one query tile and many candidate tiles at
BLEND's width, and near neighbours with small d / |x|^2."""
import ctypes

import numpy as np
import pytest
import torch

import gnpde
import gnpde_oracle as O
import knn_oracle as KO
from gnpde import _lib, ops
from gnpde.graph_rewiring import KNN
from test_gpu_parity import DEV, OPT, RTOL, T, _prep_oracle, rel

pytestmark = pytest.mark.gpu


def _opt(k, sym=False):
    return {'rewire_KNN_k': k, 'rewire_KNN_sym': sym, 'rewire_KNN_T': 'raw'}


@pytest.mark.parametrize("name", ["k_eq_n", "tails", "k1", "cora_width", "clustered", "blend_width"])
def test_knn_vs_oracle(name):
    x, res = KO.fixture(name)
    N, C, k = KO.SHAPES[name]
    strict = name in KO.STRICT
    if strict:
        assert KO.strict_share(res) >= 0.9
    idx, dist, n_valid = ops.knn(T(x), k, return_dist=True)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1, N, k)
    assert n_valid.dtype == torch.int32 and n_valid.tolist() == [N]
    KO.check(res, idx.cpu().numpy(), strict=strict)
    # the distances are those of the returned indices, each within (C + 3) 2^-24 of the exact value
    Dg = np.take_along_axis(res.D[0], idx[0].cpu().numpy().astype(np.int64), 1)
    assert (np.abs(dist[0].double().cpu().numpy() - Dg) <= 0.5 * KO.tau(C) * Dg).all()


def test_k_above_n_raises():
    x = np.random.default_rng(1).standard_normal((63, 4)).astype(np.float32)
    with pytest.raises(ValueError):
        ops.knn(T(x), 64)
    with pytest.raises(ValueError):
        KNN(T(x), _opt(64))


def test_exact_ties_bitwise():
    x, res = KO.ties_fixture()
    idx, dist, _ = ops.knn(T(x), 16, return_dist=True)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), res.idx)
    assert np.array_equal(dist.cpu().numpy(), res.dist.astype(np.float32))


def test_batch_and_masking():
    x, res = KO.batch_fixture()
    B, N, k = 3, 300, 8
    idx, n_valid = ops.knn(T(x), k)
    assert n_valid.tolist() == res.n_valid.tolist() == [300, 282, 150]
    got = idx.cpu().numpy()
    assert got.min() >= 0 and got.max() < N  # each graph's neighbours in its own index range
    for b in range(B):
        m = res.masked[b]
        assert (got[b][m] == np.arange(N)[m, None]).all()
        assert not m[got[b][~m]].any()
    KO.check(res, got, strict=True)
    # no leakage: graph b alone gives the same rows
    for b in range(B):
        assert torch.equal(ops.knn(T(x[b]), k)[0][0], idx[b])
    with pytest.raises(ValueError, match="unmasked"):
        KNN(T(x), _opt(151))


def test_strided_no_dist_and_determinism():
    N, C, k = KO.SHAPES["k1"][0], 33, 9
    rng = np.random.default_rng(5)
    buf = rng.standard_normal((N, 40)).astype(np.float32)
    res = KO.knn(buf[:, :C], k)
    tb = T(buf)
    idx, n_valid = ops.knn_strided(tb, C, k)  # dist_out = NULL
    KO.check(res, idx.cpu().numpy(), strict=KO.strict_share(res) >= 0.9)
    idx_c, dist_c, _ = ops.knn(tb[:, :C], k, return_dist=True)  # the .contiguous() path
    idx_s, dist_s, _ = ops.knn_strided(tb, C, k, return_dist=True)
    assert torch.equal(idx, idx_c) and torch.equal(idx, idx_s) and torch.equal(dist_c, dist_s)
    again = ops.knn_strided(tb, C, k, return_dist=True)
    assert torch.equal(again[0], idx_s) and torch.equal(again[1], dist_s)


def test_abi_errors():
    lib = _lib.load()
    vp = ctypes.c_void_p
    p = vp(4096)  # validation happens on the host, before any launch
    assert lib.gnpde_knn_f32(p, 1, 100, 8, 8, 0, p, p, p, p, vp(0)) == -1 and b"k=0" in lib.gnpde_last_error()
    assert lib.gnpde_knn_f32(p, 1, 100, 0, 8, 4, p, p, p, p, vp(0)) == -1 and b"C=0" in lib.gnpde_last_error()
    assert lib.gnpde_knn_f32(p, 1, 100, 9, 8, 4, p, p, p, p, vp(0)) == -1
    assert lib.gnpde_knn_f32(p, 1, 100, 8, 8, 4, vp(0), p, vp(0), p, vp(0)) == -1
    assert b"NULL" in lib.gnpde_last_error()
    assert lib.gnpde_knn_f32(p, 1, 100, 8, 8, 65, p, p, p, p, vp(0)) == -3
    assert b"k=65" in lib.gnpde_last_error() and b"range" in lib.gnpde_last_error()
    assert lib.gnpde_knn_f32(vp(0), 0, 100, 8, 8, 4, vp(0), vp(0), vp(0), vp(0), vp(0)) == 0  # no rows: nothing to do
    assert lib.gnpde_knn_workspace_bytes(3, 300) >= 900
    with pytest.raises(_lib.GnpdeError, match="rc=-3"):
        _lib.call("gnpde_knn_f32", p, 1, 100, 8, 8, 65, p, p, p, p, vp(0))


def test_k_above_the_kernel_range_takes_the_torch_path():
    x, _ = KO.fixture("k1")
    x = x[:300]
    res = KO.knn(x, 65)
    idx, n_valid = ops.knn(T(x), 65)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1, 300, 65) and n_valid.tolist() == [300]
    KO.check(res, idx.cpu().numpy())


def test_KNN_on_device_and_sym():
    x, res = KO.fixture("tails")  # all strict
    N, C, k = KO.SHAPES["tails"]
    assert KO.strict_share(res) == 1.0
    idx, _ = ops.knn(T(x), k)
    ei = KNN(T(x), _opt(k))
    assert ei.dtype == torch.int64 and tuple(ei.shape) == (1, 2, N * k) and ei.is_cuda
    assert np.array_equal(ei.cpu().numpy(), KO.edge_index(idx.cpu().numpy().astype(np.int64)))
    assert np.array_equal(ei.cpu().numpy(), KO.edge_index(res.idx))
    es = KNN(T(x), _opt(k, sym=True))
    assert es.dtype == torch.int64 and es.is_cuda
    assert np.array_equal(es.cpu().numpy(), KO.to_undirected(KO.edge_index(res.idx)[0], N)[None])
    with pytest.raises(NotImplementedError):
        KNN(T(np.stack([x, x])), _opt(k, sym=True))


def test_rewired_graph_end_to_end():
    """The kNN edge_index of the embeddings drives a ConstantODEblock solve: equal to the
    oracle's solve on the oracle's kNN graph (an all-strict fixture, so the graphs agree)."""
    N, C, k = 257, 16, 7
    x = np.random.default_rng(6).standard_normal((1, N, C)).astype(np.float32)
    res = KO.knn(x, k)
    assert KO.strict_share(res) == 1.0
    ei = KNN(T(x), _opt(k))
    want_ei = KO.edge_index(res.idx)
    assert np.array_equal(ei.cpu().numpy(), want_ei)
    opt = dict(OPT, hidden_dim=C, method='euler', step_size=0.25, add_source=True)
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0, 1])).to(DEV).eval()
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.4)
        blk.odefunc.beta_train.fill_(0.3)
    data = gnpde.GraphData()
    data.new_graph(ei, N)
    blk.set_x0(T(x))
    with torch.no_grad():
        z = blk(T(x), data)
    eo, wo = _prep_oracle(want_ei, N)
    f = lambda t, y: O.laplacian_rhs(eo, y, x, 0.4, 0.3, edge_weight=wo, add_source=True)  # noqa: E731
    assert rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'euler', 0.25)) <= RTOL


def test_bf16_raises():
    x = T(KO.fixture("tails")[0])
    with pytest.raises(TypeError, match="float32"):
        ops.knn(x.to(torch.bfloat16), 7)
    with pytest.raises(TypeError, match="float32"):
        KNN(x.to(torch.bfloat16), _opt(7))
