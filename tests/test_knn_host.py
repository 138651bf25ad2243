"""Host: the kNN rewiring's oracle, its torch restatement (ops.knn_torch) and the
gnpde.graph_rewiring plumbing, on CPU tensors (no GPU: the search is injected)."""
import numpy as np
import pytest
import torch

import knn_oracle as KO
from gnpde import graph_rewiring, ops
from gnpde.graph_rewiring import KNN, apply_KNN


def _opt(k, sym=False, T='raw'):
    return {'rewire_KNN_k': k, 'rewire_KNN_sym': sym, 'rewire_KNN_T': T, 'rewire_KNN_epoch': 5}


def test_oracle_matches_sklearn_brute():
    """sklearn.neighbors is what the reference's own distances_kNN.apply_feat_KNN uses."""
    nb = pytest.importorskip("sklearn.neighbors")
    x, res = KO.fixture("tails")  # tie-free: all strict
    assert KO.strict_share(res) == 1.0
    N, C, k = KO.SHAPES["tails"]
    dist, ind = nb.NearestNeighbors(n_neighbors=k, algorithm='brute').fit(x.astype(np.float64)).kneighbors(
        x.astype(np.float64))
    assert np.array_equal(ind, res.idx[0])
    assert np.allclose(dist ** 2, res.dist[0], rtol=1e-9, atol=1e-12)


def test_oracle_ties_take_the_lower_index():
    x, res = KO.ties_fixture()
    # a duplicated row and its original are at distance 0 of each other: the lower index first
    src = int(np.flatnonzero((x[:560] == x[560]).all(1))[0])
    assert res.dist[0][560, 0] == 0.0 and res.idx[0][560, 0] == src
    d = res.dist[0]
    assert (d[:, 1:] >= d[:, :-1]).all()
    tie = d[:, 1:] == d[:, :-1]
    assert tie.any() and (res.idx[0][:, 1:][tie] > res.idx[0][:, :-1][tie]).all()


@pytest.mark.parametrize("name", ["k_eq_n", "tails", "k1", "clustered", "cora_width"])
def test_knn_torch_vs_oracle(name):
    x, res = KO.fixture(name)
    k = KO.SHAPES[name][2]
    strict = name in KO.STRICT
    if strict:
        assert KO.strict_share(res) >= 0.9
    idx, dist, n_valid = ops.knn_torch(torch.tensor(x), k, return_dist=True)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (1,) + x.shape[:1] + (k,)
    assert n_valid.tolist() == res.n_valid.tolist()
    KO.check(res, idx.numpy(), strict=strict)
    want = res.dist[0]
    assert np.abs(dist[0].double().numpy() - want).max() <= KO.tau(x.shape[1]) * want.max()


def test_knn_torch_exact_ties():
    x, res = KO.ties_fixture()
    idx, dist, _ = ops.knn_torch(torch.tensor(x), 16, return_dist=True)
    assert np.array_equal(idx.numpy().astype(np.int64), res.idx)
    assert np.array_equal(dist.numpy(), res.dist.astype(np.float32))


def test_knn_torch_batch_and_masks():
    x, res = KO.batch_fixture()
    idx, n_valid = ops.knn_torch(torch.tensor(x), 8)
    assert n_valid.tolist() == res.n_valid.tolist() == [300, 300 - 17 - 1, 150]
    KO.check(res, idx.numpy(), strict=True)


def test_KNN_shape_dtype_and_rows():
    x, res = KO.fixture("tails")
    N, C, k = KO.SHAPES["tails"]
    for xin in (torch.tensor(x), torch.tensor(x).unsqueeze(0)):
        ei = KNN(xin, _opt(k), knn=ops.knn_torch)
        assert ei.dtype == torch.int64 and tuple(ei.shape) == (1, 2, N * k)
        assert np.array_equal(ei[0, 0].numpy(), np.repeat(np.arange(N), k))
        assert np.array_equal(ei.numpy(), KO.edge_index(res.idx))


def test_KNN_batch_masked_rows():
    x, res = KO.batch_fixture()
    ei = KNN(torch.tensor(x), _opt(8), knn=ops.knn_torch).numpy()
    assert ei.shape == (3, 2, 300 * 8)
    want = KO.edge_index(res.idx)
    assert np.array_equal(ei[:, 0], want[:, 0])
    nb = ei[:, 1].reshape(3, 300, 8)
    for b in range(3):
        m = res.masked[b]
        assert (nb[b][m] == np.arange(300)[m, None]).all()    # masked queries: themselves
        assert not m[nb[b][~m]].any()                          # never a neighbour
    KO.check(res, nb, strict=True)


def test_KNN_sym_is_to_undirected_at_b1_and_raises_at_b2():
    x, res = KO.fixture("tails")
    N, C, k = KO.SHAPES["tails"]
    ei = KNN(torch.tensor(x), _opt(k, sym=True), knn=ops.knn_torch)
    want = KO.to_undirected(KO.edge_index(res.idx)[0], N)
    assert ei.dtype == torch.int64 and np.array_equal(ei.numpy(), want[None])
    with pytest.raises(NotImplementedError):
        KNN(torch.from_numpy(np.stack([x, x])), _opt(k, sym=True), knn=ops.knn_torch)


def test_KNN_k_above_the_valid_count_raises():
    x, _ = KO.batch_fixture()  # graph 2 has 150 unmasked rows
    xt = torch.tensor(x)
    KNN(xt, _opt(150), knn=ops.knn_torch)
    with pytest.raises(ValueError, match="unmasked"):
        KNN(xt, _opt(151), knn=ops.knn_torch)
    with pytest.raises(ValueError):
        KNN(xt, _opt(301), knn=ops.knn_torch)


def test_product_path_refuses_cpu_and_bf16():
    x = torch.tensor(KO.fixture("tails")[0])
    with pytest.raises(RuntimeError, match="ROCm device"):
        KNN(x, _opt(7))
    with pytest.raises(TypeError, match="float32"):
        KNN(x.to(torch.bfloat16), _opt(7))


class _Stub(object):
    """forward_encoder doubles the features' first column block, forward_ODE negates and shifts:
    three different inputs to the search."""

    def __init__(self):
        self.calls = []

    def forward_encoder(self, x, pos_encoding):
        self.calls.append(("enc", pos_encoding))
        return x[..., :3] * 2.0

    def forward_ODE(self, x, graph_data, pos_encoding, x2):
        self.calls.append(("ode", graph_data, pos_encoding, x2))
        return torch.flip(x, dims=[-1])[..., :4] + 1.0


def test_apply_KNN_dispatch(monkeypatch):
    monkeypatch.setattr(graph_rewiring.ops, "knn", ops.knn_torch)
    x = torch.tensor(KO.fixture("tails")[0]).unsqueeze(0)
    k = 7
    model = _Stub()
    want = {
        'raw': x,
        'T0': x[..., :3] * 2.0,
        'TN': torch.flip(x, dims=[-1])[..., :4] + 1.0,
    }
    for T, feats in want.items():
        ei = apply_KNN(x, "graph", "x2", "pos", model, _opt(k, T=T))
        assert np.array_equal(ei.numpy(), KO.edge_index(KO.knn(feats.numpy(), k).idx)), T
    assert model.calls == [("enc", "pos"), ("ode", "graph", "pos", "x2")]
    with pytest.raises(Exception, match="rewire_KNN_T"):
        apply_KNN(x, "graph", "x2", "pos", model, _opt(k, T='T7'))
