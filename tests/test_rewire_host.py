"""Host-side checks of the rewire_attention block, on CPU: the registry switch, the
constructor contract, every raise, ops.two_hop_torch and the block's 'random' union against
the float64 oracle (tests/rewire_oracle.py), the threshold arithmetic, the conditions the
GPU tests rest on (asserted from the oracle alone), and the oracle against the recorded
output of the reference's own add_khop_edges (tests/golden/rewire)."""
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import rewire_oracle as RO
from conftest import GOLDEN
from gnpde import ops

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 6, 'block': 'rewire_attention', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': False, 'max_nfe': 1000,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16,
       'att_samp_pct': 0.5, 'new_edges': 'k_hop_att', 'sparsify': 'S_hat', 'threshold_type': 'addD_rvR',
       'rw_addD': 0.02, 'use_flux': False}

# the fixtures of the kept-set checks and the rw_addD each is thresholded with
KEPT = dict(short=0.02, directed=0.02, dups=0.02, empty=0.02, hub=0.02, wide=0.02)


def _block(func=None, **kw):
    opt = dict(OPT, **kw)
    return gnpde.RewireAttODEblock(func or gnpde.LaplacianODEFunc, [], opt, None, t=torch.tensor([0, 1]))


def test_registry_switch():
    assert gnpde.set_block(dict(OPT, block='rewire_attention', gnpde_rewire_attention=True)) is gnpde.RewireAttODEblock
    with pytest.raises(NotImplementedError, match="gnpde_rewire_attention"):
        gnpde.set_block(dict(OPT, block='rewire_attention'))
    with pytest.raises(NotImplementedError, match="gnpde_rewire_attention"):
        gnpde.set_block(dict(OPT, block='rewire_attention', gnpde_rewire_attention=False))
    from gnpde.block_transformer_rewiring import RewireAttODEblock
    assert RewireAttODEblock is gnpde.RewireAttODEblock


@pytest.mark.parametrize("function", ["laplacian", "transformer"])
def test_state_dict_keys_equal_hard_attention(function):
    func = gnpde.LaplacianODEFunc if function == 'laplacian' else gnpde.ODEFuncTransformerAtt
    opt = dict(OPT, function=function)
    blk = gnpde.RewireAttODEblock(func, [], opt, None, t=torch.tensor([0, 1]))
    hard = gnpde.HardAttODEblock(func, [], dict(opt, block='hard_attention'), None, t=torch.tensor([0, 1]))
    assert list(blk.state_dict().keys()) == list(hard.state_dict().keys())
    assert hasattr(blk, 'multihead_att_layer') == (function == 'laplacian')
    assert blk.train_integrator is gnpde.integrator.odeint and blk.test_integrator is gnpde.integrator.odeint
    assert repr(blk) == "RewireAttODEblock( Time Interval 0 -> 1)"
    for name in ('get_attention_weights', 'renormalise_attention', 'add_random_edges', 'add_khop_edges',
                 'densify_edges', 'threshold_edges', 'forward'):
        assert callable(getattr(blk, name))


def test_att_samp_pct_assertion():
    for bad in (0.0, 1.5):
        with pytest.raises(AssertionError):
            _block(att_samp_pct=bad)


def _with_graph(blk, name='toy', B=1):
    ei, w0, N = RO.prepared(name)
    e = torch.from_numpy(np.repeat(ei, B, axis=0))
    blk.num_nodes = N
    blk.data_edge_index = e
    blk.odefunc.edge_index = e
    blk.odefunc.edge_weight = torch.from_numpy(np.repeat(w0, B, axis=0))
    return blk


def test_raises():
    x = torch.zeros(1, 3, 6)
    with pytest.raises(NotImplementedError, match="B = 1"):
        _with_graph(_block(), B=2).rewire(torch.zeros(2, 3, 6))
    with pytest.raises(NotImplementedError, match="B = 1"):
        _with_graph(_block(new_edges='random'), B=2).add_random_edges()
    with pytest.raises(NotImplementedError, match="random_walk"):
        _with_graph(_block(new_edges='random_walk')).rewire(x)
    with pytest.raises(NotImplementedError, match="use_flux"):
        _with_graph(_block(use_flux=True)).threshold_edges(x, torch.zeros(1))
    # k_hop_lap is `pass`: pc_change = 0 and the quantile's q is negative
    with pytest.raises(ValueError, match=r"pc_change.*rw_addD") as ei:
        _with_graph(_block(new_edges='k_hop_lap')).rewire(x)
    assert "q =" in str(ei.value) and "-50" in str(ei.value)
    # 'random' with a small rw_addD: one pair added to 7 edges, q far above 1
    blk = _with_graph(_block(new_edges='random', rw_addD=0.3))
    with pytest.raises(ValueError, match=r"pc_change.*rw_addD"):
        blk.rewire(x, pairs=torch.tensor([[0], [0]]))
    with pytest.raises(NotImplementedError, match="k = 2"):
        _with_graph(_block()).add_khop_edges(k=3)


def test_two_hop_input_raises():
    ei, w0, N = RO.prepared('toy')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.two_hop(torch.from_numpy(ei), torch.from_numpy(w0), num_nodes=N)
    with pytest.raises(TypeError):
        ops.two_hop(torch.from_numpy(ei), torch.from_numpy(w0).double(), num_nodes=N)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.two_hop((torch.zeros(4, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)), torch.zeros(1))
    with pytest.raises(ValueError, match="2\\^31"):
        ops.two_hop_check_length(2 ** 31)
    assert ops.two_hop_check_length(2 ** 31 - 1) == 2 ** 31 - 1
    with pytest.raises(NotImplementedError, match="B = 1"):
        ops.two_hop_torch(torch.from_numpy(np.repeat(ei, 2, axis=0)), torch.from_numpy(np.repeat(w0, 2, axis=0)),
                          num_nodes=N)


@pytest.mark.parametrize("route", ["dense", "sparse"])
@pytest.mark.parametrize("name", RO.NAMES)
def test_two_hop_torch_vs_oracle(name, route):
    ei, w0, N = RO.prepared(name)
    want = RO.product(name)
    e, v, rowptr = ops.two_hop_torch(torch.from_numpy(ei), torch.from_numpy(w0), num_nodes=N,
                                     dense_n=(1 << 30) if route == 'dense' else 0)
    assert e.dtype == torch.int64 and v.dtype == torch.float32 and rowptr.dtype == torch.int32
    assert e.shape == want['edge_index'].shape and (e.numpy() == want['edge_index']).all()
    assert (rowptr.numpy() == want['rowptr']).all()
    S = want['values']
    # torch's own order of fp32 products and sums: any order of the n non-negative terms stays inside
    bound = (want['n'] + 3) * 2.0 ** -24 * S
    assert (np.abs(v.double().numpy() - S) <= bound).all()
    diag = want['edge_index'][0, 0] == want['edge_index'][0, 1]
    assert (v.numpy()[diag] == 0).all()
    # the same through a coalesced CSR with CSR-order values
    if route == 'dense' and name in ('toy', 'directed'):
        W = want['W']
        r, c = np.nonzero(W)
        rp = np.zeros(N + 1, np.int32)
        rp[1:] = np.cumsum(np.bincount(r, minlength=N))
        e2, v2, rp2 = ops.two_hop_torch((torch.from_numpy(rp), torch.from_numpy(c.astype(np.int32))),
                                        torch.from_numpy(W[r, c].astype(np.float32)))
        assert torch.equal(e2, e) and torch.equal(rp2, rowptr)
        assert (np.abs(v2.double().numpy() - S) <= bound + 2.0 ** -24 * S).all()   # W's entries rounded once more


def test_threshold_arithmetic_on_the_toy_graph():
    """The reference's toy edge list [[0,2,2,1],[1,0,1,2]] with self loops: 7 edges, every one of
    the 9 positions reachable in two hops."""
    ei, w0, N = RO.prepared('toy')
    assert N == 3 and ei.shape == (1, 2, 7)
    assert (ei[0, :, :4] == np.array([[0, 2, 2, 1], [1, 0, 1, 2]])).all() and (ei[0, 0, 4:] == ei[0, 1, 4:]).all()
    p = RO.product('toy')
    assert p['edge_index'].shape[2] == 9 and (p['rowptr'] == [0, 3, 6, 9]).all()
    assert (p['values'][[0, 4, 8]] == 0).all() and (np.delete(p['values'], [0, 4, 8]) > 0).all()
    # pc_change = 9 / 7 - 1; rw_addD = 0.02 gives q = 3.76: the usual outcome on a graph this dense
    with pytest.raises(ValueError):
        RO.threshold(w0, 7, 9, 0.02)
    pc, q, thr = RO.threshold(w0, 7, 9, -1.0)
    assert pc == 9 / 7 - 1 and q == 1 / (9 / 7 - 1 + 1.0) and 0 < q < 1
    s = np.sort(w0.astype(np.float64).reshape(-1))
    rank = q * 6
    lo = int(np.floor(rank))
    assert abs(thr - (s[lo] + (rank - lo) * (s[lo + 1] - s[lo]))) <= 1e-15
    r = RO.rewire_khop(ei, w0, N, -1.0, 0)
    assert (r['mask'] == (p['values'] > thr)).all()
    sums = np.zeros(N)
    np.add.at(sums, r['edge_index'][0, 0], r['weights'])
    assert np.allclose(sums[np.unique(r['edge_index'][0, 0])], 1.0, atol=1e-12)


def _bounds(name):
    """(ub per row) of the oracle's graph: which regime a row takes."""
    ei, w0, N = RO.prepared(name)
    A = (RO.product(name)['W'] != 0).astype(np.int64)
    return A @ A.sum(axis=1)


def test_fixtures_reach_every_regime():
    assert _bounds('wide').max() > ops.TWO_HOP_LDS_MAX and (_bounds('wide') <= ops.TWO_HOP_LDS_MAX).any()
    ub = _bounds('hub')
    assert ub.max() > ops.TWO_HOP_LDS_MAX and ((ub > 64) & (ub <= ops.TWO_HOP_LDS_MAX)).any() and (ub <= 64).any()
    ub = _bounds('empty')
    assert (ub == 0).any() and (ub > 0).any()
    ei, w0, N = RO.prepared('empty')
    assert (np.bincount(ei[0, 0], minlength=N)[ub == 0] > 0).any()     # a stored row whose neighbour rows are empty
    assert np.bincount(RO.prepared('hub')[0][0, 0]).max() > 64          # a neighbour row longer than a wavefront


@pytest.mark.parametrize("name", sorted(KEPT))
def test_kept_set_conditions_hold(name):
    """What the GPU kept-set checks rest on, from the oracle alone: q in (0, 1) and at most 1 %
    of the scores within tau * threshold of the threshold."""
    ei, w0, N = RO.prepared(name)
    r = RO.rewire_khop(ei, w0, N, KEPT[name], 0)
    assert 0 < r['q'] < 1
    assert r['undecided'].mean() <= 0.01
    assert 0 < r['mask'].sum() < r['mask'].size


def test_random_union_vs_oracle():
    ei, w0, N = RO.prepared('directed')
    blk = _with_graph(_block(new_edges='random', rw_addD=0.5), 'directed')
    M = RO.n_random(N, 0.5)
    assert M == N
    pairs = np.random.default_rng(5).integers(0, N, size=(2, M))
    pairs[:, :10] = ei[0, :, :10]                 # pairs the graph already has
    pairs[:, 10:15] = pairs[:, 15:20]             # and repeated draws
    blk.add_random_edges(torch.from_numpy(pairs))
    want = RO.union_random(ei, pairs, N)
    assert blk.data_edge_index.shape == want.shape and (blk.data_edge_index.numpy() == want).all()
    assert blk.odefunc.edge_index is blk.data_edge_index
    # the block's own draw: M pairs from its generator, reproducible from the seed
    a, b = [_with_graph(_block(new_edges='random', rw_addD=0.5), 'directed') for _ in range(2)]
    a.add_random_edges()
    b.add_random_edges()
    assert torch.equal(a.data_edge_index, b.data_edge_index)
    assert ei.shape[2] < a.data_edge_index.shape[2] <= ei.shape[2] + M


@pytest.mark.parametrize("name", ["toy", "short", "dups"])
def test_oracle_vs_reference_golden(name):
    """The oracle's S against the dense matrix the reference's own add_khop_edges forms
    (src/block_transformer_rewiring.py:68-77), recorded in float64 by gen_golden_rewire.py."""
    d = np.load(os.path.join(GOLDEN, "rewire", "khop_%s.npz" % name), allow_pickle=False)
    meta = json.loads(str(d["meta"]))
    ei, w0, N = RO.prepared(name)
    assert meta["N"] == N and (d["edge_index"] == ei).all() and (d["w0"] == w0).all()
    p = RO.two_hop(d["edge_index"], d["w0"], N)
    assert np.abs(p['S'] - d["S"]).max() <= 1e-12
    # the positions cover every non-zero of the recorded matrix (and the diagonal besides)
    struct = np.zeros((N, N), bool)
    struct[p['edge_index'][0, 0], p['edge_index'][0, 1]] = True
    assert (struct | (d["S"] == 0)).all()
    with open(os.path.join(GOLDEN, "rewire", "MANIFEST.json")) as fh:
        assert name in [m["name"] for m in json.load(fh)]
