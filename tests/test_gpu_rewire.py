"""The rewire_attention block on the GPU: the two-hop product kernel (csrc/two_hop.hip) against
the float64 oracle (tests/rewire_oracle.py) in every row regime, the kept set, and the block
end to end (training and eval forwards, gradients, the transformer RHS, 'random').

Value bound of the kernel: |S_gpu - S| <= (n_ij + 3) 2^-24 S with n_ij the products of the
position — derived, not measured: every term is non-negative, so any fixed order of n fp32
products and sums (here: one fma per product in CSR order, one add of W[i, j], an exact
halving) stays within it; a duplicate-summed entry of W carries one rounding per duplicate,
which the raw edge pairs n_ij counts cover (d1 + d2 - 1 <= d1 d2)."""
import numpy as np
import pytest
import torch

import gnpde
import gnpde_oracle as O
import rewire_oracle as RO
from gnpde import ops
from test_gpu_parity import OPT as BASE_OPT, RTOL, T, _set_qk, rel
from test_rewire_host import KEPT

pytestmark = pytest.mark.gpu
DEV = "cuda"

OPT = dict(BASE_OPT, block='rewire_attention', att_samp_pct=0.5, new_edges='k_hop_att', sparsify='S_hat',
           threshold_type='addD_rvR', rw_addD=0.02, use_flux=False)

# (fixture, lds_max): None = the default boundary (512, the largest); 0 = every row with a product in the
# global regime; 64 / 16 = a boundary inside the fixture's own spread of bounds
CASES = [(n, None) for n in RO.NAMES] + [('toy', 0), ('short', 0), ('dups', 0), ('empty', 0), ('hub', 0),
                                          ('hub', 64), ('directed', 16)]


def _two_hop(name, lds_max, **kw):
    ei, w0, N = RO.prepared(name)
    return ops.two_hop(T(ei), T(w0), num_nodes=N, lds_max=lds_max, return_col=True, **kw)


@pytest.mark.parametrize("name,lds_max", CASES)
def test_two_hop_vs_oracle(name, lds_max):
    want = RO.product(name)
    e, v, rowptr, col = _two_hop(name, lds_max)
    assert e.dtype == torch.int64 and v.dtype == torch.float32 and rowptr.dtype == torch.int32
    assert (rowptr.cpu().numpy() == want['rowptr']).all()
    assert e.shape == want['edge_index'].shape and (e.cpu().numpy() == want['edge_index']).all()
    assert (col.cpu().numpy() == want['edge_index'][0, 1]).all()
    S = want['values']
    err = np.abs(v.double().cpu().numpy() - S)
    bound = (want['n'] + 3) * 2.0 ** -24 * S
    print("two_hop %s lds_max=%s: nnz %d, max err / bound %.3f" % (name, lds_max, S.size,
                                                                  (err / np.maximum(bound, 1e-300)).max() if S.size else 0))
    assert (err <= bound).all()
    diag = want['edge_index'][0, 0] == want['edge_index'][0, 1]
    assert (v.cpu().numpy()[diag] == 0).all()
    # deterministic: a second call, and the other scratch geometry, give the same bits
    e2, v2, rowptr2, col2 = _two_hop(name, lds_max)
    assert torch.equal(v, v2) and torch.equal(e, e2) and torch.equal(rowptr, rowptr2)
    e3, v3, _, _ = _two_hop(name, lds_max, scratch_bytes=1)    # one resident wavefront walks every wide row
    assert torch.equal(v, v3) and torch.equal(e, e3)


def test_two_hop_regimes_agree_bitwise():
    """The summation order is the CSR order of row i in every regime: the same bits."""
    a = _two_hop('hub', None)
    for lds_max in (0, 64, 512):
        b = _two_hop('hub', lds_max)
        assert torch.equal(a[1], b[1]) and torch.equal(a[0], b[0])


def test_two_hop_inputs():
    ei, w0, N = RO.prepared('directed')
    want = RO.product('directed')
    g = ops.GraphCSR(T(ei), N)
    e, v, rowptr = ops.two_hop(g, T(w0))
    assert (e.cpu().numpy() == want['edge_index']).all()
    # a coalesced CSR with CSR-order values
    r, c = np.nonzero(want['W'])
    rp = np.zeros(N + 1, np.int32)
    rp[1:] = np.cumsum(np.bincount(r, minlength=N))
    e2, v2, rowptr2 = ops.two_hop((T(rp), T(c.astype(np.int32))), T(want['W'][r, c].astype(np.float32)))
    assert torch.equal(e, e2) and torch.equal(v, v2) and torch.equal(rowptr, rowptr2)   # no duplicates: W is exact
    with pytest.raises(TypeError):
        ops.two_hop(g, T(w0).double())
    with pytest.raises(ValueError, match="lds_max"):
        ops.two_hop(g, T(w0), lds_max=ops.TWO_HOP_LDS_MAX + 1)
    # the torch restatement on the device: same positions
    e3, v3, rowptr3 = ops.two_hop_torch(T(ei), T(w0), num_nodes=N)
    assert torch.equal(e, e3) and torch.equal(rowptr, rowptr3)
    assert rel(v3, v.double().cpu().numpy()) <= 1e-6


def _block(func, name, **kw):
    ei, attr, N, fill = RO.raw(name)
    opt = dict(OPT, self_loop_weight=fill, **kw)
    blk = gnpde.RewireAttODEblock(func, [], opt, DEV, t=torch.tensor([0, 1])).to(DEV)
    data = gnpde.GraphData()
    data.new_graph(T(ei), N, edge_attr=T(attr))
    return blk, data, N


def _prepared_on_device(blk, data, name):
    """The block's own prepared graph; it equals the oracle's (the weights to fp32 rounding)."""
    blk.reset_graph_data(data, torch.float32)
    ei, w0, N = RO.prepared(name)
    assert (blk.data_edge_index.cpu().numpy() == ei).all()
    w_dev = blk.odefunc.edge_weight.cpu().numpy()
    assert np.abs(w_dev.astype(np.float64) - w0).max() <= 2e-7
    return ei, w_dev, N


def _weight_tol(r):
    """Relative bound of a renormalised weight s / (group sum + 1e-16): the score's and the sum's
    relative error, each at most the product's (n_max + 3) 2^-24, plus the fp32 sum's own roundings
    (positive terms: at most one ulp of the total per term is not reached by far; 2 ulps taken), the
    division and the rounding of the stored result."""
    return (2 * (r['two_hop']['n'].max() + 3) + 4) * 2.0 ** -24


@pytest.mark.parametrize("name", sorted(KEPT))
def test_kept_set_vs_oracle(name):
    """Decided edges (oracle score further than tau * threshold from the oracle threshold) are kept
    or dropped exactly as in the oracle; the kept weights renormalise to the oracle's."""
    blk, data, N = _block(gnpde.LaplacianODEFunc, name, rw_addD=KEPT[name], hidden_dim=8)
    blk.train()
    ei, w_dev, N = _prepared_on_device(blk, data, name)
    r = RO.rewire_khop(ei, w_dev, N, KEPT[name], 0)
    assert 0 < r['q'] < 1 and r['undecided'].mean() <= 0.01
    with torch.no_grad():
        blk.rewire(T(np.zeros((1, N, 8), np.float32)))
    assert abs(blk.q - r['q']) <= 1e-12 and abs(float(blk.threshold) - r['threshold']) <= 1e-6 * r['threshold']
    new = r['two_hop']['edge_index']
    got = np.zeros(new.shape[2], bool)
    kept = blk.odefunc.edge_index.cpu().numpy()
    key = new[0, 0] * N + new[0, 1]
    kk = kept[0, 0] * N + kept[0, 1]
    assert (np.diff(kk) > 0).all()                         # list order: ascending (row, col), each once
    at = np.searchsorted(key, kk)
    assert (key[at] == kk).all()
    got[at] = True
    dec = ~r['undecided']
    assert (got[dec] == r['mask'][dec]).all()
    assert blk.retained == kept.shape[2] and blk.data_edge_index is blk.odefunc.edge_index
    assert blk.odefunc.edge_weight is blk.odefunc.attention_weights
    assert blk.reg_odefunc.odefunc.edge_index is not None
    if not r['undecided'].any():
        gw = blk.odefunc.edge_weight.double().cpu().numpy()[0]
        assert (np.abs(gw - r['weights']) <= _weight_tol(r) * r['weights']).all()


E2E = [('short', -3.0), ('hub', 0.02)]


@pytest.mark.parametrize("norm_idx", [0, 1])
@pytest.mark.parametrize("name,rw_addD", E2E)
def test_training_forward_and_gradients_vs_oracle(name, rw_addD, norm_idx):
    """Training forward (laplacian, rk4) against the float64 solve over the oracle's rewired graph;
    gradients of x and alpha_train against float64 autograd over that fixed graph."""
    C = 8
    blk, data, N = _block(gnpde.LaplacianODEFunc, name, rw_addD=rw_addD, hidden_dim=C, method='rk4', step_size=0.5,
                          attention_norm_idx=norm_idx)
    blk.train()
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.3)
    ei, w_dev, N = _prepared_on_device(blk, data, name)
    r = RO.rewire_khop(ei, w_dev, N, rw_addD, norm_idx)
    assert 0 < r['q'] < 1 and not r['undecided'].any() and r['mask'].sum() > 10
    x = np.random.default_rng(7).standard_normal((1, N, C)).astype(np.float32)
    xt = T(x).requires_grad_(True)
    z = blk(xt, data)
    assert (blk.odefunc.edge_index.cpu().numpy() == r['edge_index']).all()
    gw = blk.odefunc.edge_weight.double().cpu().numpy()[0]
    assert (np.abs(gw - r['weights']) <= _weight_tol(r) * r['weights']).all()
    es, ws = r['edge_index'], r['weights'][None]
    f = lambda t, y: O.laplacian_rhs(es, y, None, 0.3, 0.0, edge_weight=ws)  # noqa: E731
    want = O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.5)
    assert rel(z, want) <= RTOL
    gout = np.random.default_rng(8).standard_normal((1, N, C)).astype(np.float32)
    z.backward(T(gout))
    # float64 autograd over the fixed rewired graph
    A = torch.zeros(N, N, dtype=torch.float64).index_put_((torch.from_numpy(es[0, 0]), torch.from_numpy(es[0, 1])),
                                                          torch.from_numpy(ws[0]), accumulate=True)
    x64 = torch.from_numpy(x[0]).double().requires_grad_(True)
    al = torch.tensor(0.3, dtype=torch.float64, requires_grad=True)
    rhs = lambda y: torch.sigmoid(al) * (A @ y - y)  # noqa: E731
    y = x64
    for _ in range(2):
        dt = 0.5
        k1 = rhs(y)
        k2 = rhs(y + dt * k1 / 3.0)
        k3 = rhs(y + dt * (k2 - k1 / 3.0))
        k4 = rhs(y + dt * (k1 - k2 + k3))
        y = y + (k1 + 3.0 * (k2 + k3) + k4) * dt * 0.125
    assert np.abs(y.detach().numpy() - want[0]).max() <= 1e-12
    (y * torch.from_numpy(gout[0]).double()).sum().backward()
    assert rel(xt.grad[0], x64.grad.numpy()) <= 1e-4
    ga = float(al.grad)
    assert abs(float(blk.odefunc.alpha_train.grad) - ga) <= 1e-4 * abs(ga)


@pytest.mark.parametrize("name", ['short', 'hub'])
def test_eval_forward_vs_oracle_and_hard_attention(name):
    C, h, att = 8, 2, 16
    kw = dict(hidden_dim=C, heads=h, attention_dim=att, method='rk4', step_size=0.5, attention_norm_idx=1)
    blk, data, N = _block(gnpde.LaplacianODEFunc, name, **kw)
    blk.eval()
    rng = np.random.default_rng(11)
    Wq, bq, Wk, bk = _set_qk(blk.multihead_att_layer, rng, C, att, scale=0.3)
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    ei, w_dev, N = _prepared_on_device(blk, data, name)
    with torch.no_grad():
        z = blk(T(x), data)
    mean = O.transformer_attention(x, ei, Wq, bq, Wk, bk, h, 1).mean(axis=2)
    assert np.abs(blk.odefunc.edge_weight.double().cpu().numpy() - mean).max() <= 2e-6
    assert blk.odefunc.attention_weights is blk.odefunc.edge_weight
    f = lambda t, y: O.laplacian_rhs(ei, y, None, 0.0, 0.0, edge_weight=mean)  # noqa: E731
    want = O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.5)
    assert rel(z, want) <= RTOL
    hard = gnpde.HardAttODEblock(gnpde.LaplacianODEFunc, [], dict(blk.opt, block='hard_attention'), DEV,
                                 t=torch.tensor([0, 1])).to(DEV).eval()
    hard.load_state_dict(blk.state_dict())
    with torch.no_grad():
        zh = hard(T(x), data)
    assert rel(z, zh.double().cpu().numpy()) <= 1e-6


def test_transformer_training_forward_vs_oracle():
    """function='transformer': the RHS recomputes its attention over the kept list at every
    evaluation; against the oracle's transformer RHS over the oracle's kept list."""
    name, rw_addD, C, h, att = 'hub', 0.02, 8, 2, 16
    blk, data, N = _block(gnpde.ODEFuncTransformerAtt, name, function='transformer', rw_addD=rw_addD, hidden_dim=C,
                          heads=h, attention_dim=att, method='rk4', step_size=0.5, attention_norm_idx=0)
    blk.train()
    rng = np.random.default_rng(13)
    Wq, bq, Wk, bk = _set_qk(blk.odefunc.multihead_att_layer, rng, C, att, scale=0.3)
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(0.3)
    ei, w_dev, N = _prepared_on_device(blk, data, name)
    r = RO.rewire_khop(ei, w_dev, N, rw_addD, 0)
    assert not r['undecided'].any()
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    with torch.no_grad():
        z = blk(T(x), data)
        f0 = blk.odefunc(0.0, T(x))
    es = r['edge_index']
    assert (blk.odefunc.edge_index.cpu().numpy() == es).all()
    f = lambda t, y: O.transformer_rhs(es, y, None, Wq, bq, Wk, bk, h, 0, 0.3, 0.0)  # noqa: E731
    assert rel(f0, f(0.0, x)) <= RTOL
    assert rel(z, O.odeint_fixed(f, x, 0.0, 1.0, 'rk4', 0.5)) <= RTOL


def test_random_edges_recalculated_attention():
    """new_edges='random' with injected pairs, sparsify='recalc_att': the union list exactly, the
    kept weights (the recomputed head-mean attention, renormalised) on the decided edges."""
    name, rw_addD, C, h, att = 'directed', 0.95, 8, 2, 16
    blk, data, N = _block(gnpde.LaplacianODEFunc, name, new_edges='random', sparsify='recalc_att', rw_addD=rw_addD,
                          hidden_dim=C, heads=h, attention_dim=att, method='rk4', step_size=0.5, attention_norm_idx=1)
    blk.train()
    rng = np.random.default_rng(17)
    Wq, bq, Wk, bk = _set_qk(blk.multihead_att_layer, rng, C, att, scale=0.3)
    ei, w_dev, N = _prepared_on_device(blk, data, name)
    M = RO.n_random(N, rw_addD)
    pairs = rng.integers(0, N, size=(2, M))
    new = RO.union_random(ei, pairs, N)
    pc, q, thr = RO.threshold(w_dev, ei.shape[2], new.shape[2], rw_addD)
    assert 0 < q < 1
    x = rng.standard_normal((1, N, C)).astype(np.float32)
    scores = O.transformer_attention(x, new, Wq, bq, Wk, bk, h, 1).mean(axis=2)[0]
    und = RO.undecided(scores, thr, 2e-5 / thr)      # the fp32 attention's own error, 2e-5 absolute
    assert not und.any()
    mask, kept, w = RO.keep(new, scores, thr, 1, N)
    assert mask.sum() > 10
    with torch.no_grad():
        z = blk(T(x), data, pairs=T(pairs))
    assert abs(blk.q - q) <= 1e-12
    got = blk.odefunc.edge_index.cpu().numpy()
    kk, key = got[0, 0] * N + got[0, 1], new[0, 0] * N + new[0, 1]
    at = np.searchsorted(key, kk)
    assert (np.diff(kk) > 0).all() and (key[at] == kk).all()
    gm = np.zeros(new.shape[2], bool)
    gm[at] = True
    assert (gm[~und] == mask[~und]).all()
    gw = np.zeros(new.shape[2])
    gw[at] = blk.odefunc.edge_weight.double().cpu().numpy()[0]
    ww = np.zeros(new.shape[2])
    ww[mask] = w
    both = gm & mask
    assert rel(gw[both], ww[both]) <= RTOL
    assert torch.isfinite(z).all()
