"""CPU: the multi_modal fixtures (tests/golden/multimodal, the reference's own Laplacian
forward on the restated cross-attention, float64) against the numpy restatement
tests/multimodal_oracle.py, the torch restatement of the kernel's contract
(ops.cross_attention_torch), and the host side of the option: what selects
MultiModalLaplacianODEFunc, its parameters and everything that still raises."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import multimodal_oracle as MM
from conftest import GOLDEN as _GOLDEN
from gnpde import ops
from gnpde.function_laplacian_multimodal import MultiModalLaplacianODEFunc

GOLDEN = os.path.join(_GOLDEN, "multimodal")
FWD = sorted(glob.glob(os.path.join(GOLDEN, "mm_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "mmgrad_*.npz")))
ORACLE_TOL = 1e-12
REF32_CAP = 5e-6   # the generator's fixture condition: half of the device bar (1e-5)

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 12, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'step_size': 1, 'max_nfe': 1000,
       'multi_modal': True, 'gnpde_multi_modal': True, 'second_modality_dim': 7, 'mix_features': False,
       'attention_dim': 16, 'attention_type': 'scaled_dot', 'beltrami': False, 'square_plus': False,
       'reweight_attention': False, 'data_norm': 'rw'}


def load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def relerr(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_manifest_lists_the_fixtures():
    names = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
    assert sorted(names) == sorted(os.path.basename(p)[:-4] for p in FWD + GRAD)
    assert len(FWD) >= 4 and len(GRAD) >= 2
    assert max(os.path.getsize(p) for p in FWD + GRAD) < 100 * 1000
    metas = [load(p)[1] for p in FWD]
    assert any(m["add_source"] for m in metas) and any(not m["add_source"] for m in metas)
    assert any(m["no_alpha_sigmoid"] for m in metas) and any(m["B"] == 2 for m in metas)


@pytest.mark.parametrize("path", FWD + GRAD, ids=os.path.basename)
def test_oracle_matches_the_reference_fixture(path):
    d, m = load(path)
    f, xt = MM.fixture_rhs(d)
    assert relerr(f, d["f"]) <= ORACLE_TOL
    if "xt" in d.files:
        assert relerr(xt, d["xt"]) <= ORACLE_TOL
    # the generator's condition on the draw: the reference's own fp32 run is well inside the bar
    assert relerr(d["f_ref32"], d["f"]) <= REF32_CAP
    assert abs(relerr(d["f_ref32"], d["f"]) - m["ref32_dev"]) <= 1e-12
    if not m["add_source"]:
        assert not d["x0"].any()


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_oracle_gradients_match_the_reference_autograd(path):
    d, _ = load(path)
    g = MM.fixture_grads(d)
    names = sorted(k for k in d.files if k.startswith("g_"))
    assert names == sorted(g)
    for n in names:
        want = d[n]
        err = float(np.abs(g[n].reshape(want.shape) - want).max())
        assert err <= ORACLE_TOL * max(1.0, float(np.abs(want).max())), (n, err)


@pytest.mark.parametrize("B,N,M,C", [(1, 1, 1, 4), (2, 37, 45, 12), (1, 70, 33, 80)])
def test_cross_attention_torch_matches_the_oracle(B, N, M, C):
    rng = np.random.default_rng(B + N + M + C)
    q, k, v = (rng.standard_normal(s).astype(np.float32) for s in ((B, N, C), (B, M, C), (B, M, C)))
    scale = 1.0 / np.sqrt(C)
    want, lse = MM.cross_attention(q, k, v, scale, lse=True)
    got, got_lse = ops.cross_attention_torch(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), scale,
                                             lse=True)
    assert tuple(got.shape) == (B, N, C) and tuple(got_lse.shape) == (B, N)
    assert relerr(got.numpy(), want) <= 1e-5
    assert relerr(got_lse.numpy(), lse) <= 1e-5
    # float64 inputs are refused (the contract is fp32), as are mismatched shapes and M = 0
    with pytest.raises(TypeError):
        ops.cross_attention_torch(torch.from_numpy(q).double(), torch.from_numpy(k), torch.from_numpy(v), scale)
    with pytest.raises(ValueError):
        ops.cross_attention_torch(torch.from_numpy(q), torch.from_numpy(k)[:, :, :-1], torch.from_numpy(v), scale)
    with pytest.raises(ValueError, match="M = 0"):
        ops.cross_attention_torch(torch.from_numpy(q), torch.from_numpy(k)[:, :0], torch.from_numpy(v)[:, :0], scale)


def test_cross_attention_needs_a_device():
    q = torch.zeros(1, 3, 4)
    with pytest.raises(RuntimeError, match="ROCm device"):
        ops.cross_attention(q, q, q, 0.5)


def test_set_function_selects_the_class():
    assert gnpde.set_function(OPT) is MultiModalLaplacianODEFunc
    assert gnpde.MultiModalLaplacianODEFunc is MultiModalLaplacianODEFunc
    assert gnpde.set_function(dict(OPT, multi_modal=False)) is gnpde.LaplacianODEFunc
    assert gnpde.set_function(dict(OPT, gnpde_multi_modal=False)) is gnpde.LaplacianODEFunc
    assert not issubclass(MultiModalLaplacianODEFunc, gnpde.LaplacianODEFunc)


def test_state_dict_and_hooks():
    func = MultiModalLaplacianODEFunc(12, 12, OPT, None)
    ref = gnpde.LaplacianODEFunc(12, 12, dict(OPT, multi_modal=False), None)
    extra = ["Q2.weight", "Q2.bias", "V2.weight", "V2.bias", "K2.weight", "K2.bias"]
    assert list(func.state_dict()) == list(ref.state_dict()) + extra
    assert tuple(func.Q2.weight.shape) == (12, 12)
    assert tuple(func.K2.weight.shape) == (12, 7) and tuple(func.V2.weight.shape) == (12, 7)
    for lin in (func.Q2, func.K2, func.V2):    # the fork's constant weight initialisation
        assert bool((lin.weight == 1e-5).all())
    assert func.y is None
    assert func.affine is False and not func.fold_dense
    assert not func.supports_feature_padding() and not func.supports_node_layout()
    # none of the hooks the integrator keys its affine Laplacian fast paths on
    for hook in ("_weights_tensor", "fixed_grid_backward_ok", "adjoint_const_weights", "adjoint_direct_ok"):
        assert not hasattr(func, hook)
    assert hasattr(func, "rhs_stage") and hasattr(func, "graph_capture_state")


def test_block_builds_and_hands_y_over():
    blk = gnpde.ConstantODEblock(gnpde.set_function(OPT), [], OPT, None)
    assert isinstance(blk.odefunc, MultiModalLaplacianODEFunc)
    y = torch.zeros(1, 3, 7)
    blk.reset_graph_data(None, torch.float32, y)
    assert blk.odefunc.y is y


def test_raises():
    # without the key every function raises as before
    plain = dict(OPT, gnpde_multi_modal=False)
    with pytest.raises(NotImplementedError, match="multi_modal"):
        gnpde.LaplacianODEFunc(12, 12, plain, None)
    with pytest.raises(NotImplementedError, match="multi_modal"):
        gnpde.ODEFuncTransformerAtt(12, 12, dict(plain, function='transformer'), None)
    with pytest.raises(NotImplementedError, match="multi_modal"):
        gnpde.ODEFuncAtt(12, 12, dict(plain, function='GAT', gnpde_gat=True), None)
    # with the key: the plain class points at set_function; transformer / GAT / other blocks say what is served
    with pytest.raises(NotImplementedError, match="set_function"):
        gnpde.LaplacianODEFunc(12, 12, OPT, None)
    with pytest.raises(NotImplementedError, match="function='laplacian'"):
        gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, function='transformer'), None)
    with pytest.raises(NotImplementedError, match="function='laplacian'"):
        gnpde.ODEFuncAtt(12, 12, dict(OPT, function='GAT', gnpde_gat=True), None)
    for block in ("attention", "mixed", "hard_attention"):
        with pytest.raises(NotImplementedError, match="block='constant'"):
            MultiModalLaplacianODEFunc(12, 12, dict(OPT, block=block), None)
    no_d2 = {k: v for k, v in OPT.items() if k != 'second_modality_dim'}
    with pytest.raises(ValueError, match="second_modality_dim"):
        MultiModalLaplacianODEFunc(12, 12, no_d2, None)
    with pytest.raises(ValueError, match="gnpde_multi_modal"):
        MultiModalLaplacianODEFunc(12, 12, plain, None)


def test_evaluation_time_raises():
    func = MultiModalLaplacianODEFunc(12, 12, OPT, None)
    x = torch.zeros(2, 5, 12)
    with pytest.raises(RuntimeError, match="y is not set"):
        func(torch.tensor(0.0), x)
    func.y = torch.zeros(3, 4, 7)
    with pytest.raises(ValueError, match="batch"):
        func(torch.tensor(0.0), x)
    func.y = torch.zeros(2, 0, 7)
    with pytest.raises(ValueError, match="M = 0"):
        func(torch.tensor(0.0), x)
    func.y = torch.zeros(2, 4, 6)
    with pytest.raises(ValueError, match="second_modality_dim"):
        func(torch.tensor(0.0), x)
    func.y = torch.zeros(2, 4, 7)
    with pytest.raises(NotImplementedError, match="fp32"):
        func(torch.tensor(0.0), x.to(torch.bfloat16))
