"""Pins the transformer mix_features restatement (tests/mix_oracle.py) against the reference's
own pieces composed as its call site intends, in float64 (tests/golden/mix/mix_*.npz,
mixgrad_*.npz, made by tests/golden/gen_golden_mix.py), and the host side of the feature: the
opt-in key, the settings that still raise, the unchanged state_dict and the refusals of what
is out of scope (bf16 states, node layouts, feature padding, the multi-GPU wrappers)."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gnpde
import gnpde_oracle as O
import mix_oracle as M
from conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "mix")  # a directory of its own, with its own MANIFEST.json
MIX = sorted(glob.glob(os.path.join(GOLDEN, "mix_*.npz")))
MIXGRAD = sorted(glob.glob(os.path.join(GOLDEN, "mixgrad_*.npz")))
PNAMES = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wout", "bout")

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 12, 'block': 'constant', 'function': 'transformer', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'step_size': 1, 'max_nfe': 1000,
       'multi_modal': False, 'mix_features': True, 'attention_dim': 16, 'attention_type': 'scaled_dot',
       'beltrami': False, 'square_plus': False, 'reweight_attention': False}


def load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


def test_the_cover_of_the_issue_is_present():
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as fh:
        assert sorted(json.load(fh)) == sorted(os.path.basename(p)[:-4] for p in MIX + MIXGRAD)
    fwd = [load(p)[1] for p in MIX]
    key = lambda m: (m["attention_type"], m["score_mode"], m["attention_norm_idx"], m["square_plus"])  # noqa: E731
    have = set(key(m) for m in fwd)
    for want in (("scaled_dot", "reference", 0, False), ("scaled_dot", "reference", 1, False),
                 ("scaled_dot", "per_edge", 0, False), ("scaled_dot", "per_edge", 1, False)):
        assert want in have
    assert {"exp_kernel", "cosine_sim", "pearson"} <= set(m["attention_type"] for m in fwd)
    assert {1, 2, 3, 4, 8} <= set(m["heads"] for m in fwd)
    dks = set(m["attention_dim"] // m["heads"] for m in fwd)
    assert {4, 8, 16, 64} <= dks and any(dk % 4 for dk in dks)
    assert {12, 128, 162} <= set(m["C"] for m in fwd)
    assert any(m["B"] == 2 for m in fwd) and any(m["add_source"] for m in fwd)
    assert any(m["no_alpha_sigmoid"] for m in fwd) and any(m["square_plus"] for m in fwd)
    grad = set(key(load(p)[1]) for p in MIXGRAD)
    assert ("scaled_dot", "reference", 1, False) in grad and ("scaled_dot", "per_edge", 0, False) in grad
    assert any(k[0] == "exp_kernel" for k in grad) and any(k[3] for k in grad)
    assert any(m["B"] == 2 and m["heads"] == 8 for m in (load(p)[1] for p in MIXGRAD))
    for p in MIX + MIXGRAD:
        d, m = load(p)
        assert os.path.getsize(p) < 1 << 20 and m["N"] <= 80 and m["E"] <= 400
        dk = m["attention_dim"] // m["heads"]
        assert d["Wout"].shape == (m["C"], dk) and d["bout"].shape == (m["C"],)
        assert d["Wv"].shape == (m["attention_dim"], m["C"]) and d["v"].shape == (m["B"], m["N"], m["attention_dim"])
        for n in PNAMES:  # random parameters, none of them the constant 1e-5 init or a zero bias
            assert np.abs(d[n]).min() > 0 and np.unique(d[n]).size > 1
        if m["kind"] == "mix":
            assert rel(d["f_ref32"], d["f"]) <= 2e-6 and abs(rel(d["f_ref32"], d["f"]) - m["ref32_dev"]) <= 1e-12
        else:
            for n in PNAMES:
                assert d["g_" + n].shape == d[n].shape
            assert all(np.abs(d["g_" + n]).max() > 0 for n in ("Wv", "bv", "Wout", "bout"))
            if m["square_plus"]:
                assert min(m["max_margin"]) >= 1e-3
    # duplicate edges and isolated nodes
    d, m = load(os.path.join(GOLDEN, "mix_pe_n0_h4_c128.npz"))
    e = d["edge_index"][0]
    assert np.unique(e.T, axis=0).shape[0] < e.shape[1] and np.setdiff1d(np.arange(m["N"]), e[0]).size >= 3


@pytest.mark.parametrize("path", MIX + MIXGRAD, ids=os.path.basename)
def test_restatement_matches_reference(path):
    d, m = load(path)
    f, att, v = M.fixture_rhs(d)
    assert f.shape == d["f"].shape
    assert rel(f, d["f"]) <= 1e-12
    assert np.abs(att - d["attention"]).max() <= 1e-12
    assert rel(v, d["v"]) <= 1e-12
    # a row without edges: z = 0, ax = b_out
    z = M.head_aggregate(d["edge_index"], d["attention"], d["v"])
    for b in range(m["B"]):
        iso = np.setdiff1d(np.arange(m["N"]), d["edge_index"][b, 0])
        assert not z[b, iso].any()
    # the layer's layout of v is a transposed view of the projection
    lv = M.layer_values(d["v"], m["heads"])
    assert lv.shape == (m["B"], m["N"], m["attention_dim"] // m["heads"], m["heads"])
    assert np.array_equal(lv[..., 0], d["v"][..., :m["attention_dim"] // m["heads"]])


@pytest.mark.parametrize("path", MIX[:3], ids=os.path.basename)
def test_equal_heads_fold_to_the_plain_aggregation(path):
    """With the same weight in every head, z is the plain aggregation of v folded over the heads."""
    d, m = load(path)
    H, dk = m["heads"], m["attention_dim"] // m["heads"]
    w = d["attention"].mean(axis=2)
    z = M.head_aggregate(d["edge_index"], np.repeat(w[:, :, None], H, axis=2), d["v"])
    full = O.aggregate(d["edge_index"], w, d["v"])
    assert rel(z, full.reshape(m["B"], m["N"], H, dk).mean(axis=2)) <= 1e-12


def test_mix_features_is_opt_in():
    for make in (gnpde.ODEFuncTransformerAtt, gnpde.SpGraphTransAttentionLayer):
        with pytest.raises(NotImplementedError, match="gnpde_mix_features"):
            make(12, 12, dict(OPT), None)
        with pytest.raises(NotImplementedError, match="gnpde_mix_features"):
            make(12, 12, dict(OPT, gnpde_mix_features=False), None)
    func = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, gnpde_mix_features=True), None)
    assert func.multihead_att_layer.mix
    assert not func.supports_node_layout() and not func.supports_feature_padding()
    # the key alone changes nothing: mix_features=False stays the aggregation of x
    plain = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, mix_features=False, gnpde_mix_features=True), None)
    assert not plain.multihead_att_layer.mix
    assert plain.supports_node_layout() and plain.supports_feature_padding()
    bare = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, mix_features=False), None)
    assert bare.supports_node_layout() == plain.supports_node_layout()


def test_other_settings_still_raise():
    for make in (gnpde.ODEFuncTransformerAtt, gnpde.SpGraphTransAttentionLayer):
        with pytest.raises(NotImplementedError, match="multi_modal"):
            make(12, 12, dict(OPT, gnpde_mix_features=True, multi_modal=True), None)
        with pytest.raises(NotImplementedError, match="beltrami"):
            make(12, 12, dict(OPT, gnpde_mix_features=True, beltrami=True, attention_type='exp_kernel'), None)
        with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
            make(12, 12, dict(OPT, gnpde_mix_features=True, square_plus=True), None)


def test_state_dict_keys_unchanged():
    mix = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, gnpde_mix_features=True), None)
    plain = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, mix_features=False), None)
    assert list(mix.state_dict()) == list(plain.state_dict())
    lay = mix.multihead_att_layer
    assert tuple(lay.Wout.weight.shape) == (12, 8) and tuple(lay.V.weight.shape) == (16, 12)
    plain.load_state_dict(mix.state_dict())


def test_bf16_state_is_rejected_before_any_kernel():
    func = gnpde.ODEFuncTransformerAtt(12, 12, dict(OPT, gnpde_mix_features=True), None)
    with pytest.raises(NotImplementedError, match="fp32"):
        func.multihead_att_layer.project(torch.zeros(1, 4, 12, dtype=torch.bfloat16))


def test_multi_gpu_wrappers_refuse_mix_features():
    from gnpde import dist
    for cls in (dist.ColumnShardedTransformer, dist.RowShardedTransformer):
        with pytest.raises(NotImplementedError, match="mix_features"):
            cls(torch.zeros(1, 2, 4, dtype=torch.long), 4, 12, None, None, None, None, 2, 0, None, mix_features=True)
