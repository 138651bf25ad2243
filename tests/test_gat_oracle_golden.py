"""Pins the GAT restatement (tests/gat_oracle.py) against the reference's own float64
run of src/function_GAT_attention.py (tests/golden/gat/gat_*.npz, gatgrad_*.npz, made by
tests/golden/gen_golden_gat.py), and the host side of the GAT function: the registry
switch, the layer's parameters and the settings that raise."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import gat_oracle as G
import gnpde
from conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "gat")  # a directory of its own: tests/golden/MANIFEST.json lists tests/golden/*.npz

GAT = sorted(glob.glob(os.path.join(GOLDEN, "gat_*.npz")))
GATGRAD = sorted(glob.glob(os.path.join(GOLDEN, "gatgrad_*.npz")))
FWD_NAMES = ["gat_n0_h2", "gat_n1_h2", "gat_n1_h8_b2", "gat_n0_h1_b3", "gat_n0_h4_src", "gat_n1_c128",
             "gat_n0_c128_h4", "gat_n0_c162", "gat_n1_wide"]
GRAD_NAMES = ["gatgrad_n0_h2", "gatgrad_n1_h2", "gatgrad_n1_h8_b2", "gatgrad_n0_src"]

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 12, 'block': 'constant', 'function': 'GAT', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'step_size': 1, 'max_nfe': 1000,
       'multi_modal': False, 'mix_features': False, 'attention_dim': 16}


def load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


def rhs(d, m, v=None):
    v = v or {}
    g = lambda k: v[k] if k in v else d[k]  # noqa: E731
    return G.gat_rhs(d["edge_index"], g("x"), d["x0"], g("W"), g("a"), m["heads"], m["attention_norm_idx"],
                     m["leaky_relu_slope"], float(g("alpha_train")), float(g("beta_train")),
                     add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"])


def test_every_fixture_of_the_issue_is_present():
    assert sorted(os.path.basename(p)[:-4] for p in GAT) == sorted(FWD_NAMES)
    assert sorted(os.path.basename(p)[:-4] for p in GATGRAD) == sorted(GRAD_NAMES)
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as fh:  # the directory's own manifest
        assert sorted(json.load(fh)) == sorted(FWD_NAMES + GRAD_NAMES)
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))) == \
        sorted(FWD_NAMES + GRAD_NAMES)
    for p in GAT + GATGRAD:
        assert os.path.getsize(p) < 1 << 20
        d, m = load(p)
        assert m["kind"] == ("gat_grad" if os.path.basename(p).startswith("gatgrad_") else "gat")
        assert "leaky_relu_slope" in m and d["a"].ndim == 1 and d["a"].shape[0] == 2 * m["attention_dim"] // m["heads"]


@pytest.mark.parametrize("path", GAT, ids=os.path.basename)
def test_restatement_matches_reference(path):
    d, m = load(path)
    f = rhs(d, m)
    assert f.shape == d["f"].shape
    assert rel(f, d["f"]) <= 1e-12
    att = G.gat_attention(d["x"], d["edge_index"], d["W"], d["a"], m["heads"], m["attention_norm_idx"],
                          m["leaky_relu_slope"])
    assert att.shape == d["attention"].shape
    assert np.abs(att - d["attention"]).max() <= 1e-12
    # utils.softmax: every non-empty group of edge_index[norm_idx] sums to 1
    ei = d["edge_index"]
    for b in range(ei.shape[0]):
        sums = np.zeros((m["N"], m["heads"]))
        np.add.at(sums, ei[b, m["attention_norm_idx"]], att[b])
        live = np.unique(ei[b, m["attention_norm_idx"]])
        assert np.abs(sums[live] - 1.0).max() <= 1e-12


def test_wide_fixture_reaches_its_score_range():
    d, m = load(os.path.join(GOLDEN, "gat_n1_wide.npz"))
    t = np.abs(G.gat_preact(d["x"], d["edge_index"], d["W"], d["a"], m["heads"])).max()
    assert 25.0 <= t <= 35.0


@pytest.mark.parametrize("path", GATGRAD, ids=os.path.basename)
def test_grad_fixture_is_the_restatement_derivative(path):
    """The reference-autograd gradients agree with central differences of the
    restatement along random directions (method and bar of
    test_oracle_golden.py::test_grad_fixture_is_the_oracle_derivative).  The step
    keeps every LeakyReLU pre-activation on its side of the kink: the fixtures hold
    |pre-activation| >= 1e-4 and the step moves none by that much."""
    d, m = load(path)
    rng = np.random.default_rng(3)
    gout = d["gout"].astype(np.float64)
    base = {k: d[k].astype(np.float64) for k in ("x", "alpha_train", "beta_train", "W", "a")}
    pre0 = G.gat_preact(base["x"], d["edge_index"], base["W"], base["a"], m["heads"])
    assert np.abs(pre0).min() >= 1e-4 and abs(np.abs(pre0).min() - m["preact_min"]) <= 1e-12
    assert rel(rhs(d, m), d["f"]) <= 1e-12

    def loss(v):
        return float((rhs(d, m, v) * gout).sum())

    for name in base:
        g = d["g_" + name].astype(np.float64)
        assert g.shape == np.shape(base[name])
        u = rng.standard_normal(np.shape(base[name]))
        eps = 1e-6 * max(1.0, float(np.abs(base[name]).max()))
        vp, vm = dict(base), dict(base)
        vp[name] = base[name] + eps * u
        vm[name] = base[name] - eps * u
        for v in (vp, vm):
            moved = G.gat_preact(v["x"], d["edge_index"], v["W"], v["a"], m["heads"]) - pre0
            assert np.abs(moved).max() < 1e-4
        fd = (loss(vp) - loss(vm)) / (2 * eps)
        an = float((g * u).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)) + 1e-7 * float(np.abs(g).sum()), (name, fd, an)


def test_registry_switch():
    assert gnpde.set_function(dict(OPT, gnpde_gat=True)) is gnpde.ODEFuncAtt
    with pytest.raises(NotImplementedError, match="gnpde_gat"):
        gnpde.set_function(dict(OPT))
    with pytest.raises(NotImplementedError, match="gnpde_gat"):
        gnpde.set_function(dict(OPT, gnpde_gat=False))


def test_layer_parameters():
    func = gnpde.ODEFuncAtt(12, 12, dict(OPT), None)
    lay = func.multihead_att_layer
    assert isinstance(lay, gnpde.SpGraphAttentionLayer)
    names = dict(lay.named_parameters())
    assert sorted(names) == ["W", "Wout", "a"]
    assert tuple(lay.W.shape) == (12, 16) and tuple(lay.Wout.shape) == (16, 12) and tuple(lay.a.shape) == (1, 16, 1, 1)
    assert (lay.alpha, lay.h, lay.d_k, lay.attention_dim) == (0.2, 2, 8, 16)
    assert all(float(p.detach().abs().max()) > 0 for p in names.values())  # xavier_normal_, not zeros
    keys = set(func.state_dict())
    assert {"alpha_train", "beta_train", "multihead_att_layer.W", "multihead_att_layer.Wout",
            "multihead_att_layer.a"} <= keys
    assert repr(func) == "ODEFuncAtt (12 -> 12)" and repr(lay) == "SpGraphAttentionLayer (12 -> 12)"
    assert not func.supports_node_layout() and not func.supports_feature_padding()
    # attention_dim defaults to out_features
    opt = {k: v for k, v in OPT.items() if k != 'attention_dim'}
    assert tuple(gnpde.SpGraphAttentionLayer(6, 8, opt, None).W.shape) == (6, 8)


def test_fold_is_the_score_decomposition():
    """[sl | sr] = x U with U = W folded with a: the pre-activation of every edge."""
    from gnpde.function_GAT_attention import fold
    d, m = load(os.path.join(GOLDEN, "gat_n1_h8_b2.npz"))
    U = fold(torch.from_numpy(d["W"]), torch.from_numpy(d["a"]), m["heads"]).numpy()
    sp = d["x"].astype(np.float64) @ U
    h = m["heads"]
    b = np.arange(m["B"])[:, None]
    pre = sp[b, d["edge_index"][:, 0], :h] + sp[b, d["edge_index"][:, 1], h:]
    assert np.abs(pre - G.gat_preact(d["x"], d["edge_index"], d["W"], d["a"], h)).max() <= 1e-13


@pytest.mark.parametrize("key", ["mix_features", "multi_modal"])
def test_unsupported_settings_raise(key):
    with pytest.raises(NotImplementedError):
        gnpde.ODEFuncAtt(12, 12, dict(OPT, **{key: True}), None)
    with pytest.raises(NotImplementedError):
        gnpde.SpGraphAttentionLayer(12, 12, dict(OPT, **{key: True}), None)
