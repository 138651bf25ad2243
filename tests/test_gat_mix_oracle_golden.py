"""Pins the mix_features restatement (tests/gat_mix_oracle.py) against the reference's own
float64 run of src/function_GAT_attention.py with mix_features=True
(tests/golden/gat_mix/gatmix_*.npz, gatmixgrad_*.npz, made by
tests/golden/gen_golden_gat_mix.py), and the host side of the feature: the opt-in key,
the settings that still raise and the unchanged state_dict."""
import glob
import json
import os

import numpy as np
import pytest

import gat_mix_oracle as M
import gat_oracle as G
import gnpde
from conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "gat_mix")  # a directory of its own, with its own MANIFEST.json

MIX = sorted(glob.glob(os.path.join(GOLDEN, "gatmix_*.npz")))
MIXGRAD = sorted(glob.glob(os.path.join(GOLDEN, "gatmixgrad_*.npz")))
# (B, N, E, C, heads, attention_dim, attention_norm_idx) of every forward case
FWD_CASES = {
    "gatmix_n0_h2": (1, 40, 160, 12, 2, 8, 0),
    "gatmix_n1_h8_b2": (2, 33, 150, 16, 8, 16, 1),
    "gatmix_n1_c128_h4": (1, 70, 400, 128, 4, 64, 1),
    "gatmix_n0_c128_a128": (1, 70, 400, 128, 2, 128, 0),
    "gatmix_n0_c162": (1, 45, 200, 162, 4, 48, 0),
    "gatmix_n1_c80_a20": (1, 45, 200, 80, 4, 20, 1),
    "gatmix_n1_h1_b3": (3, 37, 120, 64, 1, 16, 1),
}
GRAD_NAMES = ["gatmixgrad_n0_h2", "gatmixgrad_n1_h2", "gatmixgrad_n1_h8_b2", "gatmixgrad_n0_src"]
LARGEST_GAT_FIXTURE = max(os.path.getsize(p) for p in glob.glob(os.path.join(_GOLDEN, "gat", "*.npz")))

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 12, 'block': 'constant', 'function': 'GAT', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'step_size': 1, 'max_nfe': 1000,
       'multi_modal': False, 'mix_features': True, 'attention_dim': 16}


def load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


def rhs(d, m, v=None):
    v = v or {}
    g = lambda k: v[k] if k in v else d[k]  # noqa: E731
    return M.gat_mix_rhs(d["edge_index"], g("x"), d["x0"], g("W"), g("Wout"), g("a"), m["heads"],
                         m["attention_norm_idx"], m["leaky_relu_slope"], float(g("alpha_train")),
                         float(g("beta_train")), add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"])


def test_every_fixture_of_the_issue_is_present():
    assert sorted(os.path.basename(p)[:-4] for p in MIX) == sorted(FWD_CASES)
    assert sorted(os.path.basename(p)[:-4] for p in MIXGRAD) == sorted(GRAD_NAMES)
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as fh:
        assert sorted(json.load(fh)) == sorted(list(FWD_CASES) + GRAD_NAMES)
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))) == \
        sorted(list(FWD_CASES) + GRAD_NAMES)
    flags = set()
    for p in MIX + MIXGRAD:
        assert os.path.getsize(p) <= LARGEST_GAT_FIXTURE
        d, m = load(p)
        name = os.path.basename(p)[:-4]
        assert m["kind"] == ("gat_mix_grad" if name.startswith("gatmixgrad_") else "gat_mix")
        assert d["Wout"].shape == d["W"].shape[::-1] == (m["attention_dim"], m["C"])
        assert d["wx"].shape == (m["B"], m["N"], m["attention_dim"])
        if name in FWD_CASES:
            assert (m["B"], m["N"], m["E"], m["C"], m["heads"], m["attention_dim"], m["attention_norm_idx"]) == \
                FWD_CASES[name]
            flags.add((m["add_source"], m["no_alpha_sigmoid"]))
            # the reference's own fp32 run stays well inside the project's 1e-5 bar
            assert rel(d["f_ref32"], d["f"]) <= 2e-6 and abs(rel(d["f_ref32"], d["f"]) - m["ref32_dev"]) <= 1e-12
        else:
            assert "g_Wout" in d.files and d["g_Wout"].shape == d["Wout"].shape and np.abs(d["g_Wout"]).max() > 0
    assert len(flags) >= 3  # add_source and no_alpha_sigmoid both vary
    assert any(c[6] == 0 for c in FWD_CASES.values()) and any(c[6] == 1 for c in FWD_CASES.values())


@pytest.mark.parametrize("path", MIX + MIXGRAD, ids=os.path.basename)
def test_restatement_matches_reference(path):
    d, m = load(path)
    f = rhs(d, m)
    assert f.shape == d["f"].shape
    assert rel(f, d["f"]) <= 1e-12
    assert rel(M.gat_mix_project(d["x"], d["W"]), d["wx"]) <= 1e-12
    att = G.gat_attention(d["x"], d["edge_index"], d["W"], d["a"], m["heads"], m["attention_norm_idx"],
                          m["leaky_relu_slope"])
    assert np.abs(att - d["attention"]).max() <= 1e-12


@pytest.mark.parametrize("path", MIX, ids=os.path.basename)
def test_head_mean_commutes_with_the_product(path):
    """Every head's attention multiplies the whole wx, so f = a ((A_mean (x W)) Wout - x) + b x0
    with the head-mean attention: the form the project's kernels compute."""
    import gnpde_oracle as O
    d, m = load(path)
    z = O.aggregate(d["edge_index"], d["attention"].mean(axis=2), d["wx"])
    f = O.rhs_epilogue(z @ d["Wout"].astype(np.float64), d["x"], d["x0"], float(d["alpha_train"]),
                       float(d["beta_train"]), m["add_source"], m["no_alpha_sigmoid"])
    assert rel(f, d["f"]) <= 1e-12


@pytest.mark.parametrize("path", MIXGRAD, ids=os.path.basename)
def test_grad_fixture_is_the_restatement_derivative(path):
    """The reference-autograd gradients (Wout included) agree with central differences of
    the restatement along random directions: method and bar of
    test_gat_oracle_golden.py::test_grad_fixture_is_the_restatement_derivative."""
    d, m = load(path)
    rng = np.random.default_rng(3)
    gout = d["gout"].astype(np.float64)
    base = {k: d[k].astype(np.float64) for k in ("x", "alpha_train", "beta_train", "W", "a", "Wout")}
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


def test_mix_features_is_opt_in():
    for make in (gnpde.ODEFuncAtt, gnpde.SpGraphAttentionLayer):
        with pytest.raises(NotImplementedError, match="gnpde_gat_mix_features"):
            make(12, 12, dict(OPT), None)
        with pytest.raises(NotImplementedError, match="gnpde_gat_mix_features"):
            make(12, 12, dict(OPT, gnpde_gat_mix_features=False), None)
    func = gnpde.ODEFuncAtt(12, 12, dict(OPT, gnpde_gat_mix_features=True), None)
    assert func.multihead_att_layer.mix
    # the key alone changes nothing: mix_features=False stays the aggregation of x
    plain = gnpde.ODEFuncAtt(12, 12, dict(OPT, mix_features=False, gnpde_gat_mix_features=True), None)
    assert not plain.multihead_att_layer.mix


def test_multi_modal_still_raises():
    for make in (gnpde.ODEFuncAtt, gnpde.SpGraphAttentionLayer):
        with pytest.raises(NotImplementedError, match="multi_modal"):
            make(12, 12, dict(OPT, gnpde_gat_mix_features=True, multi_modal=True), None)


def test_state_dict_keys_unchanged():
    mix = gnpde.ODEFuncAtt(12, 12, dict(OPT, gnpde_gat_mix_features=True), None)
    plain = gnpde.ODEFuncAtt(12, 12, dict(OPT, mix_features=False), None)
    assert list(mix.state_dict()) == list(plain.state_dict())
    assert sorted(dict(mix.multihead_att_layer.named_parameters())) == ["W", "Wout", "a"]
    assert tuple(mix.multihead_att_layer.Wout.shape) == (16, 12)
    plain.load_state_dict(mix.state_dict())


def test_bf16_state_is_rejected_before_any_kernel():
    import torch
    func = gnpde.ODEFuncAtt(12, 12, dict(OPT, gnpde_gat_mix_features=True), None)
    with pytest.raises(NotImplementedError, match="fp32"):
        func.multihead_att_layer.project(torch.zeros(1, 4, 12, dtype=torch.bfloat16))
