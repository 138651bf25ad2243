"""Pins the beltrami exp_kernel restatement (tests/beltrami_oracle.py) against the fixtures of
tests/golden/beltrami/ (the reference layer's own Qx / Kx / Qp / Kp modules, utils.softmax /
utils.squareplus, multiply_attention and epilogue in float64, the slice and the score written
from the formula; made by tests/golden/gen_golden_beltrami.py), the folding identity the GPU
path rests on, and the closed forms of the gradients the new kernel and its caller compute."""
import json
import os

import numpy as np
import pytest
import torch

import beltrami_oracle as BO
from conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "beltrami")
with open(os.path.join(GOLDEN, "meta.json")) as _fh:
    META = json.load(_fh)
CASES = sorted(META["cases"])
GRAD_CASES = [n for n in CASES if META["cases"][n]["has_grad"]]


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


def test_the_cases_of_the_issue_are_present():
    assert CASES == sorted(["team_n0", "team_n1", "labels", "lane", "wide", "hub", "sp_n0", "sp_n1", "src"])
    assert sorted(GRAD_CASES) == sorted(["team_n0", "team_n1", "labels", "lane", "hub", "sp_n0", "sp_n1"])
    want = dict(team_n0=(1, 6, 5, 0, 2, 8, 0), team_n1=(1, 6, 5, 0, 2, 8, 1), labels=(1, 6, 5, 3, 2, 8, 1),
                lane=(2, 4, 3, 0, 1, 6, 0), wide=(1, 8, 8, 0, 8, 128, 1), hub=(1, 6, 5, 0, 2, 8, 1),
                sp_n0=(1, 6, 5, 0, 2, 8, 0), sp_n1=(1, 6, 5, 0, 2, 8, 1), src=(1, 6, 5, 0, 2, 8, 1))
    for name in CASES:
        d, m = load(name)
        assert m == META["cases"][name]
        assert (m["B"], m["F"], m["P"], m["labels"], m["heads"], m["attention_dim"],
                m["attention_norm_idx"]) == want[name]
        assert m["C"] == m["F"] + m["P"] + m["labels"] and m["N"] <= 64 and m["E"] <= 600
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 100 << 10
        assert m["square_plus"] == name.startswith("sp_")
        assert (m["add_source"], m["no_alpha_sigmoid"]) == ((True, True) if name == "src" else (False, False))
        # distinct scalars: swapping or merging any two of them changes the result
        assert len({m[s] for s in BO.SNAMES}) == 4
        assert [m[s] for s in BO.SNAMES] == [float(np.float32(v)) for v in (1.6, 0.7, 1.5, 1.9)]
        # the generator's two conditions
        assert m["fp32_attention_err"] <= META["fp32_bar"] == 3e-6 and m["fp32_f_rel_err"] <= 3e-6
        assert m["score_span"] >= META["span_min"] == 10.0 and m["attention_span"] >= 2.0
        for n in BO.PNAMES:  # random parameters, not the constant 1e-5 init
            assert np.unique(d[n]).size > 1 and np.abs(d[n]).max() > 0.05
        assert d["Wqx"].shape == (m["attention_dim"], m["C"] - m["P"]) and d["Wkp"].shape == (m["attention_dim"], m["P"])
    # the team pair and the squareplus pair share their graph across norm_idx
    assert np.array_equal(load("team_n0")[0]["edge_index"], load("team_n1")[0]["edge_index"])
    # hub: one destination with 300 in-edges, one node with no edge at all
    d, m = load("hub")
    e = d["edge_index"][0]
    assert np.bincount(e[1], minlength=m["N"]).max() >= 300
    assert np.setdiff1d(np.arange(m["N"]), e.reshape(-1)).size >= 1


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference(name):
    d, m = load(name)
    f, att, s = BO.fixture_rhs(d)
    assert rel(s, d["prods"]) <= 1e-12
    assert np.abs(att - d["attention"]).max() <= 1e-12
    assert rel(f, d["f"]) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_folding_identity(name):
    """|qx-kx|^2/(2 lsx^2) + |qp-kp|^2/(2 lsp^2) = |q'-k'|^2 / 2: one exp_kernel of width 2 dk,
    amplitude ovx ovp and lengthscale 1 is the product of the two kernels."""
    d, m = load(name)
    _, kw = BO.fixture_args(d)
    a = {k: kw[k] for k in ("W", "heads", "F", "P", "ovx", "lsx", "ovp", "lsp")}
    lit = BO.scores(d["x"], d["edge_index"], **a)
    fold = BO.scores_folded(d["x"], d["edge_index"], **a)
    assert rel(fold, lit) <= 1e-13
    # swapping the two lengthscales is another function (the scalars discriminate)
    a2 = dict(a, lsx=a["lsp"], lsp=a["lsx"])
    assert rel(BO.scores(d["x"], d["edge_index"], **a2), lit) > 1e-2


@pytest.mark.parametrize("name", ["team_n1", "labels", "sp_n1"])
def test_scalar_gradients_are_the_finite_differences(name):
    """The four stored scalar gradients against central differences of <gout, f> in float64."""
    d, m = load(name)
    key = dict(output_var_x="ovx", lengthscale_x="lsx", output_var_p="ovp", lengthscale_p="lsp")
    for s in BO.SNAMES:
        h = 1e-6
        lo = (BO.fixture_rhs(d, **{key[s]: m[s] - h})[0] * d["gout"]).sum()
        hi = (BO.fixture_rhs(d, **{key[s]: m[s] + h})[0] * d["gout"]).sum()
        want = float(d["g_" + s].reshape(-1)[0])
        assert abs((hi - lo) / (2 * h) - want) <= 1e-6 * max(abs(want), 1e-3), s


@pytest.mark.parametrize("H,dk,dks", [(2, 8, 4), (1, 12, 6), (3, 10, 3)])
def test_score_grad_split_closed_form_is_the_autograd_gradient(H, dk, dks):
    """The oracle of ops.score_grad_split against float64 autograd, and the caller's formulas
    g_ovx = ovp S0, g_ovp = ovx S0, g_lsx = S1 / lsx, g_lsp = S2 / lsp for operands that are
    projections divided by their lengthscale."""
    rng = np.random.default_rng(H * 100 + dk)
    N, E = 12, 70
    ei = rng.integers(0, N, size=(2, E))
    qx, kx = rng.standard_normal((2, N, H, dks)) * 0.5
    qp, kp = rng.standard_normal((2, N, H, dk - dks)) * 0.5
    gs = rng.standard_normal((E, H))
    ovx, lsx, ovp, lsp = 1.6, 0.7, 1.5, 1.9
    t = {n: torch.tensor(v, dtype=torch.float64, requires_grad=True) for n, v in
         dict(qx=qx, kx=kx, qp=qp, kp=kp, ovx=ovx, lsx=lsx, ovp=ovp, lsp=lsp).items()}
    src, dst = torch.from_numpy(ei)
    s = t["ovx"] ** 2 * torch.exp(-((t["qx"][src] - t["kx"][dst]) ** 2).sum(-1) / (2 * t["lsx"] ** 2)) * \
        t["ovp"] ** 2 * torch.exp(-((t["qp"][src] - t["kp"][dst]) ** 2).sum(-1) / (2 * t["lsp"] ** 2))
    (s * torch.from_numpy(gs)).sum().backward()
    q = np.concatenate([qx / lsx, qp / lsp], axis=2).reshape(N, H * dk)
    k = np.concatenate([kx / lsx, kp / lsp], axis=2).reshape(N, H * dk)
    gq, gk, S0, S1, S2 = BO.score_grad_split(ei, q, k, gs, H, dk, dks, ovx * ovp)
    g = {n: v.grad.numpy() for n, v in t.items()}
    assert abs(ovp * S0 - g["ovx"]) <= 1e-12 * abs(g["ovx"]) and abs(ovx * S0 - g["ovp"]) <= 1e-12 * abs(g["ovp"])
    assert abs(S1 / lsx - g["lsx"]) <= 1e-12 * abs(g["lsx"]) and abs(S2 / lsp - g["lsp"]) <= 1e-12 * abs(g["lsp"])
    gq4, gk4 = gq.reshape(N, H, dk), gk.reshape(N, H, dk)
    assert rel(gq4[:, :, :dks] / lsx, g["qx"]) <= 1e-12 and rel(gq4[:, :, dks:] / lsp, g["qp"]) <= 1e-12
    assert rel(gk4[:, :, :dks] / lsx, g["kx"]) <= 1e-12 and rel(gk4[:, :, dks:] / lsp, g["kp"]) <= 1e-12
    # another split is another pair of sums
    _, _, _, T1, _ = BO.score_grad_split(ei, q, k, gs, H, dk, dks + 1, ovx * ovp)
    assert abs(T1 - S1) > 1e-3 * abs(S1)
