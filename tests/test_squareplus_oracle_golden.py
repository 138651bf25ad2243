"""Pins the oracle's squareplus normalisation (oracle/gnpde_oracle.py: squareplus,
transformer_attention / transformer_rhs with square_plus=True) and the fixtures of
tests/golden/squareplus/ (made by tests/golden/gen_golden_squareplus.py from the reference's
own prods, utils.squareplus and multiply_attention in float64) to each other: forward to
fp64 rounding, the stored autograd gradients against central differences of the oracle."""
import glob
import json
import os

import numpy as np
import pytest

import gnpde_oracle as O
from conftest import GOLDEN as _GOLDEN

# a directory with its own MANIFEST.json: tests/golden/MANIFEST.json lists tests/golden/*.npz
GOLDEN = os.path.join(_GOLDEN, "squareplus")
FWD = sorted(glob.glob(os.path.join(GOLDEN, "sp_*.npz")))
GRAD = sorted(glob.glob(os.path.join(GOLDEN, "spgrad_*.npz")))
FWD_NAMES = ["sp_sd_n0_h2", "sp_sd_n1_h2", "sp_sd_n1_h1", "sp_sd_n1_h8_b3", "sp_sd_n1_src", "sp_sd_n1_c128",
             "sp_sd_n1_c162", "sp_sd_n1_wide", "sp_pe_n0_h2", "sp_pe_n1_h2", "sp_pe_n0_nosig", "sp_pe_n1_c128_h8",
             "sp_exp_kernel_n0", "sp_exp_kernel_n1", "sp_cosine_sim_n0", "sp_cosine_sim_n1", "sp_pearson_n0",
             "sp_pearson_n1"]
GRAD_NAMES = ["spgrad_sd_n0_h2", "spgrad_sd_n1_h2", "spgrad_sd_n1_h8_b2", "spgrad_sd_n1_src", "spgrad_pe_n0",
              "spgrad_pe_n1", "spgrad_exp_kernel_n0", "spgrad_exp_kernel_n1", "spgrad_cosine_sim_n0",
              "spgrad_cosine_sim_n1", "spgrad_pearson_n0", "spgrad_pearson_n1"]
PARAMS = ("x", "alpha_train", "beta_train", "Wq", "bq", "Wk", "bk")


def load(path):
    d = np.load(path, allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30)


def _kw(m, v):
    kw = dict(attention_type=m["attention_type"], score_mode=m["score_mode"])
    if m["attention_type"] == "exp_kernel":
        kw.update(output_var=float(v.get("output_var", m["output_var"])),
                  lengthscale=float(v.get("lengthscale", m["lengthscale"])))
    return kw


def attention(d, m, v=None):
    v = v or {}
    g = lambda k: v[k] if k in v else d[k]  # noqa: E731
    return O.transformer_attention(g("x"), d["edge_index"], g("Wq"), g("bq"), g("Wk"), g("bk"), m["heads"],
                                   m["attention_norm_idx"], square_plus=True, **_kw(m, v))


def rhs(d, m, v=None):
    v = v or {}
    g = lambda k: v[k] if k in v else d[k]  # noqa: E731
    return O.transformer_rhs(d["edge_index"], g("x"), d["x0"], g("Wq"), g("bq"), g("Wk"), g("bk"), m["heads"],
                             m["attention_norm_idx"], float(g("alpha_train")), float(g("beta_train")),
                             add_source=m["add_source"], no_alpha_sigmoid=m["no_alpha_sigmoid"], square_plus=True,
                             **_kw(m, v))


def scores(d, m, v=None):
    v = v or {}
    g = lambda k: v[k] if k in v else d[k]  # noqa: E731
    kw = _kw(m, v)
    return O.attention_scores(g("x"), d["edge_index"], g("Wq"), g("bq"), g("Wk"), g("bk"), m["heads"],
                              kw.pop("attention_type"), kw.pop("score_mode"), **kw)


def test_every_fixture_of_the_issue_is_present():
    assert sorted(os.path.basename(p)[:-4] for p in FWD) == sorted(FWD_NAMES)
    assert sorted(os.path.basename(p)[:-4] for p in GRAD) == sorted(GRAD_NAMES)
    with open(os.path.join(GOLDEN, "MANIFEST.json")) as fh:
        assert sorted(json.load(fh)) == sorted(FWD_NAMES + GRAD_NAMES)
    gat = glob.glob(os.path.join(_GOLDEN, "gat", "*.npz"))
    cap = max(os.path.getsize(p) for p in gat)
    for p in FWD + GRAD:
        assert os.path.getsize(p) <= cap  # no file larger than the largest GAT fixture
        d, m = load(p)
        assert m["kind"] == ("squareplus_grad" if os.path.basename(p).startswith("spgrad_") else "squareplus")
        assert m["square_plus"] is True and m["C"] in (16, 128, 162) and m["heads"] in (1, 2, 4, 8)
        assert 40 <= m["N"] <= 300
    assert {load(p)[1]["heads"] for p in FWD} >= {1, 2, 8}
    assert {load(p)[1]["C"] for p in FWD} == {16, 128, 162}
    assert sum(load(p)[1]["add_source"] for p in FWD) == 1 and sum(load(p)[1]["no_alpha_sigmoid"] for p in FWD) == 1


@pytest.mark.parametrize("path", FWD, ids=os.path.basename)
def test_oracle_matches_reference(path):
    """fp64 rounding of THIS function: reference and oracle both evaluate the literal
    (t + sqrt(t^2 + 4)) / 2, whose sum cancels — sqrt(t^2 + 4) carries eps |t| absolute
    against a result of ~1/|t|, a relative eps t^2 — on scores that the two form in
    different orders.  Bar: 1e-12 + 8 eps max(t^2) (attention <= 1; 1.8e-9 at the widest
    fixture, |t| up to ~1,500)."""
    d, m = load(path)
    s = scores(d, m)
    tmax = float(np.abs(s - s.max(axis=(1, 2), keepdims=True)).max())
    bar = 1e-12 + 8 * np.finfo(np.float64).eps * tmax * tmax
    att = attention(d, m)
    assert att.shape == d["attention"].shape
    assert np.abs(att - d["attention"]).max() <= bar
    assert rel(rhs(d, m), d["f"]) <= bar
    # every non-empty group sums to 1, and the stored maxima are the scores' own
    ei, ni = d["edge_index"], m["attention_norm_idx"]
    for b in range(ei.shape[0]):
        sums = np.zeros((m["N"], m["heads"]))
        np.add.at(sums, ei[b, ni], att[b])
        assert np.abs(sums[np.unique(ei[b, ni])] - 1.0).max() <= 1e-12
        assert abs(s[b].max() - m["M"][b]) <= 1e-10 * max(1.0, abs(m["M"][b]))


def test_uniform_case_is_one_over_outdegree():
    """Fork scaled_dot, source groups: every score of a group is equal, att = p / (d p + 1e-16)."""
    d, m = load(os.path.join(GOLDEN, "sp_sd_n0_h2.npz"))
    ei = d["edge_index"]
    deg = np.bincount(ei[0, 0], minlength=m["N"])
    assert np.abs(d["attention"][0] - (1.0 / deg[ei[0, 0]])[:, None]).max() <= 1e-12


def test_batch_fixture_has_distinct_maxima():
    """A maximum taken across the batch instead of per element changes the result."""
    d, m = load(os.path.join(GOLDEN, "sp_sd_n1_h8_b3.npz"))
    M = sorted(m["M"])
    assert m["B"] == 3 and min(b - a for a, b in zip(M, M[1:])) >= 1.0
    s = scores(d, m)
    t = s - s.max()  # the wrong shift: one maximum for the whole batch
    p = 2.0 / (np.sqrt(t * t + 4.0) - t)
    wrong = np.empty_like(p)
    for b in range(3):
        sm = np.zeros((m["N"], m["heads"]))
        np.add.at(sm, d["edge_index"][b, 1], p[b])
        wrong[b] = p[b] / (sm[d["edge_index"][b, 1]] + 1e-16)
    assert np.abs(wrong - d["attention"]).max() > 2e-5


def test_wide_fixture_tells_the_two_formulas_apart():
    """Node scores of std ~ 50: the literal (t + sqrt(t^2 + 4)) / 2 in float32 misses the
    2e-5 attention bar, the form 2 / (sqrt(t^2 + 4) - t) in float32 holds it."""
    d, m = load(os.path.join(GOLDEN, "sp_sd_n1_wide.npz"))
    s = scores(d, m)
    assert 40.0 <= s.std() <= 60.0
    ei = d["edge_index"]
    t = (s - s.max(axis=(1, 2), keepdims=True)).astype(np.float32)

    def normalise(p):
        sm = np.zeros((m["N"], m["heads"]), np.float32)
        np.add.at(sm, ei[0, 1], p[0])
        return p / (sm[ei[0, 1]] + np.float32(1e-16))

    literal = normalise((t + np.sqrt(t * t + np.float32(4))) / np.float32(2))
    stable = normalise(np.float32(2) / (np.sqrt(t * t + np.float32(4)) - t))
    assert np.abs(literal.astype(np.float64) - d["attention"]).max() > 2e-5
    assert np.abs(stable.astype(np.float64) - d["attention"]).max() <= 2e-6
    assert abs(np.abs(literal.astype(np.float64) - d["attention"]).max() - m["literal_fp32_attention_err"]) <= 1e-9


@pytest.mark.parametrize("path", GRAD, ids=os.path.basename)
def test_grad_fixture_is_the_oracle_derivative(path):
    """The stored fp64 autograd gradients agree with central differences of the oracle along
    random directions (method and bar of test_oracle_golden.py).  The maximum of every batch
    element leads the next distinct score by at least 1e-3 (meta max_margin) and the step
    moves no score by that much, so the arg-max does not change inside the difference."""
    d, m = load(path)
    rng = np.random.default_rng(5)
    gout = d["gout"].astype(np.float64)
    names = list(PARAMS)
    base = {k: d[k].astype(np.float64) for k in names}
    if m["attention_type"] == "exp_kernel":
        base.update(output_var=np.float64(m["output_var"]), lengthscale=np.float64(m["lengthscale"]))
        names += ["output_var", "lengthscale"]
    assert min(m["max_margin"]) >= 1e-3
    s0 = scores(d, m, base)
    tmax = float(np.abs(s0 - s0.max(axis=(1, 2), keepdims=True)).max())
    assert rel(rhs(d, m), d["f"]) <= 1e-12 + 8 * np.finfo(np.float64).eps * tmax * tmax  # test_oracle_matches_reference

    def loss(v):
        return float((rhs(d, m, v) * gout).sum())

    for name in names:
        g = d["g_" + name].astype(np.float64).reshape(np.shape(base[name]))
        u = rng.standard_normal(np.shape(base[name]))
        eps = 1e-6 * max(1.0, float(np.abs(base[name]).max()))
        vp, vm = dict(base), dict(base)
        vp[name] = base[name] + eps * u
        vm[name] = base[name] - eps * u
        for v in (vp, vm):
            assert np.abs(scores(d, m, v) - s0).max() < 0.5 * min(m["max_margin"])
        fd = (loss(vp) - loss(vm)) / (2 * eps)
        an = float((g * u).sum())
        assert abs(fd - an) <= 1e-6 * max(1.0, abs(an)) + 1e-7 * float(np.abs(g).sum()), (name, fd, an)
