"""Host side of the beltrami exp_kernel attention (opt['beltrami'], attention_type 'exp_kernel',
opt['gnpde_beltrami_kernel']): the opt-in key and what still raises, the reference's parameter
names, the folded projection operand (built on the CPU by the function the GPU path uses)
against the float64 oracle, its cache, and the refusals of what is out of scope."""
import json
import os

import numpy as np
import pytest
import torch

import beltrami_oracle as BO
import gnpde
import gnpde.function_transformer_attention as fta
from conftest import GOLDEN as _GOLDEN

GOLDEN = os.path.join(_GOLDEN, "beltrami")
with open(os.path.join(GOLDEN, "meta.json")) as _fh:
    META = json.load(_fh)
CASES = sorted(META["cases"])

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 11, 'feat_hidden_dim': 6, 'pos_enc_hidden_dim': 5, 'block': 'constant',
       'function': 'transformer', 'augment': False, 'adjoint': False, 'tol_scale': 1, 'time': 1, 'method': 'euler',
       'no_alpha_sigmoid': False, 'step_size': 1, 'max_nfe': 1000, 'multi_modal': False, 'mix_features': False,
       'attention_dim': 8, 'attention_type': 'exp_kernel', 'beltrami': True, 'square_plus': False,
       'reweight_attention': False, 'data_norm': 'rw', 'max_iters': 1000}
KEY = dict(gnpde_beltrami_kernel=True)
MAKERS = (gnpde.ODEFuncTransformerAtt, gnpde.SpGraphTransAttentionLayer)


def load(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return d, json.loads(str(d["meta"]))


def layer_from(d, m, dtype=torch.float32):
    opt = dict(OPT, hidden_dim=m["C"], feat_hidden_dim=m["F"], pos_enc_hidden_dim=m["P"], heads=m["heads"],
               attention_dim=m["attention_dim"], attention_norm_idx=m["attention_norm_idx"], **KEY)
    lay = gnpde.SpGraphTransAttentionLayer(m["C"], m["C"], opt, None).to(dtype)
    with torch.no_grad():
        for lin, w, b in ((lay.Qx, "Wqx", "bqx"), (lay.Kx, "Wkx", "bkx"), (lay.Qp, "Wqp", "bqp"),
                          (lay.Kp, "Wkp", "bkp")):
            lin.weight.copy_(torch.from_numpy(d[w]))
            lin.bias.copy_(torch.from_numpy(d[b]))
        for s in BO.SNAMES:
            getattr(lay, s).fill_(m[s])
    return lay


# ---------------------------------------------------------------- the key
def test_the_branch_is_opt_in():
    for make in MAKERS:
        for opt in (dict(OPT), dict(OPT, gnpde_beltrami_kernel=False)):
            with pytest.raises(NotImplementedError, match="beltrami") as ei:
                make(11, 11, opt, None)
            assert "gnpde_beltrami_kernel" in str(ei.value)
    func = gnpde.ODEFuncTransformerAtt(11, 11, dict(OPT, **KEY), None)
    lay = func.multihead_att_layer
    assert lay.beltrami_kernel and not lay.mix and lay.uses_wcat() and not lay.is_uniform(0)
    plain = gnpde.ODEFuncTransformerAtt(11, 11, dict(OPT, beltrami=False), None)
    assert func.supports_node_layout() == plain.supports_node_layout() is False
    assert func.supports_feature_padding() == plain.supports_feature_padding() is False
    assert gnpde.set_function(dict(OPT, **KEY)) is gnpde.ODEFuncTransformerAtt
    for blk, cls in (('constant', gnpde.ConstantODEblock), ('attention', gnpde.AttODEblock),
                     ('mixed', gnpde.MixedODEblock), ('hard_attention', gnpde.HardAttODEblock)):
        assert gnpde.set_block(dict(OPT, block=blk, **KEY)) is cls


def test_parameters_carry_the_reference_names_and_init():
    lay = gnpde.SpGraphTransAttentionLayer(11, 11, dict(OPT, **KEY), None)
    assert list(lay.state_dict()) == META["state_dict_keys"]
    assert [n for n, _ in lay.named_parameters()][:4] == list(BO.SNAMES)
    for s in BO.SNAMES:
        assert torch.equal(getattr(lay, s).detach(), torch.ones(1))
    for n, width in (("Qx", 6), ("Vx", 6), ("Kx", 6), ("Qp", 5), ("Vp", 5), ("Kp", 5)):
        lin = getattr(lay, n)
        assert tuple(lin.weight.shape) == (8, width) and bool((lin.weight == 1e-5).all())
        assert lin.bias.abs().max() > 0  # nn.Linear's default bias
    assert tuple(lay.Wout.weight.shape) == (11, 4)
    assert not any(hasattr(lay, n) for n in ("Q", "K", "V", "output_var", "lengthscale"))
    # labels: Qx reads the feature and the label columns, C - P wide
    lab = gnpde.SpGraphTransAttentionLayer(14, 14, dict(OPT, hidden_dim=14, **KEY), None)
    assert tuple(lab.Qx.weight.shape) == (8, 9) and tuple(lab.Qp.weight.shape) == (8, 5)
    assert len(lay.score_parameters()) == 12 and all(p.requires_grad for p in lay.score_parameters())


def test_the_key_alone_changes_nothing():
    for over in (dict(beltrami=False), dict(attention_type='scaled_dot'), dict(beltrami=False,
                                                                               attention_type='scaled_dot')):
        torch.manual_seed(3)
        a = gnpde.ODEFuncTransformerAtt(11, 11, dict(OPT, **over), None)
        torch.manual_seed(3)
        b = gnpde.ODEFuncTransformerAtt(11, 11, dict(OPT, **dict(over, **KEY)), None)
        assert not b.multihead_att_layer.beltrami_kernel
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        lay = b.multihead_att_layer
        want = [lay.Q.weight, lay.Q.bias, lay.K.weight, lay.K.bias]
        if over.get('attention_type', 'exp_kernel') == 'exp_kernel':
            want += [lay.output_var, lay.lengthscale]
        assert len(lay.score_parameters()) == len(want)
        assert all(p is q for p, q in zip(lay.score_parameters(), want))


def test_what_raises_with_the_key():
    for make in MAKERS:
        with pytest.raises(NotImplementedError, match="mix_features"):
            make(11, 11, dict(OPT, mix_features=True, **KEY), None)
        with pytest.raises(NotImplementedError, match="mix_features"):
            make(11, 11, dict(OPT, mix_features=True, gnpde_mix_features=True, **KEY), None)
        with pytest.raises(NotImplementedError, match="multi_modal"):
            make(11, 11, dict(OPT, multi_modal=True, **KEY), None)
        with pytest.raises(NotImplementedError, match="multi_modal"):
            make(11, 11, dict(OPT, multi_modal=True, gnpde_multi_modal=True, second_modality_dim=4, **KEY), None)
        with pytest.raises(ValueError, match="augment"):
            make(12, 12, dict(OPT, **KEY), None)          # in_features != hidden_dim
        with pytest.raises(ValueError, match="feat_hidden_dim"):
            make(11, 11, dict(OPT, feat_hidden_dim=7, **KEY), None)      # F + P > C
        with pytest.raises(ValueError, match="pos_enc_hidden_dim"):
            make(11, 11, dict(OPT, pos_enc_hidden_dim=0, **KEY), None)   # P < 1
        with pytest.raises(ValueError, match="feat_hidden_dim"):
            make(11, 11, dict(OPT, feat_hidden_dim=0, **KEY), None)      # F < 1
        with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
            make(11, 11, dict(OPT, square_plus=True, **KEY), None)
    make(11, 11, dict(OPT, square_plus=True, gnpde_square_plus=True, **KEY), None)
    make(11, 11, dict(OPT, feat_hidden_dim=1, pos_enc_hidden_dim=10, **KEY), None)


def test_sharded_and_early_stop_refuse_the_branch():
    from gnpde import dist
    for cls in (dist.ColumnShardedTransformer, dist.RowShardedTransformer):
        with pytest.raises(NotImplementedError, match="gnpde_beltrami_kernel"):
            cls(torch.zeros(1, 2, 4, dtype=torch.long), 4, 11, None, None, None, None, 2, 0, None,
                beltrami_kernel=True)
    es_opt = dict(OPT, max_test_steps=10, earlystopxT=1)
    with pytest.raises(NotImplementedError, match="gnpde_beltrami_kernel"):
        gnpde.EarlyStopInt(1.0, dict(es_opt, **KEY))
    gnpde.EarlyStopInt(1.0, dict(es_opt, beltrami=False, **KEY))


# ---------------------------------------------------------------- the folded operand
@pytest.mark.parametrize("name", CASES)
def test_folded_operand_against_the_oracle(name):
    d, m = load(name)
    lay = layer_from(d, m)
    W, b = lay.wcat()
    att, C, F, P, H = m["attention_dim"], m["C"], m["F"], m["P"], m["heads"]
    dk = att // H
    assert tuple(W.shape) == (4 * att, C) and tuple(b.shape) == (4 * att,) and W.is_contiguous()
    assert W.dtype == torch.float32 and not W.requires_grad
    # x W'^T + b' = [q' | k'], q'_h = [qx_h / lsx | qp_h / lsp], to fp32 rounding: every term is an
    # fp32 product of O(1) operands summed over at most C <= 16 columns
    got = (torch.from_numpy(d["x"]) @ W.t() + b).double().numpy()
    _, kw = BO.fixture_args(d)
    q, k = BO.folded(d["x"], kw["W"], H, F, P, kw["lsx"], kw["lsp"])
    want = np.concatenate([q, k], axis=-1)
    assert np.abs(got - want).max() <= 4e-6 * max(1.0, np.abs(want).max())
    # the zero pattern is exact: Qx rows never read a positional column, Qp rows nothing else
    W5 = W.view(2, H, 2, dk, C).numpy()
    pcols = np.arange(F, F + P)
    xcols = np.setdiff1d(np.arange(C), pcols)
    assert not W5[:, :, 0][..., pcols].any() and not W5[:, :, 1][..., xcols].any()
    assert np.all(W5[:, :, 0][..., xcols] != 0) and np.all(W5[:, :, 1][..., pcols] != 0)
    # and the entries are the parameters divided by their lengthscale, in fp32
    lsx, lsp = np.float32(m["lengthscale_x"]), np.float32(m["lengthscale_p"])
    assert np.array_equal(W5[0, :, 0][..., xcols].reshape(att, C - P), d["Wqx"] / lsx)
    assert np.array_equal(W5[1, :, 0][..., xcols].reshape(att, C - P), d["Wkx"] / lsx)
    assert np.array_equal(W5[0, :, 1][..., pcols].reshape(att, P), d["Wqp"] / lsp)
    assert np.array_equal(W5[1, :, 1][..., pcols].reshape(att, P), d["Wkp"] / lsp)


def test_labels_case_proves_the_column_map():
    """With labels the feature part's columns are not contiguous: [0,F) and [F+P,C)."""
    d, m = load("labels")
    assert m["labels"] == 3
    W, _ = layer_from(d, m).wcat()
    F, P, C = m["F"], m["P"], m["C"]
    dk = m["attention_dim"] // m["heads"]
    row = W[0]  # head 0, first Qx row
    assert torch.equal(row[:F], torch.from_numpy(d["Wqx"][0, :F] / np.float32(m["lengthscale_x"])))
    assert torch.equal(row[F + P:], torch.from_numpy(d["Wqx"][0, F:] / np.float32(m["lengthscale_x"])))
    assert not row[F:F + P].any()
    assert torch.equal(W[dk][F:F + P], torch.from_numpy(d["Wqp"][0] / np.float32(m["lengthscale_p"])))


def test_folded_operand_follows_parameter_versions():
    d, m = load("team_n1")
    lay = layer_from(d, m)
    W0, b0 = lay.wcat()
    assert lay.wcat()[0] is W0 and lay.wcat()[1] is b0          # cached
    keep = W0.clone()
    with torch.no_grad():
        lay.lengthscale_p.mul_(2.0)
    W1, _ = lay.wcat()
    assert W1 is not W0 and torch.equal(W0, keep)               # a new operand; the old one untouched
    dk = m["attention_dim"] // m["heads"]
    assert torch.equal(W1[:dk], keep[:dk]) and torch.equal(W1[dk:2 * dk], keep[dk:2 * dk] / 2)
    with torch.no_grad():
        lay.Kx.bias.add_(1.0)
    assert not torch.equal(lay.wcat()[1], b0)
    # the amplitudes are not part of the operand
    W2 = lay.wcat()[0]
    with torch.no_grad():
        lay.output_var_x.mul_(3.0)
    assert lay.wcat()[0] is W2
    p0, p1 = lay._score_params()
    assert p1 == 1.0 and abs(p0 - 3.0 * m["output_var_x"] * m["output_var_p"]) <= 1e-6 * p0


@pytest.mark.parametrize("name", ["team_n0", "labels", "lane"])
def test_unfold_is_the_transpose_of_fold(name):
    d, m = load(name)
    att, C, F, P, H = m["attention_dim"], m["C"], m["F"], m["P"], m["heads"]
    gen = torch.Generator().manual_seed(5)
    ps = [torch.from_numpy(d[n]).double() for n in BO.PNAMES]
    lsx, lsp = torch.tensor([0.7], dtype=torch.float64), torch.tensor([1.9], dtype=torch.float64)
    W, b = fta.fold_beltrami(*ps, lsx, lsp, H, F, P, C)
    GW = torch.randn(W.shape, generator=gen, dtype=torch.float64)
    Gb = torch.randn(b.shape, generator=gen, dtype=torch.float64)
    back = fta.unfold_beltrami(GW, Gb, lsx, lsp, H, F, P, C)
    lhs = (W * GW).sum() + (b * Gb).sum()
    rhs = sum((p * g).sum() for p, g in zip(ps, back))
    assert abs(float(lhs - rhs)) <= 1e-12 * abs(float(lhs))
    assert [tuple(g.shape) for g in back] == [tuple(p.shape) for p in ps]
