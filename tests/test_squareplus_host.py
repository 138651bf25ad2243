"""Host side of the squareplus switch, on CPU: opt['square_plus'] is accepted together with
opt['gnpde_square_plus'] (ODEFuncTransformerAtt and the three attention blocks construct)
and refused without it; the GAT function keeps ignoring it; the sharded attention refuses it."""
import json
import os

import pytest
import torch

import gnpde
from conftest import GOLDEN

OPT = {'self_loop_weight': 1, 'leaky_relu_slope': 0.2, 'heads': 2, 'attention_norm_idx': 0, 'add_source': False,
       'hidden_dim': 6, 'block': 'constant', 'function': 'laplacian', 'augment': False, 'adjoint': False,
       'tol_scale': 1, 'time': 1, 'method': 'euler', 'no_alpha_sigmoid': False, 'reweight_attention': False,
       'step_size': 1, 'beltrami': False, 'attention_type': 'scaled_dot', 'square_plus': True, 'max_nfe': 1000,
       'data_norm': 'rw', 'max_iters': 1000, 'multi_modal': False, 'mix_features': False, 'attention_dim': 16}
BOTH = dict(OPT, gnpde_square_plus=True)
T01 = torch.tensor([0, 1])


def _blocks(opt):
    return [lambda: gnpde.AttODEblock(gnpde.LaplacianODEFunc, [], dict(opt, block='attention'), None, t=T01),
            lambda: gnpde.MixedODEblock(gnpde.LaplacianODEFunc, [], dict(opt, block='mixed'), None, t=T01),
            lambda: gnpde.HardAttODEblock(gnpde.LaplacianODEFunc, [], dict(opt, block='hard_attention',
                                                                             att_samp_pct=0.5), None, t=T01)]


def test_both_keys_construct():
    func = gnpde.ODEFuncTransformerAtt(6, 6, dict(BOTH, function='transformer'), None)
    lay = func.multihead_att_layer
    assert lay.square_plus and isinstance(lay, gnpde.SpGraphTransAttentionLayer)
    for make in _blocks(BOTH):
        blk = make()
        assert blk.multihead_att_layer.square_plus
    tr = gnpde.HardAttODEblock(gnpde.ODEFuncTransformerAtt, [], dict(BOTH, function='transformer',
                                                                      block='hard_attention', att_samp_pct=0.5), None,
                               t=T01)
    assert tr.odefunc.multihead_att_layer.square_plus
    # the state_dict is the softmax layer's: squareplus adds no parameter
    plain = gnpde.ODEFuncTransformerAtt(6, 6, dict(OPT, square_plus=False, function='transformer'), None)
    assert sorted(func.state_dict()) == sorted(plain.state_dict())
    assert not plain.multihead_att_layer.square_plus


def test_square_plus_alone_still_raises():
    for opt in (OPT, dict(OPT, gnpde_square_plus=False)):
        with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
            gnpde.ODEFuncTransformerAtt(6, 6, dict(opt, function='transformer'), None)
        with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
            gnpde.SpGraphTransAttentionLayer(6, 6, opt, None)
        for make in _blocks(opt):
            with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
                make()


def test_uniform_path_is_kept_under_squareplus():
    """Fork scaled_dot + source groups: the cached 1/outdeg weights, feature padding and the
    node layout stay as they are (att = p / (d p + 1e-16) is 1/outdeg to 1e-16 / (d p))."""
    func = gnpde.ODEFuncTransformerAtt(6, 6, dict(BOTH, function='transformer'), None)
    assert func.multihead_att_layer.is_uniform(0) and not func.multihead_att_layer.is_uniform(1)
    assert func.supports_feature_padding() and func.supports_node_layout()


def test_gat_function_ignores_square_plus():
    """The reference's GAT layer only ever calls softmax."""
    func = gnpde.ODEFuncAtt(6, 6, dict(OPT, function='GAT', gnpde_gat=True), None)
    assert isinstance(func.multihead_att_layer, gnpde.SpGraphAttentionLayer)


def test_sharded_attention_refuses_square_plus():
    from gnpde import dist
    z = torch.zeros(4, 6)
    for cls in (dist.RowShardedTransformer, dist.ColumnShardedTransformer):
        with pytest.raises(NotImplementedError, match="square_plus"):
            cls(torch.zeros(1, 2, 3, dtype=torch.int64), 3, 6, z, z[:, 0], z, z[:, 0], 2, 1, 0.5, square_plus=True)


def test_best_params_settings_construct():
    """The four best_params entries that set square_plus (settings recorded from
    src/best_params.py) construct their blocks once gnpde_square_plus is added."""
    with open(os.path.join(GOLDEN, "squareplus", "best_params_squareplus.json")) as fh:
        bp = json.load(fh)
    assert sorted(bp) == ["Citeseer", "CoauthorCS", "Cora", "Pubmed"]
    for name, p in bp.items():
        assert p["square_plus"] is True and p["block"] == "attention"
        opt = dict(OPT, **p)
        with pytest.raises(NotImplementedError, match="gnpde_square_plus"):
            gnpde.set_block(opt)(gnpde.set_function(opt), [], opt, None, t=T01)
        opt = dict(opt, gnpde_square_plus=True)
        blk = gnpde.set_block(opt)(gnpde.set_function(opt), [], opt, None, t=T01)
        assert isinstance(blk, gnpde.AttODEblock) and blk.multihead_att_layer.square_plus
        assert blk.multihead_att_layer.h == p["heads"]
