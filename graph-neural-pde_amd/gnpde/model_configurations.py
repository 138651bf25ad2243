"""Drop-in registry (reference src/model_configurations.py:17-44): the plugin
point ``GNN.__init__`` uses (src/GNN.py:12-15).

Built here: block 'constant', 'attention', 'mixed',
'hard_attention'; function 'laplacian', 'transformer' and 'GAT'.  'GAT'
(function_GAT_attention.ODEFuncAtt) is returned when the option dict sets
``gnpde_gat`` to a true value; without the key it raises NotImplementedError
naming the key (the plain dict's behaviour is pinned by the host tests until the
switch becomes the default).  'laplacian' with ``multi_modal`` and
``gnpde_multi_modal`` both set is function_laplacian_multimodal.MultiModalLaplacianODEFunc
(the second modality's cross-attention; block 'constant' only).  Block 'rewire_attention'
(block_transformer_rewiring.RewireAttODEblock) is returned when the option dict sets
``gnpde_rewire_attention`` to a true value; without the key it raises NotImplementedError
naming the key, rather than silently falling back to a different model.
"""
from .block_constant import ConstantODEblock
from .block_mixed import MixedODEblock
from .block_transformer_hard_attention import HardAttODEblock
from .block_transformer_rewiring import RewireAttODEblock
from .block_transformer_attention import AttODEblock
from .function_laplacian_diffusion import LaplacianODEFunc
from .function_laplacian_multimodal import MultiModalLaplacianODEFunc
from .function_GAT_attention import ODEFuncAtt
from .function_transformer_attention import ODEFuncTransformerAtt


class BlockNotDefined(Exception):
    pass


class FunctionNotDefined(Exception):
    pass


def set_block(opt):
    ode_str = opt['block']
    if ode_str == 'mixed':
        return MixedODEblock
    if ode_str == 'attention':
        return AttODEblock
    if ode_str == 'hard_attention':
        return HardAttODEblock
    if ode_str == 'constant':
        return ConstantODEblock
    if ode_str == 'rewire_attention':
        if opt.get('gnpde_rewire_attention'):
            return RewireAttODEblock
        raise NotImplementedError("gnpde: block 'rewire_attention' (block_transformer_rewiring.RewireAttODEblock) is "
                                  "opt-in: set opt['gnpde_rewire_attention'] = True to select it")
    raise BlockNotDefined


def set_function(opt):
    ode_str = opt['function']
    if ode_str == 'laplacian':
        if opt.get('multi_modal', False) and opt.get('gnpde_multi_modal', False):
            return MultiModalLaplacianODEFunc
        return LaplacianODEFunc
    if ode_str == 'transformer':
        return ODEFuncTransformerAtt
    if ode_str == 'GAT':
        if opt.get('gnpde_gat'):
            return ODEFuncAtt
        raise NotImplementedError("gnpde: function 'GAT' (function_GAT_attention.ODEFuncAtt) is opt-in: set "
                                  "opt['gnpde_gat'] = True to select it")
    raise FunctionNotDefined
