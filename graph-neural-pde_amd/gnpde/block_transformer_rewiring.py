"""Drop-in RewireAttODEblock (reference src/block_transformer_rewiring.py:8-261).

Eval (:218-223): the RHS integrates over the graph of reset_graph_data with the head mean
of the block-level attention as ``edge_weight`` and ``attention_weights``.

Training (:203-216), every step under no_grad as in the reference:
  1. densify (:152-160): 'k_hop_att' replaces the edge list by the structural positions of
     W·W (W the coalesced matrix of ``odefunc.edge_weight``; row = edge_index[0], column =
     edge_index[1]) in ascending (row, col) order with S = (0.5 W + 0.5 W·W) o (1 - I) on
     them — one sparse product on the device (ops.two_hop, csrc/two_hop.hip) where the
     reference densifies to [B, N, N] (:68-77); 'random' takes the union with
     int(N (1 / (1 - rw_addD) - 1)) drawn index pairs;
  2. threshold (:210-214): q = 1 / (pc_change - rw_addD), pc_change = post / pre - 1,
     threshold = quantile(w0, q) (ops.quantile) over the weights the graph had BEFORE
     densification — upstream GRAND's behaviour and the only reading that runs at every
     size (the fork's dense overwrite of edge_weight, :93, breaks torch.quantile above
     N = 4096 and yields 0 below);
  3. scores (:162-171): S with new_edges 'k_hop_att' and sparsify 'S_hat', else the head
     mean of the attention recomputed over the new edge list;
  4. keep score > threshold and renormalise per group of the kept list (:187-197): the kept
     list becomes edge_index / data_edge_index, the renormalised scores edge_weight and
     attention_weights.
The Laplacian RHS reads ``edge_weight`` under this block name, so autograd sees constant
weights and differentiates through x, alpha_train and beta_train, as in the hard-attention
block.

The fork's training branch cannot run as written (SURVEY.md §0.5 family): the (row, col)
columns are sorted independently (:60-61, :84-85), ``cat.shape(2)`` is called (:53),
``edge_index[norm_idx]`` is taken along the batch axis (:35).  This module builds the lines
as they are meant for B = 1 (the edge counts differ per graph); parity for that branch is
against the oracle (tests/rewire_oracle.py), the sound lines :68-77 against recorded
output.  'k_hop_lap' is ``pass`` in the reference (:157-158): pc_change = 0 and the quantile
raises; 'random_walk' calls a method that is commented out (:129, :156).  ``use_flux``
broadcasts [B,1,E] against [1,1,C] (:173-179) and is broken for E != C: it raises.
"""
import torch

from . import ops
from ._cache import _tensor_key
from .base_classes import ODEblock
from .function_transformer_attention import SpGraphTransAttentionLayer
from .integrator import odeint, odeint_adjoint


class RewireAttODEblock(ODEblock):
    def __init__(self, odefunc, regularization_fns, opt, device, t=torch.tensor([0, 1]), gamma=0.5):
        super(RewireAttODEblock, self).__init__(odefunc, regularization_fns, opt, device, t)
        assert opt['att_samp_pct'] > 0 and opt['att_samp_pct'] <= 1, "attention sampling threshold must be in (0,1]"
        self.device = device
        # the integrated copy (src/block_transformer_rewiring.py:13)
        self.odefunc = self._new_odefunc(odefunc, opt, device)
        self.train_integrator = odeint_adjoint if opt.get('adjoint', False) else odeint
        self.test_integrator = odeint
        self.set_tol()
        if opt['function'] not in {'GAT', 'transformer'}:
            self.multihead_att_layer = SpGraphTransAttentionLayer(opt['hidden_dim'], opt['hidden_dim'], opt, device,
                                                                  edge_weights=self.odefunc.edge_weight)
            if device is not None:
                self.multihead_att_layer = self.multihead_att_layer.to(device)
        self._base_graph = None
        # the 'random' draw (the reference uses np.random: no parity on the draw itself)
        self.generator = torch.Generator()
        self.generator.manual_seed(int(opt.get('seed', 0) or 0))

    def get_attention_weights(self, x):
        if self.opt['function'] not in {'GAT', 'transformer'}:
            attention, values = self.multihead_att_layer(x, self.data_edge_index)
        else:
            attention, values = self.odefunc.multihead_att_layer(x, self.data_edge_index)
        return attention

    def _install_graph(self, edge_index):
        """The device CSR of a rewired edge list as the integrated function's cached graph:
        the list's indices come from the graph's own, so the range check (a host read) is
        skipped."""
        f = self.odefunc
        n = int(self.num_nodes)
        chunk = self.opt.get('gnpde_chunk') if isinstance(self.opt, dict) else None
        f.edge_index = edge_index
        f._graph = ops.GraphCSR(edge_index, n, chunk=chunk, validate=False)
        f._graph_key = (_tensor_key(edge_index), n)
        f._w_cache = {}
        return f._graph

    def renormalise_attention(self, attention):
        """attention [B,E'] over odefunc.edge_index / (its group sum + 1e-16) (:34-37)."""
        if attention.numel() == 0:   # nothing kept: nothing to renormalise
            return attention
        g = self.odefunc.graph_for(int(self.num_nodes))
        grouped = g.csr if int(self.opt['attention_norm_idx']) == 0 else g.csc
        return ops.group_normalize(grouped, attention.reshape(-1)).reshape(attention.shape)

    def _single_graph(self):
        if self.data_edge_index.shape[0] != 1:
            raise NotImplementedError("gnpde: rewire_attention keeps a different edge count per graph; the "
                                      "reference's batched branch is broken (:35, :53, :60-61) and only B = 1 is "
                                      "supported")

    def add_random_edges(self, pairs=None):
        """:40-63: the union of the edge list with M = int(N (1 / (1 - rw_addD) - 1)) index
        pairs drawn with replacement from [0, N), in ascending (row, col) order, duplicates
        removed.  ``pairs`` [2, M] (or [1, 2, M]) int64 injects the draw."""
        self._single_graph()
        n = int(self.num_nodes)
        M = int(n * (1 / (1 - self.opt['rw_addD']) - 1))
        with torch.no_grad():
            ei = self.data_edge_index
            if pairs is None:
                pairs = torch.randint(0, n, (2, M), generator=self.generator, dtype=torch.int64)
            pairs = pairs.reshape(2, -1).to(device=ei.device, dtype=torch.int64)
            cat = torch.cat([ei[0], pairs], dim=1)
            key = torch.unique(cat[0] * n + cat[1])        # sorted: ascending (row, col)
            self.data_edge_index = torch.stack([key // n, key % n]).unsqueeze(0)
            self.odefunc.edge_index = self.data_edge_index

    def add_khop_edges(self, k=2, rm_self_loops=True):
        """:65-93 for k = 2: the positions of W·W and S on them (ops.two_hop); the positions
        become the edge list, S ``odefunc.attention_weights`` (``edge_weight`` keeps the
        graph's own weights: the threshold is their quantile)."""
        if k != 2:
            raise NotImplementedError("gnpde: add_khop_edges builds k = 2 (the reference's only call, :160)")
        self._single_graph()
        with torch.no_grad():
            f = self.odefunc
            # the prepared graph's CSR, kept across forwards (the integrated function's cached graph is
            # the rewired one after every training forward)
            key = (_tensor_key(f.edge_index), int(self.num_nodes))
            if self._base_graph is None or self._base_graph[0] != key:
                self._base_graph = (key, ops.GraphCSR(f.edge_index, int(self.num_nodes)))
            g = self._base_graph[1]
            ei, S, rowptr = ops.two_hop(g, f.edge_weight)
            self.data_edge_index = ei
            f.edge_index = ei
            f.attention_weights = S.reshape(1, -1)

    def densify_edges(self, pairs=None):
        new_edges = self.opt['new_edges']
        if new_edges == 'random':
            self.add_random_edges(pairs)
        elif new_edges == 'random_walk':
            raise NotImplementedError("gnpde: new_edges='random_walk' calls add_rw_edges, which the reference has "
                                      "commented out (block_transformer_rewiring.py:129, :156)")
        elif new_edges == 'k_hop_lap':
            pass
        elif new_edges == 'k_hop_att':
            self.add_khop_edges(k=2)

    def threshold_edges(self, x, threshold):
        """:162-197: the scores of the densified list against the threshold; the kept list and
        its renormalised weights go onto the integrated function."""
        if self.opt.get('use_flux', False):
            raise NotImplementedError("gnpde: use_flux is broken in the reference (broadcasts [B,1,E] against "
                                      "[1,1,C], block_transformer_rewiring.py:173-179)")
        self._single_graph()
        with torch.no_grad():
            if self.opt['new_edges'] == 'k_hop_att' and self.opt['sparsify'] == 'S_hat':
                mean_att = self.odefunc.attention_weights
            else:
                mean_att = ops.mix_weights(self.get_attention_weights(x))
            mean_att = mean_att.reshape(1, -1)
            mask = (mean_att > threshold).reshape(-1)
            kept = self.data_edge_index[:, :, mask].contiguous()   # sizes the kept list: the forward's host read
            self._install_graph(kept)
            weights = self.renormalise_attention(mean_att[:, mask].contiguous())
        self.retained = kept.shape[2]
        print('retaining {} of {} edges'.format(kept.shape[2], self.data_edge_index.shape[2]))
        self.data_edge_index = kept
        self.odefunc.edge_weight = weights  # rewiring the structure: the preprocessed weights are replaced
        self.odefunc.attention_weights = weights

    def rewire(self, x, pairs=None):
        """The training forward's graph surgery (:204-216)."""
        self._single_graph()
        with torch.no_grad():
            # (the attention of :206-207 is read by no branch once the scores are S or recomputed: skipped)
            w0 = self.odefunc.edge_weight
            pre_count = self.odefunc.edge_index.shape[2]
            self.densify_edges(pairs)
            post_count = self.odefunc.edge_index.shape[2]
            pc_change = post_count / pre_count - 1
            rw_addD = self.opt['rw_addD']
            d = pc_change - rw_addD
            q = 1 / d if d != 0 else float('inf')
            if not 0 <= q <= 1:
                raise ValueError("gnpde: rewire_attention: quantile q = 1 / (pc_change - rw_addD) = %r is outside "
                                 "[0, 1] (pc_change = %r, rw_addD = %r), as torch.quantile raises in the reference "
                                 "(block_transformer_rewiring.py:214)" % (q, pc_change, rw_addD))
            self.pc_change, self.q = pc_change, q
            self.threshold = ops.quantile(w0, q)
            self.threshold_edges(x, self.threshold)

    def forward(self, x, graph_data, y=None, pairs=None):
        self.reset_graph_data(graph_data, x.dtype, y)
        for f in (self.odefunc, self.reg_odefunc.odefunc):
            f.compact_sampled = False
        if self.training:
            self.rewire(x, pairs)
        else:
            self.odefunc.edge_index = self.data_edge_index
            att = self.get_attention_weights(x)
            # head mean (:221); with autograd recording the torch mean keeps the attention's graph
            mean_att = att.mean(dim=2) if att.requires_grad else ops.mix_weights(att)
            self.odefunc.edge_weight = mean_att
            self.odefunc.attention_weights = mean_att
        self.reg_odefunc.odefunc.edge_index = self.odefunc.edge_index
        self.reg_odefunc.odefunc.edge_weight = self.odefunc.edge_weight
        self.reg_odefunc.odefunc.attention_weights = self.odefunc.attention_weights
        return self._integrate(x, {'step_size': self.opt.get('step_size')})

    def __repr__(self):
        return self.__class__.__name__ + '( Time Interval ' + str(self.t[0].item()) + ' -> ' + \
            str(self.t[1].item()) + ")"
