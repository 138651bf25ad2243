"""Graph rewiring: kNN and GDC.

kNN graph rewiring (the reference's ``rewire_KNN``; src/graph_rewiring.py:122-161, called
from the training loop at src/graph_datasets/run_GNN.py:252-254): every
``rewire_KNN_epoch`` epochs the graph becomes the k nearest neighbours of the current node
embeddings.  The reference delegates the search to ``pykeops.LazyTensor.argKmin``; here it
is the exact top-k kernel of csrc/knn.hip (``ops.knn``).

The reference's lines read as they are meant:

* Input.  ``x`` [B, N, C] fp32 (or [N, C], treated as B = 1); k = ``opt['rewire_KNN_k']``.
* Masked rows.  The reference maps all-zero rows (the fork's batch padding) to NaN and
  then to inf (:128-130).  Here a row is masked when it is all zero or holds any
  non-finite value.  A masked row is never a candidate; a masked query row outputs its
  own index k times (parallel self loops, inert on a zero row: the COO convention here
  keeps duplicates and sums them).
* Distance.  d_ij = sum_c (x_ic - x_jc)^2 in fp32, the reference's difference form (:136),
  not the Gram form |xi|^2 + |xj|^2 - 2 xi.xj, whose cancellation error scales with |x|^2
  and reorders near neighbours.  All terms are non-negative, so any summation order is
  within (C + 3) 2^-24 relative of the exact value.  The self index is not excluded
  (d_ii = 0), as in the reference.
* Order.  Each query's k neighbours come in ascending (d_ij, j): distance first, the lower
  index on a tie.  The order is total, so the result is deterministic and independent of
  the kernel's tiling.  KeOps' tie behaviour is unspecified (and the library is not a
  dependency here): this is a definition, not a parity claim.
* Output.  int64 [B, 2, N k] (:139-143): row 0 the query index i repeated k times
  (position i k + m -> i), row 1 the neighbours.
* ``rewire_KNN_sym``.  ``to_undirected`` per graph: both directions, sorted by (row, col),
  duplicates removed, in torch ops on the device.  B = 1 only; B > 1 raises
  NotImplementedError (the edge counts differ per graph; HardAttODEblock treats the same
  case the same way).
* Errors.  k above the number of unmasked rows of any batch element raises ValueError;
  this is the one host read per rewire (the per-graph counts of the mask pre-pass).  A
  bf16 or CPU ``x`` raises, as elsewhere on the product path.

GDC graph diffusion rewiring (the reference's ``--rewiring gdc`` and BLEND's
``pos_enc_type='GDC'``: ``apply_gdc`` src/graph_rewiring.py:42-81, ``GDCWrapper`` :378-434,
which subclass PyG's ``GDC``).  PyG is not a dependency: what follows is a definition, not a
parity claim against PyG's tie behaviour or its push approximation.  One graph (B = 1; B > 1
raises NotImplementedError): ``edge_index`` [2, E] or [1, 2, E] int64, optional weights
``edge_attr`` (ones otherwise), N = ``num_nodes``.

1. Self loops.  ``__call__``: M = coalesce(A) + w_self I, duplicates summed, w_self =
   ``self_loop_weight`` (0 / None: none) — PyG's add_self_loops then coalesce.
   ``position_encoding``: add_remaining_self_loops (:407-410) — an existing loop keeps its
   weight, a missing one gets w_self (``ops.add_self_loops``).
2. ``normalization_in='sym'``: T = D^-1/2 M D^-1/2, deg the column sums, inf -> 0
   (``ops.norm_weights``, GCN).  DEPARTURE: M must be symmetric; it is checked once on the
   device and a non-symmetric input raises ValueError (symmetrise with ``to_undirected``).
   The reference's datasets are undirected, and the iteration bounds rest on T's spectrum
   lying in [-1, 1].
3. Diffusion.  'ppr': S = alpha (I - (1 - alpha) T)^-1; any other ``gdc_method``: heat,
   S = exp(-t (I - T)).  Column blocks of up to 128 seeds, each a short polynomial
   recurrence in T on the SpMM kernel (``ops.diffusion_schedule`` / ``ops.diffusion_block``:
   Chebyshev iteration for ppr, Horner on the Taylor series for heat), truncated at
   tol = 1e-6 of the column's scale.
4. Sparsification.  'topk' (dim = 0): per column j the k entries S[i, j] largest in the total
   order (value descending, i ascending) as edges (i, j); zeros are candidates like any
   value, so a component smaller than k pads with zero-weight edges to the lowest indices
   and E = N k always; k > N raises ValueError.  'threshold': the entries with
   S[i, j] >= ``gdc_threshold``.
5. ``normalization_out='col'``: every kept weight divided by its column's kept sum (topk:
   the sum in rank order, sequentially in fp32: the bits do not depend on the tiling).
6. ``type='combined'``: the edges sorted by (row, col) with their weights, written into
   ``data.edge_index`` / ``data.edge_attr`` at the rank they came in.
7. ``type='pos_encoding'``: the dense [N, N] column-normalised S without sparsification
   (:419-434), transposed for ``pos_enc_orientation='col'``; N N 4 bytes above ``max_bytes``
   (8 GiB) raises ValueError.
8. ``exact``.  DEPARTURE: both settings return the exact matrix to the tolerance above (the
   push approximation's own error is not reproduced).  ``exact=False`` with a self-loop
   weight other than 1 raises ValueError (the wrapper's assert).
"""
import torch

from . import ops


def to_undirected(ei, num_nodes):
    """[2, E] -> both directions, sorted by (row, col), duplicates removed."""
    row = torch.cat([ei[0], ei[1]])
    col = torch.cat([ei[1], ei[0]])
    key = torch.unique(row * num_nodes + col)  # sorted
    return torch.stack([torch.div(key, num_nodes, rounding_mode='floor'), key % num_nodes])


def KNN(x, opt, knn=None):
    """The kNN edge_index of x (module docstring).  knn: the search, ``ops.knn`` by default;
    ``ops.knn_torch`` is the same contract in torch ops on any device."""
    k = int(opt['rewire_KNN_k'])
    if x.dim() == 2:
        x = x.unsqueeze(0)
    with torch.no_grad():
        idx, n_valid = (ops.knn if knn is None else knn)(x, k)
        short = int(n_valid.min())  # the host read of a rewire
        if short < k:
            raise ValueError("KNN: rewire_KNN_k=%d exceeds the %d unmasked rows of a graph" % (k, short))
        B, N = idx.shape[0], idx.shape[1]
        first = torch.arange(N, device=idx.device, dtype=torch.int64).repeat_interleave(k).expand(B, N * k)
        ei = torch.stack([first, idx.reshape(B, N * k).to(torch.int64)], dim=1)
        if opt.get('rewire_KNN_sym', False):
            if B > 1:
                raise NotImplementedError("rewire_KNN_sym with B > 1: the edge counts differ per graph")
            ei = to_undirected(ei[0], N).unsqueeze(0)
    return ei


@torch.no_grad()
def apply_KNN(x, graph_data, x2, pos_encoding, model, opt):
    """The reference's dispatch on ``rewire_KNN_T``: the raw features, the encoder's output
    (T0) or the ODE's final state (TN).  model: anything with ``forward_encoder(x,
    pos_encoding)`` and ``forward_ODE(x, graph_data, pos_encoding, x2)``."""
    if opt['rewire_KNN_T'] == "raw":
        ei = KNN(x, opt)
    elif opt['rewire_KNN_T'] == "T0":
        ei = KNN(model.forward_encoder(x, pos_encoding), opt)
    elif opt['rewire_KNN_T'] == 'TN':
        ei = KNN(model.forward_ODE(x, graph_data, pos_encoding, x2), opt)
    else:
        raise Exception("Need to set rewire_KNN_T")
    return ei


class GDCWrapper(object):
    """The reference's GDCWrapper (src/graph_rewiring.py:378-434) without a PyG base class:
    ``__call__(data)`` rewires ``data`` (any object with edge_index, edge_attr, num_nodes),
    ``position_encoding(data)`` returns the dense column-normalised diffusion matrix.
    gdc: the driver, ``ops.gdc`` by default; ``ops.gdc_torch`` is the same contract in torch
    ops on any device.
    The constructor's defaults are the reference's, and its default ``sparsification_kwargs``
    (threshold by ``avg_degree``) is NOT served: ``__call__`` takes ``method='topk'`` with ``k``
    (``dim`` 0) or ``method='threshold'`` with ``eps`` and raises NotImplementedError for
    anything else, so a default-constructed wrapper serves ``position_encoding`` only (which
    does not sparsify).  ``apply_gdc`` always passes one of the two served forms."""

    def __init__(self, self_loop_weight=1, normalization_in='sym', normalization_out='col',
                 diffusion_kwargs=dict(method='ppr', alpha=0.15),
                 sparsification_kwargs=dict(method='threshold', avg_degree=64), exact=True, gdc=None,
                 max_bytes=ops.GDC_MAX_BYTES):
        if normalization_in != 'sym' or normalization_out != 'col':
            raise NotImplementedError("GDCWrapper: normalization_in='sym' and normalization_out='col' (the "
                                      "reference's apply_gdc) are the supported normalisations")
        self.self_loop_weight = self_loop_weight
        self.normalization_in = normalization_in
        self.normalization_out = normalization_out
        self.diffusion_kwargs = dict(diffusion_kwargs)
        self.sparsification_kwargs = dict(sparsification_kwargs)
        self.exact = exact
        self.gdc = gdc
        self.max_bytes = max_bytes
        if self_loop_weight and not (exact or self_loop_weight == 1):
            raise ValueError("GDCWrapper: exact=False needs self_loop_weight == 1, got %r" % (self_loop_weight,))

    def _args(self, dense):
        d, s = self.diffusion_kwargs, self.sparsification_kwargs
        kw = dict(method='ppr' if d.get('method') == 'ppr' else 'heat', self_loop_weight=self.self_loop_weight or 0.0,
                  dense=dense, max_bytes=self.max_bytes)
        if kw['method'] == 'ppr':
            kw['alpha'] = d['alpha']
        else:
            kw['t'] = d['t']
        if not dense:
            if s.get('method') == 'topk':
                if s.get('dim', 0) != 0:
                    raise NotImplementedError("GDCWrapper: topk with dim=0 (per column) only")
                kw.update(sparsification='topk', k=int(s['k']))
            elif s.get('method') == 'threshold' and 'eps' in s:
                kw.update(sparsification='threshold', threshold=float(s['eps']))
            else:
                raise NotImplementedError("GDCWrapper: sparsification %r (topk with k | threshold with eps)" % (s,))
        return kw

    def _run(self, data, dense):
        ei = data.edge_index
        batched = ei.dim() == 3
        if batched and ei.shape[0] != 1:
            raise NotImplementedError("gnpde: GDC with B > 1: the rewired edge count differs per graph")
        w = data.edge_attr
        if w is not None:
            w = w.reshape(-1)
        N = data.num_nodes[0] if isinstance(data.num_nodes, list) else data.num_nodes
        with torch.no_grad():
            out = (ops.gdc if self.gdc is None else self.gdc)(ei, w, int(N), **self._args(dense))
        return out, batched

    def __call__(self, data):
        (ei, w), batched = self._run(data, False)
        data.edge_index = ei.unsqueeze(0) if batched else ei
        data.edge_attr = w.unsqueeze(0) if batched else w
        return data

    def position_encoding(self, data):
        return self._run(data, True)[0]


def apply_gdc(data, opt, type="combined", gdc=None):
    """The reference's apply_gdc (src/graph_rewiring.py:42-81) with its option mapping:
    gdc_method ('ppr', anything else: heat), ppr_alpha / heat_time, gdc_sparsification ('topk':
    gdc_k per column; otherwise the threshold gdc_threshold), self_loop_weight (0: no self
    loops), exact; type 'combined' rewires ``data``, 'pos_encoding' returns the dense encoding
    (pos_enc_orientation 'row', or 'col': its transpose)."""
    if opt['gdc_method'] == 'ppr':
        diff_args = dict(method='ppr', alpha=opt['ppr_alpha'])
    else:
        diff_args = dict(method='heat', t=opt['heat_time'])
    if opt['gdc_sparsification'] == 'topk':
        sparse_args = dict(method='topk', k=opt['gdc_k'], dim=0)
    else:
        sparse_args = dict(method='threshold', eps=opt['gdc_threshold'])
    diff_args['eps'] = opt['gdc_threshold']
    slw = float(opt['self_loop_weight']) if opt['self_loop_weight'] != 0 else None
    wrapper = GDCWrapper(slw, normalization_in='sym', normalization_out='col', diffusion_kwargs=diff_args,
                         sparsification_kwargs=sparse_args, exact=opt['exact'], gdc=gdc)
    if isinstance(data.num_nodes, list):
        data.num_nodes = data.num_nodes[0]
    if type == 'combined':
        return wrapper(data)
    if type == 'pos_encoding':
        if opt['pos_enc_orientation'] == "row":
            return wrapper.position_encoding(data)
        if opt['pos_enc_orientation'] == "col":
            return wrapper.position_encoding(data).T
        raise ValueError("apply_gdc: pos_enc_orientation %r (row | col)" % (opt['pos_enc_orientation'],))
    return data
