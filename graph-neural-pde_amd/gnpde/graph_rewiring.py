"""Graph rewiring: kNN, GDC and positional-encoding distances.

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

Positional-encoding distance rewiring (the reference's ``--rewiring pos_enc_knn``:
``apply_pos_dist_rewire`` src/graph_rewiring.py:318-375 with ``hyperbolic_distances.hyperbolize``
and ``distances_kNN``).  Those lines do not run with current numpy / scipy / sklearn; what is
built is what they intend, per graph, for encodings x [N, C]:

* d_ij = sum_c (x_ic - x_jc)^2 in fp32 (the difference form above); the rank value u_ij =
  d_ij r_i r_j with r_i = 1 / max(1 - |x_i|^2, 2^-52) for ``pos_enc_type`` HYP* (|x|^2, 1 - |x|^2
  and r in float64, r rounded to fp32 once), u_ij = d_ij for DW*.
* Distances.  HYP*: D = arccosh(1 + 2u), the Poincare ball; DW*: D = sqrt(u).  Both are monotone
  in u, so all ranking is done on u.
* 'topk': row i -> the ``gdc_k`` columns of smallest (u_ij, j), the self index included (D_ii = 0,
  sklearn's `precomputed` kNN); int64 [B, 2, N k], src = the row.  An all-zero row is the origin,
  a point like any other; only a row with a non-finite value is masked, and it raises.
* 'threshold': thr = numpy.quantile(D, quant) over all N^2 entries (linear interpolation, the
  diagonal included); the edges are numpy.where(D <= thr): i ascending, j ascending within i.
  With pos = quant (N^2 - 1) and lo = floor(pos), {D <= thr} = {u <= u_(lo)}: one order statistic,
  found by a radix select over the matrix's tiles, which are recomputed by every pass and never
  stored (csrc/posdist.hip).
* DEPARTURES: the encodings are passed in (no pickle cache on disk), and the helpers
  ``apply_dist_KNN`` / ``apply_dist_threshold`` take encodings, not a dense distance matrix.
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


# --------------------------------------------------------------------------- positional-encoding distances
def _metric_of(pos_enc_type):
    t = str(pos_enc_type)
    if t.startswith("HYP"):
        return 'poincare'
    if t.startswith("DW"):
        return 'euclid'
    raise ValueError("apply_pos_dist_rewire: pos_enc_type %r (HYP* | DW*)" % (pos_enc_type,))


def hyperbolize(x, max_bytes=ops.POSDIST_MAX_BYTES):
    """The dense Poincare distances of the encodings x [B, N, C] (or [N, C]): fp32 [B, N, N]
    (the reference's hyperbolic_distances.hyperbolize, for small N: 4 B N^2 bytes above
    max_bytes, 8 GiB, raises ValueError).  Plain torch on x's device; the rewiring itself never
    forms this matrix."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    B, N, _C = x.shape
    if 4 * B * N * N > int(max_bytes):
        raise ValueError("hyperbolize: the dense [%d, %d, %d] distances take %d bytes, above max_bytes=%d"
                         % (B, N, N, 4 * B * N * N, int(max_bytes)))
    x = x.float()
    out = torch.empty(B, N, N, dtype=torch.float32, device=x.device)
    for b in range(B):
        u = ops._pair_dense_u(x[b], ops._lib.METRIC_POINCARE, max_bytes, "hyperbolize")
        out[b] = ops.pair_dist_from_u(u, 'poincare').float()
    return out


def apply_dist_KNN(x, k, metric='poincare', backend=None):
    """The k nearest neighbours of every row of the encodings x [B, N, C] (or [N, C]) under
    ``metric`` as an edge list: int64 [B, 2, N k], src = the row (position i k + m -> i), dst its
    neighbours in ascending (distance, index), the self index included (sklearn's `precomputed`
    kNN of the reference's apply_dist_KNN).  DEPARTURE: takes the encodings, not a dense
    distance matrix.  A row with a non-finite value, or k above N, raises ValueError (the one
    host read: the pre-pass's counts)."""
    be = ops.POSDIST_HIP if backend is None else backend
    k = int(k)
    if x.dim() == 2:
        x = x.unsqueeze(0)
    with torch.no_grad():
        idx, n_valid = be.pos_knn(x, k, metric)
        B, N = idx.shape[0], idx.shape[1]
        short = int(n_valid.min())  # the host read
        if short < N:
            raise ValueError("apply_dist_KNN: %d rows of a graph hold a non-finite value" % (N - short))
        first = torch.arange(N, device=idx.device, dtype=torch.int64).repeat_interleave(k).expand(B, N * k)
        return torch.stack([first, idx.reshape(B, N * k).to(torch.int64)], dim=1)


def apply_feat_KNN(x, k, backend=None):
    """The reference's apply_feat_KNN: apply_dist_KNN under the Euclidean metric."""
    return apply_dist_KNN(x, k, metric='euclid', backend=backend)


def apply_dist_threshold(x, quant=1 / 1000, metric='poincare', backend=None):
    """Every pair of rows of the encodings x [N, C] (or [1, N, C]) whose distance is at most
    numpy.quantile(D, quant) of all N^2 distances (linear interpolation, the diagonal included):
    int64 [1, 2, E] in numpy.where order, src = the row.  DEPARTURE: takes the encodings, not a
    dense distance matrix.  B > 1 raises NotImplementedError (the edge counts differ per graph);
    quant outside [0, 1], a non-finite value or E >= 2^35 raises ValueError."""
    be = ops.POSDIST_HIP if backend is None else backend
    quant = float(quant)
    if not 0.0 <= quant <= 1.0:
        raise ValueError("apply_dist_threshold: quantile %r outside [0, 1]" % (quant,))
    if x.dim() == 3 and x.shape[0] != 1:
        raise NotImplementedError("apply_dist_threshold with B > 1: the edge counts differ per graph")
    with torch.no_grad():
        return be.threshold_edges(x, quant, metric).unsqueeze(0)


def apply_pos_dist_rewire(data, opt, pos_encoding, backend=None):
    """The reference's apply_pos_dist_rewire (src/graph_rewiring.py:318-375; ``--rewiring
    pos_enc_knn``): the graph becomes the gdc_k nearest neighbours of every node's positional
    encoding, or every pair within the pos_dist_quantile quantile of all N^2 distances.

    pos_encoding: [N, C] or [1, N, C] fp32 on the device, required.  DEPARTURE: the encodings
    are passed in; the reference's pickle cache of encodings and distances on disk is out of
    scope, like every loader.  The dense distance matrix is never formed.
    Options read: pos_enc_type (HYP*: Poincare distances; DW*: Euclidean; anything else raises
    ValueError), gdc_sparsification ('topk' with gdc_k <= 64 | 'threshold'), pos_dist_quantile
    (HYP* only: for DW* the reference passes no quantile to apply_dist_threshold, which then
    takes its default of 1/1000 — kept).
    Writes data.edge_index at the rank it came in ([2, E], or [1, 2, E]) and returns data;
    data.edge_attr, the weights of edges that no longer exist, becomes None.
    Raises: NotImplementedError for B > 1 under 'threshold'; ValueError for a row with a
    non-finite value, a quantile outside [0, 1], gdc_k outside [1, min(64, N)], or E >= 2^35
    (before the edge list is allocated).  backend: ops.POSDIST_HIP by default; ops.POSDIST_TORCH
    is the same contract in torch ops on any device."""
    metric = _metric_of(opt['pos_enc_type'])
    x = pos_encoding
    sp = opt['gdc_sparsification']
    if sp == 'topk':
        k = int(opt['gdc_k'])
        if not 1 <= k <= ops.KNN_MAX_K:
            raise ValueError("apply_pos_dist_rewire: gdc_k=%d outside [1, %d]" % (k, ops.KNN_MAX_K))
        ei = apply_dist_KNN(x, k, metric, backend)
    elif sp == 'threshold':
        quant = opt['pos_dist_quantile'] if metric == 'poincare' else 1 / 1000
        ei = apply_dist_threshold(x, quant, metric, backend)
    else:
        raise ValueError("apply_pos_dist_rewire: gdc_sparsification %r (topk | threshold)" % (sp,))
    old = data.edge_index
    batched = old is not None and old.dim() == 3
    if not batched:
        if ei.shape[0] != 1:
            raise ValueError("apply_pos_dist_rewire: B = %d encodings for an unbatched edge_index" % ei.shape[0])
        ei = ei[0]
    data.edge_index = ei
    data.edge_attr = None
    return data
