"""kNN graph rewiring (the reference's ``rewire_KNN``; src/graph_rewiring.py:122-161, called
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
