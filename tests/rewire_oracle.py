"""float64 numpy restatement of the rewire_attention block's graph surgery
(gnpde.block_transformer_rewiring; reference src/block_transformer_rewiring.py, the lines
as they are meant, B = 1) and the seeded fixtures of its tests.

W[i, j] = sum of w0 over the edges (i, j) (row = edge_index[0], column = edge_index[1]);
S = (0.5 W + 0.5 W·W) o (1 - I) on the structural non-zeros of W·W in ascending
(row, col) order (:65-93); q = 1 / (pc_change - rw_addD), threshold = quantile(w0, q)
(linear) over the weights the graph had before densification (:210-214); keep
score > threshold, renormalise per group of the kept list (:187-197)."""
import functools

import numpy as np

import gnpde_oracle as O

TAU = 2.0 ** -20


def dense_w(ei, w, N):
    W = np.zeros((N, N))
    np.add.at(W, (np.asarray(ei)[0, 0], np.asarray(ei)[0, 1]), np.asarray(w, np.float64).reshape(-1))
    return W


def two_hop(ei, w, N):
    """dict: W, S (dense), edge_index [1,2,nnz], values, rowptr, n (products per position:
    pairs of stored edges (i, m), (m, j), duplicates counted as the edges they are)."""
    ei = np.asarray(ei)
    W = dense_w(ei, w, N)
    A = np.zeros((N, N))
    np.add.at(A, (ei[0, 0], ei[0, 1]), 1.0)
    n = A @ A
    S = (0.5 * W + 0.5 * (W @ W)) * (1.0 - np.eye(N))
    pos = np.argwhere(n > 0)                      # row-major: ascending (row, col)
    r, c = pos[:, 0], pos[:, 1]
    rowptr = np.zeros(N + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(r, minlength=N))
    return dict(W=W, S=S, edge_index=np.stack([r, c])[None], values=S[r, c], rowptr=rowptr, n=n[r, c])


def union_random(ei, pairs, N):
    """'random' (:40-63): the union of the edge list with the drawn pairs [2, M], ascending
    (row, col), duplicates removed."""
    cat = np.concatenate([np.asarray(ei)[0], np.asarray(pairs).reshape(2, -1)], axis=1)
    key = np.unique(cat[0] * N + cat[1])
    return np.stack([key // N, key % N])[None]


def n_random(N, rw_addD):
    return int(N * (1 / (1 - rw_addD) - 1))


def threshold(w0, pre_count, post_count, rw_addD):
    """(pc_change, q, threshold): quantile(w0, q) with linear interpolation (:210-214)."""
    pc_change = post_count / pre_count - 1
    d = pc_change - rw_addD
    q = 1 / d if d != 0 else float('inf')
    if not 0 <= q <= 1:
        raise ValueError("pc_change=%r rw_addD=%r q=%r" % (pc_change, rw_addD, q))
    return pc_change, q, float(np.quantile(np.asarray(w0, np.float64).reshape(-1), q))


def keep(ei_new, scores, thr, norm_idx, N):
    """(mask, kept edge_index [1,2,K], renormalised weights [K]) (:187-197)."""
    scores = np.asarray(scores, np.float64).reshape(-1)
    mask = scores > thr
    kept = np.asarray(ei_new)[:, :, mask]
    return mask, kept, O.group_normalize(scores[mask], kept[0, norm_idx], N)


def undecided(scores, thr, tau=TAU):
    return np.abs(np.asarray(scores, np.float64).reshape(-1) - thr) <= tau * abs(thr)


def rewire_khop(ei, w0, N, rw_addD, norm_idx):
    """The whole k_hop_att / S_hat training surgery on the prepared graph (ei, w0)."""
    th = two_hop(ei, w0, N)
    pc, q, thr = threshold(w0, np.asarray(ei).shape[2], th['edge_index'].shape[2], rw_addD)
    mask, kept, w = keep(th['edge_index'], th['values'], thr, norm_idx, N)
    return dict(two_hop=th, pc_change=pc, q=q, threshold=thr, mask=mask, edge_index=kept, weights=w,
                undecided=undecided(th['values'], thr))


# --------------------------------------------------------------------------- fixtures
def _undirected(rng, N, n_pairs):
    a = rng.integers(0, N, size=n_pairs)
    b = rng.integers(0, N, size=n_pairs)
    ok = a != b
    key = np.unique(np.minimum(a, b)[ok] * N + np.maximum(a, b)[ok])
    a, b = key // N, key % N
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def _directed(rng, lo, hi, n):
    N = hi - lo
    key = np.unique(rng.integers(0, N, size=n) * N + rng.integers(0, N, size=n))
    e = np.stack([key // N, key % N]) + lo
    return e[:, rng.permutation(e.shape[1])]


NAMES = ('toy', 'n1', 'short', 'directed', 'dups', 'empty', 'hub', 'wide')
SEEDS = dict(toy=0, n1=0, short=0, directed=0, dups=0, empty=0, hub=0, wide=0)


@functools.lru_cache(maxsize=None)
def raw(name, seed=None):
    """(edge_index [1,2,E] int64, edge_attr [1,E] fp32 in [0.2, 1), N, self_loop_weight)."""
    rng = np.random.default_rng(1000 * NAMES.index(name) + (SEEDS[name] if seed is None else seed))
    fill = 1.0
    if name == 'toy':                    # the reference's toy edge list (test/test_*: 3 nodes)
        N, e = 3, np.array([[0, 2, 2, 1], [1, 0, 1, 2]])
    elif name == 'n1':
        N, e = 1, np.zeros((2, 0), np.int64)
    elif name == 'short':                # about 2 neighbours per node: rows shorter than a wavefront
        N = 64
        e = _undirected(rng, N, 64)
    elif name == 'directed':             # asymmetric: W·W against W^T·W, row / column swaps
        N = 97
        e = _directed(rng, 0, N, 400)
    elif name == 'dups':                 # duplicate edges in the input
        N = 50
        e = _directed(rng, 0, N, 150)
        e = np.concatenate([e, e[:, rng.integers(0, e.shape[1], size=60)]], axis=1)
        e = e[:, rng.permutation(e.shape[1])]
    elif name == 'empty':                # no self loops, isolated nodes: empty input and output rows
        N, fill = 80, 0.0
        e = _directed(rng, 0, 50, 150)
        sink = np.stack([np.arange(50, 56), np.arange(60, 66)])   # stored rows whose neighbour rows are empty
        e = np.concatenate([e, sink], axis=1)[:, rng.permutation(e.shape[1] + 6)]
    elif name == 'hub':                  # node 0 adjacent to half the graph
        N = 300
        nb = np.arange(1, 151)
        e = np.concatenate([_undirected(rng, N, 300), np.stack([np.zeros_like(nb), nb]),
                            np.stack([nb, np.zeros_like(nb)])], axis=1)
        e = np.unique(e[0] * N + e[1])
        e = np.stack([e // N, e % N])
    elif name == 'wide':                 # rows beyond any LDS table at the default boundary
        N = 3000
        nb = rng.permutation(np.arange(1, N))[:1500]
        e = np.concatenate([_undirected(rng, N, 4000), np.stack([np.zeros_like(nb), nb]),
                            np.stack([nb, np.zeros_like(nb)])], axis=1)
        e = np.unique(e[0] * N + e[1])
        e = np.stack([e // N, e % N])
    else:
        raise KeyError(name)
    e = e.astype(np.int64)[None]
    attr = rng.uniform(0.2, 1.0, size=(1, e.shape[2])).astype(np.float32)
    return e, attr, N, fill


@functools.lru_cache(maxsize=None)
def prepared(name, seed=None):
    """The graph as reset_graph_data prepares it: self loops (weight self_loop_weight, none at
    0) and the rw normalisation (norm_dim = 1) of the random positive edge attributes, the
    weights rounded to fp32 (what the device holds).  (edge_index [1,2,E], w0 fp32 [1,E], N)."""
    e, attr, N, fill = raw(name, seed)
    eis, ws = O.get_rw_adj(e, edge_weight=attr, norm_dim=1, fill_value=fill, num_nodes=N)
    return np.stack(eis, 0), np.stack(ws, 0).astype(np.float32), N


@functools.lru_cache(maxsize=None)
def product(name, seed=None):
    ei, w0, N = prepared(name, seed)
    return two_hop(ei, w0, N)
