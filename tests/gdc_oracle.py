"""float64 numpy oracle of the GDC rewiring (gnpde.graph_rewiring's contract) and the fixtures
its tests share: dense M, T = D^-1/2 M D^-1/2, S = alpha inv(I - (1 - alpha) T) (ppr) or
expm(-t (I - T)) (heat), top-k per column by the total order (value descending, row ascending),
threshold, column normalisation.

Acceptance (``check``) of a selection idx / val [N, k] (row j = column j of S):
  * values: |val - S[idx, j]| <= 1e-5 max_i S[i, j]: the project's 1e-5 parity bar at the
    column's scale (tau_j);
  * boundary rule, on EVERY column: each selected i has S[i, j] >= s_k - tau_j and each
    unselected i has S[i, j] <= s_k + tau_j, s_k the oracle's k-th value;
  * a column whose oracle gap s_k - s_{k+1} >= 2 tau_j is DECIDED: the rule forces the exact
    index set there, which is asserted explicitly.
"""
import collections

import numpy as np
import scipy.linalg

BAR = 1e-5

# name -> (N, deg, k); generator seed 3
SHAPES = {"small": (300, 6, 16), "wide": (777, 5, 64), "k128": (200, 8, 128)}
SEED = 3
ALPHAS = (0.05, 0.15)
HEAT_T = 3.0

Result = collections.namedtuple("Result", "S idx val wnorm tau decided")


def graph(N, deg, seed=SEED):
    """A connected undirected graph: a path along rng.permutation(N) plus N deg / 2 - (N - 1)
    random pairs (self pairs dropped), symmetrised, weights 1 -> (edge_index int64 [2, E], N).
    Duplicate pairs stay in the list (the contract sums them)."""
    rng = np.random.default_rng(seed)
    p = rng.permutation(N)
    extra = N * deg // 2 - (N - 1)
    a, b = rng.integers(0, N, extra), rng.integers(0, N, extra)
    keep = a != b
    src = np.concatenate([p[:-1], a[keep]])
    dst = np.concatenate([p[1:], b[keep]])
    ei = np.stack([np.concatenate([src, dst]), np.concatenate([dst, src])]).astype(np.int64)
    return ei, N


def dense_m(ei, w, N, w_self=1.0, remaining=False):
    """M = coalesce(A) + w_self I, or (remaining) A with the missing self loops filled."""
    w = np.ones(ei.shape[1]) if w is None else np.asarray(w, np.float64)
    M = np.zeros((N, N))
    if remaining:
        loop = ei[0] == ei[1]
        np.add.at(M, (ei[0][~loop], ei[1][~loop]), w[~loop])
        d = np.full(N, float(w_self))
        for e in np.flatnonzero(loop):  # the last existing loop keeps its weight
            d[ei[0][e]] = w[e]
        if w_self:
            M[np.arange(N), np.arange(N)] = d
        else:
            np.add.at(M, (ei[0][loop], ei[1][loop]), w[loop])
        return M
    np.add.at(M, (ei[0], ei[1]), w)
    return M + float(w_self) * np.eye(N)


def transition(M):
    deg = M.sum(0)
    with np.errstate(divide="ignore"):
        f = deg ** -0.5
    f[np.isinf(f)] = 0.0
    return f[:, None] * M * f[None, :]


def diffusion(T, method, alpha=None, t=None):
    n = T.shape[0]
    if method == "ppr":
        return alpha * np.linalg.inv(np.eye(n) - (1.0 - alpha) * T)
    return scipy.linalg.expm(-t * (np.eye(n) - T))


def topk(S, k):
    """Per column the k largest in (value descending, row ascending) -> idx [N, k] (row j =
    column j), val."""
    n = S.shape[0]
    idx = np.empty((S.shape[1], k), np.int64)
    for j in range(S.shape[1]):
        idx[j] = np.lexsort((np.arange(n), -S[:, j]))[:k]
    return idx, S[idx, np.arange(S.shape[1])[:, None]]


def col_normalise(val):
    s = val.sum(1, keepdims=True)
    return np.where(s == 0, 0.0, val / np.where(s == 0, 1.0, s))


def reference(ei, w, N, k, method, alpha=None, t=None, w_self=1.0):
    S = diffusion(transition(dense_m(ei, w, N, w_self)), method, alpha, t)
    idx, val = topk(S, k)
    tau = BAR * S.max(0)
    if k < N:
        srt = -np.sort(-S, axis=0)
        decided = srt[k - 1] - srt[k] >= 2 * tau
    else:
        decided = np.ones(S.shape[1], bool)
    return Result(S, idx, val, col_normalise(val), tau, decided)


_CACHE = {}


def fixture(name, method="ppr", alpha=0.05, t=HEAT_T):
    """(edge_index, N, k, Result) of a named fixture; computed once and shared (read-only)."""
    key = (name, method, alpha if method == "ppr" else t)
    if key not in _CACHE:
        N, deg, k = SHAPES[name]
        ei, _ = graph(N, deg)
        res = reference(ei, None, N, k, method, alpha, t)
        for a in res:
            a.setflags(write=False)
        _CACHE[key] = (ei, N, k, res)
    return _CACHE[key]


def decided_share(res):
    return float(res.decided.mean())


def check(res, idx, val):
    """The acceptance rule of the module docstring; idx / val [N, k], row j = column j."""
    S, tau = res.S, res.tau
    idx = np.asarray(idx, np.int64)
    val = np.asarray(val, np.float64)
    n, k = S.shape[0], res.idx.shape[1]
    assert idx.shape == (S.shape[1], k) and val.shape == idx.shape
    cols = np.arange(S.shape[1])[:, None]
    assert ((idx >= 0) & (idx < n)).all()
    assert (np.sort(idx, 1)[:, 1:] != np.sort(idx, 1)[:, :-1]).all(), "a row selected twice"
    got = S[idx, cols]
    err = np.abs(val - got) / tau[:, None]
    print("gdc check: max |val - S| / tau = %.3f, decided share %.3f" % (err.max(), decided_share(res)))
    assert (err <= 1.0).all()
    sk = res.val[:, -1]
    assert (got >= (sk - tau)[:, None]).all(), "a selected entry below s_k - tau"
    sel = np.zeros((S.shape[1], n), bool)
    sel[cols, idx] = True
    assert (np.where(sel, -np.inf, S.T) <= (sk + tau)[:, None]).all(), "an unselected entry above s_k + tau"
    d = res.decided
    assert np.array_equal(np.sort(idx[d], 1), np.sort(res.idx[d], 1))


def edges_to_columns(ei, w, N, k):
    """A (row, col)-sorted rewired edge list with E = N k -> (idx, wnorm) [N, k] per column,
    rows ascending inside a column."""
    ei, w = np.asarray(ei), np.asarray(w)
    assert ei.shape == (2, N * k) and w.shape == (N * k,)
    order = np.lexsort((ei[0], ei[1]))
    assert np.array_equal(ei[1][order], np.repeat(np.arange(N), k))
    return ei[0][order].reshape(N, k), w[order].reshape(N, k)


def check_edges(res, ei, w, N, k):
    """check() for a column-normalised rewired edge list: the values are compared after
    undoing the normalisation with the oracle's kept sum of the SAME index set."""
    idx, wn = edges_to_columns(ei, w, N, k)
    ksum = res.S[idx, np.arange(N)[:, None]].sum(1, keepdims=True)
    check(res, idx, wn.astype(np.float64) * ksum)
    assert np.abs(wn.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
