"""float64 oracle of the kNN rewiring (gnpde.graph_rewiring) and the acceptance checks the
host and the GPU tests share.

Contract (gnpde/graph_rewiring.py): d_ij = sum_c (x_ic - x_jc)^2, a row is masked when it
is all zero or holds a non-finite value (never a candidate; as a query it returns itself k
times), neighbours in ascending (d_ij, j).

Tolerance, derived: a fp32 difference-form distance is within (C + 3) 2^-24 relative of the
exact value for any summation order (all terms are non-negative), so two of them compare
within tau = 2 (C + 3) 2^-24.
"""
import functools

import numpy as np

CHUNK_BYTES = 1 << 26


def tau(C):
    return 2.0 * (C + 3) * 2.0 ** -24


def masked_rows(x):
    return np.all(x == 0, axis=-1) | ~np.all(np.isfinite(x), axis=-1)


def distance_rows(x):
    """[N, C] -> the full [N, N] float64 difference-form distances (masked rows as zeros),
    chunked over query rows: no [N, N, C] array."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    D = np.empty((N, N), np.float64)
    rows = max(1, CHUNK_BYTES // max(1, 8 * N * C))
    for r0 in range(0, N, rows):
        diff = x[r0:r0 + rows, None, :] - x[None, :, :]
        D[r0:r0 + rows] = np.einsum('rnc,rnc->rn', diff, diff)
    return D


class Result(object):
    """idx [B, N, k] int64, dist [B, N, k] float64 (sorted), D [B, N, N] (the full rows; inf
    at masked candidates), masked [B, N], n_valid [B], strict [B, N] (every gap among the
    first k + 1 sorted distances exceeds tau relative; False for masked queries)."""


def knn(x, k):
    x = np.asarray(x)
    if x.ndim == 2:
        x = x[None]
    B, N, C = x.shape
    t = tau(C)
    res = Result()
    res.k, res.C = k, C
    res.masked = masked_rows(x)
    res.n_valid = (~res.masked).sum(1)
    res.idx = np.empty((B, N, k), np.int64)
    res.dist = np.empty((B, N, k), np.float64)
    res.D = np.empty((B, N, N), np.float64)
    res.strict = np.zeros((B, N), bool)
    for b in range(B):
        if res.n_valid[b] < k:
            raise ValueError("k=%d exceeds the %d unmasked rows" % (k, res.n_valid[b]))
        xb = np.where(res.masked[b][:, None], 0.0, x[b].astype(np.float64))
        D = distance_rows(xb)
        D[:, res.masked[b]] = np.inf
        order = np.argsort(D, axis=1, kind='stable')  # stable: the lower index wins a tie
        res.D[b] = D
        res.idx[b] = order[:, :k]
        res.dist[b] = np.take_along_axis(D, order[:, :k], 1)
        m = min(k + 1, int(res.n_valid[b]))
        head = np.take_along_axis(D, order[:, :m], 1)
        gaps_ok = (head[:, 1:] - head[:, :-1]) > t * head[:, 1:]
        res.strict[b] = gaps_ok.all(axis=1) & ~res.masked[b]
        own = np.arange(N)
        res.idx[b][res.masked[b]] = own[res.masked[b], None]
        res.dist[b][res.masked[b]] = 0.0
    return res


def strict_share(res):
    live = ~res.masked
    return float(res.strict[live].mean())


def check(res, idx, strict=False):
    """Acceptance of a product result idx [B, N, k] against the oracle: (a) distinct, in
    range, unmasked; (b) position by position |D[j_m] - D_(m)| <= tau D_(m) (exactly 0
    where D_(m) = 0); (c), when asked, exact indices on the oracle's strict rows.  No row
    is excluded from (a) or (b); masked queries must return themselves."""
    idx = np.asarray(idx).astype(np.int64)
    B, N, k = res.idx.shape
    assert idx.shape == (B, N, k), idx.shape
    t = tau(res.C)
    for b in range(B):
        got, msk = idx[b], res.masked[b]
        own = np.arange(N)[:, None]
        assert np.array_equal(got[msk], np.broadcast_to(own, (N, k))[msk]), "a masked query must return itself"
        g = got[~msk]
        assert g.min() >= 0 and g.max() < N, "index out of range"
        assert not msk[g].any(), "a masked row came back as a neighbour"
        s = np.sort(g, axis=1)
        assert (s[:, 1:] != s[:, :-1]).all(), "duplicate neighbours"
        Dg = np.take_along_axis(res.D[b][~msk], g, 1)
        want = res.dist[b][~msk]
        bad = np.abs(Dg - want) > t * want
        assert not bad.any(), "position check: %d entries off, worst %.3e relative" % (
            bad.sum(), np.max(np.abs(Dg - want)[bad] / np.maximum(want[bad], 1e-300)))
        if strict:
            rows = res.strict[b]
            assert np.array_equal(got[rows], res.idx[b][rows]), "indices differ on %d strict rows" % (
                (got[rows] != res.idx[b][rows]).any(axis=1).sum())


def to_undirected(ei, N):
    """numpy to_undirected of one [2, E] graph: both directions, sorted by (row, col), unique."""
    row = np.concatenate([ei[0], ei[1]]).astype(np.int64)
    col = np.concatenate([ei[1], ei[0]]).astype(np.int64)
    key = np.unique(row * N + col)
    return np.stack([key // N, key % N])


def edge_index(idx):
    """[B, N, k] -> int64 [B, 2, N k]: row 0 the query repeated k times, row 1 the neighbours."""
    B, N, k = idx.shape
    first = np.broadcast_to(np.repeat(np.arange(N), k), (B, N * k))
    return np.stack([first, idx.reshape(B, N * k)], axis=1).astype(np.int64)


# --------------------------------------------------------------------------- fixtures
# name -> (N, C, k); inputs from default_rng(1), standard normal unless stated
SHAPES = {
    "k_eq_n": (50, 3, 50),
    "tails": (257, 5, 7),
    "k1": (700, 33, 1),
    "cora_width": (1000, 80, 64),
    "clustered": (1200, 64, 32),
    "blend_width": (2500, 162, 64),
}
STRICT = ("k_eq_n", "tails", "k1", "clustered")  # fixtures asserted under (c): strict share >= 0.9


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(x fp32 [N, C] read-only, the oracle's Result), computed once per process."""
    N, C, k = SHAPES[name]
    rng = np.random.default_rng(1)
    if name == "clustered":  # 12 centres x 5, noise 0.05: near neighbours with small d / |x|^2
        centres = 5.0 * rng.standard_normal((12, C))
        x = centres[np.arange(N) % 12] + 0.05 * rng.standard_normal((N, C))
    else:
        x = rng.standard_normal((N, C))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x, knn(x, k)


@functools.lru_cache(maxsize=None)
def ties_fixture():
    """Integer coordinates in -3..3, (600, 6), the last 40 rows copies of earlier ones, k = 16:
    every fp32 distance is an exact small integer, ties everywhere."""
    rng = np.random.default_rng(2)
    x = rng.integers(-3, 4, size=(600, 6)).astype(np.float32)
    x[560:] = x[rng.integers(0, 560, size=40)]
    x.setflags(write=False)
    return x, knn(x, 16)


@functools.lru_cache(maxsize=None)
def batch_fixture():
    """B = 3, N = 300, C = 16, k = 8; 0 / 17 / 150 all-zero rows and one NaN row in graph 1."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((3, 300, 16)).astype(np.float32)
    for b, nz in enumerate((0, 17, 150)):
        x[b, rng.choice(300, size=nz, replace=False)] = 0.0
    live = np.flatnonzero(~masked_rows(x[1]))
    x[1, live[5], 3] = np.nan
    x.setflags(write=False)
    return x, knn(x, 8)
