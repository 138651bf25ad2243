"""float64 oracle of the positional-encoding distance rewiring (gnpde.graph_rewiring
apply_pos_dist_rewire) and the acceptance checks the host and the GPU tests share.

Definitions (per graph, x [N, C]):

    q_i  = |x_i|^2
    d_ij = sum_c (x_ic - x_jc)^2
    u_ij = d_ij r_i r_j,  r_i = 1 / max(1 - q_i, eps), eps = 2^-52     ('poincare')
    u_ij = d_ij                                                         ('euclid')
    D_ij = arccosh(1 + 2 u_ij)  ('poincare'),   D_ij = sqrt(u_ij)  ('euclid')
    topk:      row i -> the k columns of smallest D_ij, the self index included (D_ii = 0,
               sklearn's `precomputed` kNN), in ascending (D_ij, j)
    threshold: thr = numpy.quantile(D, quant) over all N^2 entries (linear interpolation);
               edges = numpy.where(D <= thr)

D is monotone in u, so every ranking here is taken on u (arccosh and sqrt can merge two u
that differ in the last bit; u is the sharper key).  arccosh(1 + 2u) is evaluated as
log1p(2u + 2 sqrt(u (u + 1))), the same function without the cancellation of 1 + 2u.

Set identity: with M = N^2, pos = quant (M - 1), lo = floor(pos), linear interpolation gives
v_(lo) <= thr <= v_(lo+1), and thr = v_(lo+1) only when v_(lo+1) = v_(lo) or pos is an integer
(then lo is that index).  So {D <= thr} = {D <= v_(lo)} = {u <= u_(lo)}: one order statistic.

Tolerance tau(C, q_i, q_j), the relative error bound of the product's fp32 u_ij, from its
arithmetic (e = 2^-24, the fp32 unit roundoff; E = 2^-53, fp64's):

* d: every difference is rounded once (1 e on the difference, 2 e on its square) and the C
  non-negative squares are accumulated by fused multiply-adds, one rounding each; as in
  knn_oracle.tau, any order of the sum is within (C + 3) e of the exact value.
* r ('poincare' only; 'euclid' multiplies by exactly 1): q is summed in fp64 from exact
  squares (fp32 squares fit fp64), (C + 1) E relative; 1 - q then carries that error amplified
  by the cancellation, q / |1 - q| (C + 1) E, plus its own rounding E; the reciprocal adds E and
  the rounding of r to fp32 adds e:  rho_i = e + (2 + (C + 1) q_i / |1 - q_i|) E.
  A row whose 1 - q lies within 4 (C + 1) E q of eps ("on the rim": the clamp's decision is
  not determined) gets tau = inf, i.e. all its entries are undecided.  A clamped row has
  r = 2^52 exactly (rho = 0).
* u = d (r_i r_j): two more fp32 roundings, 2 e.

  tau = ((C + 3) e + rho_i + rho_j + 2 e) (1 + 1e-6)     (the factor covers second order)

The product's threshold (or a row's k-th value) is itself an fp32 u of some entry, and an order
statistic of perturbed values moves by at most the largest perturbation; so against the
oracle's value u* an entry is decided when it clears u* by its own tau plus the largest tau of
the matrix (`decide`).  The undecided entries, other than the entry that IS u*, are the band.
(With an empty band the boundary entry is pinned too: the product returns exactly k distinct
indices per row, and its edge count is checked against count_le.)
"""
import functools

import numpy as np

EPS = 2.0 ** -52
E32 = 2.0 ** -24
E64 = 2.0 ** -53
BAND_SHARE = 0.01   # the band may hold at most this share of the kept entries


def sq_norms(x):
    x = np.asarray(x, np.float64)
    return np.einsum('nc,nc->n', x, x)


def rank_values(x, metric):
    """float64 u [N, N]."""
    x = np.asarray(x, np.float64)
    N, C = x.shape
    d = np.empty((N, N), np.float64)
    rows = max(1, (1 << 26) // max(1, 8 * N * C))
    for r0 in range(0, N, rows):
        diff = x[r0:r0 + rows, None, :] - x[None, :, :]
        d[r0:r0 + rows] = np.einsum('rnc,rnc->rn', diff, diff)
    if metric == 'euclid':
        return d
    assert metric == 'poincare', metric
    r = 1.0 / np.maximum(1.0 - sq_norms(x), EPS)
    return d * np.outer(r, r)     # (symmetric to the bit, as d is)


def dist_from_u(u, metric):
    u = np.asarray(u, np.float64)
    if metric == 'euclid':
        return np.sqrt(u)
    return np.log1p(2.0 * u + 2.0 * np.sqrt(u * (u + 1.0)))


def distances(x, metric):
    return dist_from_u(rank_values(x, metric), metric)


def tau(C, qi, qj, metric='poincare'):
    """The relative error bound of the fp32 u_ij (module docstring); broadcasts over q."""
    qi, qj = np.asarray(qi, np.float64), np.asarray(qj, np.float64)
    base = (C + 3) * E32
    if metric == 'euclid':
        return np.broadcast_to(base * (1 + 1e-6), np.broadcast(qi, qj).shape).copy()

    def rho(q):
        gap = 1.0 - q
        rim = np.abs(gap - EPS) <= 4 * (C + 1) * E64 * q
        with np.errstate(divide='ignore', invalid='ignore'):
            r = E32 + (2 + (C + 1) * q / np.abs(gap)) * E64
        r = np.where(gap < EPS, 0.0, r)
        return np.where(rim, np.inf, r)
    return (base + rho(qi) + rho(qj) + 2 * E32) * (1 + 1e-6)


def tau_matrix(x, metric):
    q = sq_norms(x)
    return tau(np.asarray(x).shape[1], q[:, None], q[None, :], metric)


def pair_rank(N, quant):
    """(lo, hi, frac) of numpy.quantile's linear method among M = N^2 values, from exact
    rational arithmetic on the float quant."""
    from fractions import Fraction
    M = N * N
    pos = Fraction(float(quant)) * (M - 1)
    lo = int(pos.numerator // pos.denominator)
    return lo, min(lo + 1, M - 1), float(pos - lo)


def quantile_threshold(u, quant, metric):
    """(thr, u_lo): numpy.quantile of D over all entries, and the order statistic u_(lo)."""
    N = u.shape[0]
    thr = float(np.quantile(dist_from_u(u, metric), quant))
    lo = pair_rank(N, quant)[0]
    return thr, float(np.partition(u.reshape(-1), lo)[lo])


def threshold_edges(u, quant, metric):
    """numpy.where(D <= numpy.quantile(D, quant)) as int64 [2, E]."""
    D = dist_from_u(u, metric)
    return np.stack(np.where(D <= np.quantile(D, quant))).astype(np.int64)


def knn(u, k):
    """idx [N, k]: ascending (u, j), stable."""
    return np.argsort(u, axis=1, kind='stable')[:, :k]


def decide(u, tm, ustar):
    """(keep, drop): the entries surely at or below / surely above a product threshold whose
    exact value is within the matrix's largest finite tau of ustar (ustar: scalar, or [N, 1]
    per row).  The rest is the band."""
    tmax = np.max(tm[np.isfinite(tm)]) if np.isfinite(tm).any() else 0.0
    with np.errstate(invalid='ignore'):
        keep = u * (1 + tm) <= ustar * (1 - tmax)
        drop = u * (1 - tm) > ustar * (1 + tmax)
    keep &= np.isfinite(tm)
    drop &= np.isfinite(tm)
    return keep, drop


def check_edges(u, tm, u_lo, ei, what=""):
    """Acceptance of a product edge list ei [2, E] against the oracle's rank values: numpy.where
    order without duplicates; every emitted edge has u <= u_lo (1 + tau) (it is not surely
    above), every entry surely below is present; the band holds at most BAND_SHARE of the kept
    entries (a condition on the fixture: it fails, it does not skip).  Returns the band size."""
    N = u.shape[0]
    ei = np.asarray(ei)
    assert ei.dtype == np.int64 and ei.ndim == 2 and ei.shape[0] == 2, (ei.dtype, ei.shape)
    assert ei.size == 0 or (ei.min() >= 0 and ei.max() < N)
    key = ei[0] * N + ei[1]
    assert (np.diff(key) > 0).all(), "%s: not in numpy.where order, or duplicates" % what
    got = np.zeros((N, N), bool)
    got[ei[0], ei[1]] = True
    keep, drop = decide(u, tm, u_lo)
    band = ~keep & ~drop & (u != u_lo)      # (the boundary entry itself is the oracle's, not an undecided one)
    kept = int((u <= u_lo).sum())
    print("%s: E=%d, oracle keeps %d, band %d" % (what, ei.shape[1], kept, band.sum()))
    assert band.sum() <= BAND_SHARE * kept, "%s: band of %d entries over %d kept" % (what, band.sum(), kept)
    assert not (got & drop).any(), "%s: %d emitted edges above u_lo (1 + tau)" % (what, (got & drop).sum())
    assert not (~got & keep).any(), "%s: %d edges below the band missing" % (what, (~got & keep).sum())
    return int(band.sum())


def check_knn(u, tm, k, idx, what=""):
    """Acceptance of product kNN indices idx [N, k] (rows without a non-finite value): in range
    and distinct per row; as a set, nothing surely above the oracle's k-th value and everything
    surely below it; non-decreasing u along a row up to tau; band <= BAND_SHARE of N k."""
    N = u.shape[0]
    idx = np.asarray(idx).astype(np.int64)
    assert idx.shape == (N, k), idx.shape
    assert idx.min() >= 0 and idx.max() < N
    s = np.sort(idx, axis=1)
    assert (s[:, 1:] != s[:, :-1]).all(), "%s: duplicate neighbours" % what
    kth = np.sort(u, axis=1)[:, k - 1:k]
    keep, drop = decide(u, tm, kth)
    band = ~keep & ~drop & (u != kth)       # (the boundary entry itself is the oracle's, not an undecided one)
    print("%s: band %d of %d kept" % (what, band.sum(), N * k))
    assert band.sum() <= BAND_SHARE * N * k, "%s: band of %d entries over %d kept" % (what, band.sum(), N * k)
    got = np.zeros((N, N), bool)
    got[np.arange(N)[:, None], idx] = True
    assert not (got & drop).any(), "%s: %d neighbours above the k-th value's band" % (what, (got & drop).sum())
    assert not (~got & keep).any(), "%s: %d neighbours below the band missing" % (what, (~got & keep).sum())
    ug = np.take_along_axis(u, idx, 1)
    tg = np.take_along_axis(tm, idx, 1)
    tg = np.where(np.isfinite(tg), tg, 1.0)
    assert (ug[:, :-1] * (1 - tg[:, :-1]) <= ug[:, 1:] * (1 + tg[:, 1:])).all(), "%s: rows not ascending" % what
    return int(band.sum())


def edge_index(idx):
    """[N, k] -> int64 [2, N k]: row 0 the query repeated k times, row 1 the neighbours."""
    N, k = idx.shape
    return np.stack([np.repeat(np.arange(N), k), idx.reshape(-1)]).astype(np.int64)


# --------------------------------------------------------------------------- fixtures
# name -> (N, C, k, seed); points inside the unit ball (both metrics read the same x)
SHAPES = {
    "one": (1, 4, 1, 1),            # M = 1
    "partial": (63, 3, 7, 1),       # one partial tile, odd C
    "hyps16": (165, 16, 16, 1),     # HYPS16's width, three row tiles, tile tails, diagonal and off-diagonal tiles
    "chunks33": (300, 33, 64, 1),   # two column chunks, a short second one
    "dw64": (300, 64, 64, 1),       # DW64's width, two whole chunks
    "rim": (165, 16, 16, 2),        # norms up to 0.95, one row at |x| = 1.5 (the eps clamp), one at the origin
}
METRICS = ("poincare", "euclid")
# quantiles per fixture: 0, 1/1000, 1/100, a value whose position is an integer, 0.5, 1.  The
# integer position is covered at N = 63 and 165 ((M - 1) / 4 is an integer and 0.25 an exact
# float) and trivially at N = 1; the N = 300 fixtures have NONE: M - 1 = 89,999 has no divisor
# that makes quant (M - 1) an exact float product.
QUANTS = {
    "one": (0.0, 0.001, 0.5, 1.0),
    "partial": (0.0, 0.001, 0.25, 0.5, 1.0),
    "hyps16": (0.0, 0.001, 0.01, 0.25, 0.5, 1.0),
    "chunks33": (0.0, 0.001, 0.01, 0.5, 1.0),
    "dw64": (0.0, 0.001, 0.01, 0.5, 1.0),
    "rim": (0.0, 0.001, 0.01, 0.25, 0.5, 1.0),
}


@functools.lru_cache(maxsize=None)
def points(name):
    """x fp32 [N, C], read-only."""
    N, C, _k, seed = SHAPES[name]
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((N, C))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    hi = 0.95 if name == "rim" else 0.8
    x = v * rng.uniform(0.05, hi, size=(N, 1))
    if name == "rim":
        x[17] = 1.5 * v[17]
        x[100] = 0.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fixture(name, metric):
    """(x, u float64 [N, N], tau [N, N]), computed once per process; read-only."""
    x = points(name)
    u = rank_values(x, metric)
    tm = tau_matrix(x, metric)
    u.setflags(write=False)
    tm.setflags(write=False)
    return x, u, tm


@functools.lru_cache(maxsize=None)
def ties_points():
    """Lattice points k / 8, k in -3..3, (200, 4), the last 40 rows copies of earlier ones: every
    Euclidean d is an exact multiple of 1/64 in fp32 and in float64, ties everywhere."""
    rng = np.random.default_rng(4)
    x = rng.integers(-3, 4, size=(200, 4)).astype(np.float32) / 8
    x[160:] = x[rng.integers(0, 160, size=40)]
    x.setflags(write=False)
    return x
