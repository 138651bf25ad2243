"""Golden fixtures of the positional-encoding distance rewiring: tests/golden/posdist/*.npz.

The reference's own lines do not run (hyperbolic_distances.hyperbolize passes `initial=` to
np.maximum; distances_kNN imports DistanceMetric from where it no longer lives and loops
`for i in len(x)`), so the fixtures are produced with the libraries those lines call, composed
as they intend:

    squared distances    scipy.spatial.distance.pdist(x, 'sqeuclidean') / squareform
    hyperbolic D         arccosh(1 + 2 d / (max(1 - q_i, eps) max(1 - q_j, eps))), eps = float64 eps
    Euclidean D          scipy pdist(x, 'euclidean') / squareform
    kNN                  sklearn.neighbors.NearestNeighbors(n_neighbors=k, metric='precomputed')
    threshold            numpy.quantile(D, quant) and numpy.where(D <= thr)

Inputs: posdist_oracle.points(name), cast to float64.  Each file holds x, D (float64), knn
(sklearn's indices, int32), quants, thr (one per quant) and edges_<i> (int32 [2, E], one per
quant).  Run from the repository root:  python tests/golden/gen_golden_posdist.py
"""
import json
import os
import sys

import numpy as np
from scipy.spatial.distance import pdist, squareform
from sklearn.neighbors import NearestNeighbors

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import posdist_oracle as PO  # noqa: E402

OUT_DIR = os.path.join(HERE, "posdist")
NAMES = ("partial", "hyps16", "rim")
QUANTS = (0.001, 0.01, 0.25)


def dense(x, metric):
    if metric == 'euclid':
        return squareform(pdist(x, 'euclidean'))
    d = squareform(pdist(x, 'sqeuclidean'))
    den = np.maximum(1.0 - np.sum(x ** 2, axis=1), np.finfo(np.double).eps)
    return np.arccosh(1.0 + 2.0 * d / (den[:, None] * den[None, :]))


def main():
    os.makedirs(OUT_DIR, exist_ok=True)
    names = []
    for name in NAMES:
        k = PO.SHAPES[name][2]
        x = np.asarray(PO.points(name), np.float64)
        for metric in PO.METRICS:
            D = dense(x, metric)
            nbrs = NearestNeighbors(n_neighbors=k, metric='precomputed').fit(D)
            idx = nbrs.kneighbors(D)[1]
            out = dict(x=PO.points(name), D=D, knn=idx.astype(np.int32), quants=np.array(QUANTS))
            thr = []
            for i, q in enumerate(QUANTS):
                t = np.quantile(D, q, axis=None)
                thr.append(t)
                out["edges_%d" % i] = np.stack(np.where(D <= t)).astype(np.int32)
            out["thr"] = np.array(thr)
            fn = "%s_%s.npz" % (name, metric)
            np.savez_compressed(os.path.join(OUT_DIR, fn), **out)
            names.append(fn)
            print(fn, os.path.getsize(os.path.join(OUT_DIR, fn)))
    with open(os.path.join(OUT_DIR, "MANIFEST.json"), "w") as fh:
        json.dump(sorted(names), fh, indent=1)


if __name__ == "__main__":
    main()
