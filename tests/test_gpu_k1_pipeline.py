"""K1's pipelined edge loop (csrc/aggregate.hpp) on a small graph: rows of 0 .. 700 edges — around
the 4- and 8-edge batches, and long rows — several of each per wavefront, the last row slot of
the launch empty.

The graph has fewer than ops.SMALL_GRAPH_ROWS rows and is built with the default split, so every
row of more than ops.SMALL_CHUNK = 16 edges is a hub of chunks of at most 16 edges: what runs here
is the loop's first 32-edge chunk of a row slot (always its LAST one), the short batches, and the
in-launch hub combine of 2 .. 44 chunks.  The second and later chunks of a row slot, the
next-chunk column prefetch and the 256-edge items of the large graphs are run by
tests/test_gpu_long_items.py, on the same row lengths at chunk = 256.

The schedule is not allowed to move a bit: tests/golden/k1_pipeline/rk4_c128_rows.npy holds
64 rows of the three-step rk4 result at C = 128 as the library computed them BEFORE the
loop was pipelined (edges of a row summed in CSR order, acc = fmaf(w, x, acc)), at this split.
"""
import os

import numpy as np
import pytest
import torch

import gnpde
from conftest import GOLDEN
from gnpde import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
# the tolerances of tests/test_gpu_parity.py for the same comparisons
RTOL = 1e-5        # fp32 RHS and fixed-grid integration against the fp64 reference
BF16_TOL = 2e-2    # bf16 against the fp64 reference on the unrounded inputs
BF16_ROUND = 4e-3  # bf16 RHS against the reference on the same bf16-rounded inputs

GOLDEN_ROWS = os.path.join(GOLDEN, "k1_pipeline", "rk4_c128_rows.npy")

# edges per row: empty, self loop only, around the 4- and 8-edge batches and the 16-edge split, and
# hubs of 2 .. 44 chunks (at this graph's 16-edge split no item reaches a second 32-edge chunk of a
# row slot; the lengths around 32, 64 and 256 are boundaries at chunk = 256: test_gpu_long_items.py)
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65, 255, 256, 257, 700)
ALPHA, BETA = 0.3, -0.2
STEPS, DT = 3, 0.1


def _repeats(L):
    # enough rows of each length that a wavefront (1-16 row slots) meets several of them
    return 260 if L <= 9 else 60 if L <= 65 else 12 if L <= 257 else 3


class Case(object):
    """The graph and its inputs, built once on the host from fixed seeds."""

    def __init__(self):
        rng = np.random.default_rng(20250)
        lens = np.concatenate([np.full(_repeats(L), L) for L in LENGTHS])
        lens = lens[rng.permutation(lens.size)]
        g = self._graph(lens, rng)
        if g.csr.plan.n_items % 2 == 0:  # an odd item count: the last wavefront's last row slot is empty
            lens = np.concatenate([lens, [0]])
            g = self._graph(lens, rng)
        assert g.chunk == ops.SMALL_CHUNK  # the small-graph split: the golden rows were recorded at it
        assert g.csr.plan.n_items % 2 == 1 and g.csr.plan.n_heavy >= 3
        self.graph, self.lens, self.N = g, lens, lens.size
        self.w = rng.uniform(0.1, 1.0, size=(1, self.ei.shape[2])).astype(np.float32)
        self.w /= 8.0  # row sums of O(1): the flow stays bounded
        self.rng = rng

    def _graph(self, lens, rng):
        N = lens.size
        src = np.repeat(np.arange(N), lens)
        dst = rng.integers(0, N, size=src.size)
        first = np.cumsum(lens) - lens
        dst[first[lens > 0]] = np.arange(N)[lens > 0]  # every non-empty row holds its self loop
        p = np.random.default_rng(7).permutation(src.size)
        self.ei = np.stack([src[p], dst[p]])[None]
        return ops.GraphCSR(torch.from_numpy(self.ei).to(DEV), N)

    def state(self, C):
        r = np.random.default_rng(1000 + C)
        return (r.standard_normal((1, self.N, C)).astype(np.float32),
                r.standard_normal((1, self.N, C)).astype(np.float32))


@pytest.fixture(scope="module")
def case():
    return Case()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rel(a, b):
    return float((a.detach().double().cpu() - b).abs().max() / b.abs().max())


def ref_rhs(case, x, x0):
    """sigma(alpha) (A x - x) + beta x0 in fp64 (torch, host)."""
    src, dst = torch.from_numpy(case.ei[0, 0]), torch.from_numpy(case.ei[0, 1])
    w = torch.from_numpy(case.w[0]).double()
    ax = torch.zeros_like(x[0]).index_add_(0, src, w[:, None] * x[0][dst])
    return (1.0 / (1.0 + np.exp(-ALPHA)) * (ax - x[0]) + BETA * x0[0])[None]


def ref_rk4(case, x, x0):
    """STEPS steps of the 3/8-rule rk4 (torchdiffeq rk4_alt_step_func) in fp64."""
    y = x
    f = lambda v: ref_rhs(case, v, x0)  # noqa: E731
    for _ in range(STEPS):
        k1 = f(y)
        k2 = f(y + DT * k1 / 3.0)
        k3 = f(y + DT * (k2 - k1 / 3.0))
        k4 = f(y + DT * (k1 - k2 + k3))
        y = y + (k1 + 3.0 * (k2 + k3) + k4) * DT * 0.125
    return y


OPT = {'hidden_dim': 0, 'block': 'constant', 'add_source': True, 'no_alpha_sigmoid': False, 'max_nfe': 10 ** 6,
       'multi_modal': False}


def make_func(case, C, x0, dtype):
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C), DEV).to(DEV)
    with torch.no_grad():
        func.alpha_train.fill_(ALPHA)
        func.beta_train.fill_(BETA)
    func.edge_index, func.edge_weight, func.x0 = T(case.ei), T(case.w), T(x0).to(dtype)
    return func


def rk4(case, C, dtype, graph):
    x, x0 = case.state(C)
    func = make_func(case, C, x0, dtype)
    with torch.no_grad():
        z = gnpde.odeint(func, T(x).to(dtype), torch.tensor([0.0, STEPS * DT], device=DEV), method='rk4',
                         options={'step_size': DT, 'gnpde_graph': graph})
    torch.cuda.synchronize()
    return z[1]


def golden_rows(case):
    return np.sort(np.random.default_rng(64).choice(case.N, size=64, replace=False))


CASES = [(128, torch.float32), (64, torch.float32), (7, torch.float32), (162, torch.float32),
         (256, torch.float32), (162, torch.bfloat16)]
IDS = ["%d-%s" % (C, "bf16" if dt == torch.bfloat16 else "fp32") for C, dt in CASES]


@pytest.mark.parametrize("C,dtype", CASES, ids=IDS)
def test_plain_rhs_vs_fp64(case, C, dtype):
    x, x0 = case.state(C)
    g = case.graph
    wc = g.gather_weights(T(case.w))
    a, b = torch.tensor(ALPHA, device=DEV), torch.tensor(BETA, device=DEV)
    xd, x0d = T(x).to(dtype), T(x0).to(dtype)
    f = ops.spmm_rhs(g, wc, xd, x0d, a, b, add_source=True)
    f2 = ops.spmm_rhs(g, wc, xd, x0d, a, b, add_source=True)
    assert torch.equal(f, f2)  # two runs, equal bits
    want = ref_rhs(case, torch.from_numpy(x).double(), torch.from_numpy(x0).double())
    if dtype == torch.float32:
        err = rel(f, want)
        print("C=%d fp32 RHS rel err %.3e" % (C, err))
        assert err <= RTOL
    else:
        want_r = ref_rhs(case, xd.double().cpu(), x0d.double().cpu())
        err, err_r = rel(f, want), rel(f, want_r)
        print("C=%d bf16 RHS rel err %.3e (rounded inputs %.3e)" % (C, err, err_r))
        assert err_r <= BF16_ROUND and err <= BF16_TOL
    # the rows without edges: sigma(alpha) (0 - x) + beta x0, whatever their wavefront's other rows did
    empty = torch.from_numpy(np.flatnonzero(case.lens == 0)).to(DEV)
    if dtype == torch.float32:
        assert rel(f[0][empty], want[0][empty.cpu()]) <= RTOL
    else:  # against the reference on the same bf16-rounded inputs
        assert rel(f[0][empty], want_r[0][empty.cpu()]) <= BF16_ROUND


@pytest.mark.parametrize("C,dtype", CASES, ids=IDS)
def test_fused_rk4_steps_vs_fp64_and_bitwise(case, C, dtype):
    z = rk4(case, C, dtype, graph=False)
    assert torch.equal(z, rk4(case, C, dtype, graph=False))  # two runs, equal bits
    assert torch.equal(z, rk4(case, C, dtype, graph=True))   # eager and graph-replayed steps, equal bits
    x, x0 = case.state(C)
    want = ref_rk4(case, torch.from_numpy(x).double(), torch.from_numpy(x0).double())[0]
    err = rel(z.float(), want)
    print("C=%d %s rk4 x%d rel err %.3e" % (C, dtype, STEPS, err))
    assert err <= (RTOL if dtype == torch.float32 else BF16_TOL)


def test_rk4_c128_rows_equal_the_unpipelined_kernel(case):
    z = rk4(case, 128, torch.float32, graph=False)
    got = z[0][torch.from_numpy(golden_rows(case)).to(DEV)].cpu()
    want = torch.from_numpy(np.load(GOLDEN_ROWS))
    assert want.shape == (64, 128) and want.dtype == torch.float32
    assert torch.equal(got, want)
