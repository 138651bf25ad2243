"""Frozen rows of the no-grad fixed-grid rk4 solve (gnpde.integrator._frozen_rows, DESIGN.md
section 6.23): rows whose only edge is their own self loop of weight exactly 1.0 and that no
other row gathers have f = 0; the solve leaves them out of every launch but its last, which
takes them through all the steps at once (gnpde_spmm_rhs_frozen_f32).  The result must equal,
bit for bit, the same solve with the path switched off, the path must really be taken (no
silent fallback), and everything it does not cover must fall back and still give the same bits.

The graph (4,500 rows, C = 128, fp32; the node layout forced on): 1,027 frozen rows (odd, no
multiple of 8; 3,473 live rows, odd too), 200 self-loop-only rows of weight 1.0 that live rows
and a hub DO gather (they are not in-degree 1, so they stay live: ops.layout_order), a hub
row of 301 edges whose sources include those, rows without any edge, rows whose single edge
is no self loop, and ordinary rows.
"""
import numpy as np
import pytest
import torch

import gnpde
from gnpde import integrator as gi, ops

DEV = "cuda"
DT = 0.0625  # a power of two: grid times and step sizes exact in fp32
N, C = 4500, 128
NF, NS, NZ, NQ = 1027, 200, 50, 50
OPT = {'block': 'constant', 'function': 'laplacian', 'add_source': False, 'no_alpha_sigmoid': False,
       'max_nfe': 10 ** 9, 'multi_modal': False}
STEPS = (1, 2, 6, 7, 13)  # both sides of GRAPH_MIN_STEPS, odd and even


def _graph(seed=5):
    """edge_index [1,2,E] (row = edge_index[0] aggregates x[edge_index[1]]), weights [1,E], and
    the node groups, in a shuffled user numbering."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(N)
    F, S, Z, Q = np.split(ids[:NF + NS + NZ + NQ], [NF, NF + NS, NF + NS + NZ])
    H = ids[NF + NS + NZ + NQ]
    L = ids[NF + NS + NZ + NQ + 1:]
    gatherable = np.concatenate([S, Z, Q, [H], L])  # everything but the frozen rows
    src, dst, w = [], [], []

    def add(s, d, ww):
        src.append(np.asarray(s).reshape(-1))
        dst.append(np.asarray(d).reshape(-1))
        w.append(np.broadcast_to(np.asarray(ww, np.float32), src[-1].shape).copy())

    add(F, F, 1.0)                                           # frozen: one self loop of weight 1
    add(S, S, 1.0)                                           # the same rows, but gathered by others
    add(Q, rng.choice(L, NQ), rng.uniform(0.2, 1.0, NQ))     # a single edge that is no self loop
    hub_src = np.concatenate([[H], S, rng.choice(L, 100, replace=False)])
    add(np.full(hub_src.size, H), hub_src, rng.uniform(0.001, 0.01, hub_src.size))  # 301 edges
    add(L, L, rng.uniform(0.1, 0.5, L.size))                 # ordinary rows: a self loop ...
    k = 5
    add(np.repeat(L, k), rng.choice(gatherable, L.size * k), rng.uniform(0.02, 0.2, L.size * k))  # ... + 5 edges
    add(L[:NZ], Z, 0.1)                                      # every edge-less row is gathered
    add(L[NZ:NZ + NQ], Q, 0.1)
    add(L[200:210], np.full(10, H), 0.1)
    order = rng.permutation(sum(a.size for a in src))        # COO order is not row order
    ei = np.stack([np.concatenate(src), np.concatenate(dst)])[:, order]
    ww = np.concatenate(w)[order]
    groups = dict(F=F, S=S, Z=Z, Q=Q, H=int(H), L=L)
    return ei[None], ww[None], groups


class Problem(object):
    def __init__(self):
        ei, w, self.groups = _graph()
        self.ei_np, self.w_np = ei, w
        self.ei = torch.from_numpy(ei).to(DEV)
        self.w = torch.from_numpy(w).to(DEV)
        g = torch.Generator(device=DEV)
        g.manual_seed(3)
        self.x = torch.randn(1, N, C, generator=g, device=DEV)
        self.off = {}

    def func(self, ei=None, w=None, add_source=False):
        f = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C, add_source=add_source), DEV).to(DEV)
        with torch.no_grad():
            f.alpha_train.fill_(0.3)
            f.beta_train.fill_(-0.2)
        f.edge_index = self.ei if ei is None else ei
        f.edge_weight = self.w.clone() if w is None else w
        if add_source:
            f.x0 = self.x.clone()
        return f

    def reference(self, n):
        """The n-step solve with the frozen path switched off: computed once per n, never written."""
        if n not in self.off:
            self.off[n] = solve_off(self.func(), self.x, [0.0, n * DT], False)[1]
        return self.off[n]


_problem = []


@pytest.fixture
def pr():
    """The problem (built once), with the node layout forced on for this small state."""
    keep = ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES
    ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES = 0, 0
    try:
        if not _problem:
            _problem.append(Problem())
        yield _problem[0]
    finally:
        ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES = keep


def solve(func, x, times, graph):
    """-> (solution, how many solves took the frozen path)."""
    before = gi.frozen_stats['solves']
    with torch.no_grad():
        z = gnpde.odeint(func, x, torch.tensor(times, device=DEV), method='rk4',
                         options={'step_size': DT, 'gnpde_graph': graph})
    torch.cuda.synchronize()
    return z, gi.frozen_stats['solves'] - before


def solve_off(func, x, times, graph):
    keep = gi.FROZEN_ROWS
    gi.FROZEN_ROWS = False
    try:
        z, taken = solve(func, x, times, graph)
    finally:
        gi.FROZEN_ROWS = keep
    assert taken == 0
    return z


@pytest.mark.gpu
def test_graph_has_what_the_path_must_survive(pr):
    func = pr.func()
    lay = func.node_layout(pr.x)
    assert lay is not None and lay.frozen is not None
    fr, gr = lay.frozen, pr.groups
    assert fr.n_rows == N and fr.n_rows - fr.n_live == NF >= ops.FROZEN_MIN_ROWS
    assert fr.n_live % 2 == 1 and NF % 2 == 1 and NF % 8 != 0
    # the frozen rows are exactly the user rows F; the gathered self-loop-only rows stay live
    tail = set(lay.order[fr.n_live:].tolist())
    assert tail == set(gr['F'].tolist()) and not tail & set(gr['S'].tolist())
    g = lay.graph
    rp = g.csr.rowptr.long()
    ln = (rp[1:] - rp[:-1])
    hub = int(lay.new_id[gr['H']])
    assert int(ln[hub]) > 256 and int(ln[hub]) > g.csr.plan.chunk
    hub_cols = set(g.csr.col[rp[hub]:rp[hub + 1]].tolist())
    assert set(lay.new_id[torch.from_numpy(gr['S']).to(DEV)].tolist()) <= hub_cols
    assert int((ln[lay.new_id[torch.from_numpy(gr['Z']).to(DEV)]] == 0).sum()) == NZ
    assert int((ln[lay.new_id[torch.from_numpy(gr['Q']).to(DEV)]] == 1).sum()) == NQ
    # the plan's last items are the frozen rows, and in-degree is non-increasing
    it = g.csr.plan.items[:g.csr.plan.n_items * 4].view(-1, 4)
    assert torch.equal(it[fr.n_live_items:, 0].long(), torch.arange(fr.n_live, N, device=DEV))
    assert int(it[:fr.n_live_items, 0].max()) < fr.n_live
    deg = g.indeg.long()
    assert bool((deg[1:] <= deg[:-1]).all()) and bool((deg[fr.n_live:] == 1).all())


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "replayed"))
@pytest.mark.parametrize("n", STEPS)
def test_frozen_solve_equals_the_full_solve(pr, n, graph):
    assert gi.GRAPH_MIN_STEPS in range(min(STEPS) + 1, max(STEPS)) and gi.FROZEN_ROWS and gi.RK4_INPLACE
    func = pr.func()
    keep = pr.x.clone()
    want = pr.reference(n)
    z, taken = solve(func, pr.x, [0.0, n * DT], graph)
    assert taken == 1
    assert torch.equal(z[0], keep) and torch.equal(pr.x, keep)  # the caller's y0 is untouched
    assert torch.equal(z[1], want)
    # again on the same module: its pool, its captured graphs, the rows the last solve left in a and b
    z2, taken = solve(func, pr.x, [0.0, n * DT], graph)
    assert taken == 1 and torch.equal(z2[1], want) and torch.equal(pr.x, keep)


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "replayed"))
def test_shorter_last_step(pr, graph):
    """The frozen rows are taken through all the steps by the solve's last launch, with that
    launch's coefficients: a last step of another size (6.5 steps of DT) gives the same bits."""
    times = [0.0, 6.5 * DT]
    want = solve_off(pr.func(), pr.x, times, graph)[1]
    z, taken = solve(pr.func(), pr.x, times, graph)
    assert taken == 1 and torch.equal(z[1], want)
    assert not torch.equal(want, pr.reference(6)) and not torch.equal(want, pr.reference(7))


@pytest.mark.gpu
def test_frozen_solve_vs_float64_oracle(pr):
    import gnpde_oracle as O
    n = 7
    A = O.LaplacianCSR(pr.ei_np, pr.w_np, N, dtype=np.float64)
    z, taken = solve(pr.func(), pr.x, [0.0, n * DT], None)
    assert taken == 1
    want = O.odeint_fixed(lambda tt, y: A.rhs(y, 0.3), pr.x.cpu().numpy(), 0.0, n * DT, 'rk4', DT)
    err = float(np.abs(z[1].double().cpu().numpy() - want).max() / np.abs(want).max())
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_fallbacks_are_not_frozen_and_give_the_same_bits(pr):
    n = 7
    sl = ((pr.ei[0, 0] == pr.ei[0, 1]) & (pr.ei[0, 0] == int(pr.groups['F'][17]))).nonzero().view(-1)
    assert sl.numel() == 1
    # one frozen row's weight is not 1
    w = pr.w.clone()
    w[0, sl] = 0.5
    z, taken = solve(pr.func(w=w), pr.x, [0.0, n * DT], None)
    assert taken == 0 and torch.equal(z[1], solve_off(pr.func(w=w.clone()), pr.x, [0.0, n * DT], None)[1])
    assert not torch.equal(z[1], pr.reference(n))
    # a source term
    z, taken = solve(pr.func(add_source=True), pr.x, [0.0, n * DT], None)
    assert taken == 0
    assert torch.equal(z[1], solve_off(pr.func(add_source=True), pr.x, [0.0, n * DT], None)[1])
    # B = 2
    ei2, w2, x2 = pr.ei.expand(2, -1, -1).contiguous(), pr.w.expand(2, -1).contiguous(), torch.cat([pr.x, -pr.x])
    z, taken = solve(pr.func(ei=ei2, w=w2), x2, [0.0, n * DT], None)
    assert taken == 0 and torch.equal(z[1], solve_off(pr.func(ei=ei2, w=w2.clone()), x2, [0.0, n * DT], None)[1])
    assert torch.equal(z[1][0], pr.reference(n)[0])
    # three output times
    times = [0.0, 3 * DT, n * DT]
    z, taken = solve(pr.func(), pr.x, times, None)
    assert taken == 0 and torch.equal(z, solve_off(pr.func(), pr.x, times, None))
    assert torch.equal(z[2], pr.reference(n))


@pytest.mark.gpu
@pytest.mark.parametrize("graph", (False, True), ids=("eager", "replayed"))
def test_weights_edited_in_place_drop_the_path(pr, graph):
    n = 7
    func = pr.func()
    z, taken = solve(func, pr.x, [0.0, n * DT], graph)
    assert taken == 1 and torch.equal(z[1], pr.reference(n))
    loops = (pr.ei[0, 0] == pr.ei[0, 1]).nonzero().view(-1)
    with torch.no_grad():
        func.edge_weight[0, loops] *= 0.75  # every self loop, the frozen rows' among them
    z, taken = solve(func, pr.x, [0.0, n * DT], graph)
    assert taken == 0
    want = solve_off(pr.func(w=func.edge_weight.clone()), pr.x, [0.0, n * DT], graph)[1]
    assert torch.equal(z[1], want) and not torch.equal(want, pr.reference(n))
    # back to unit weights: the path returns
    with torch.no_grad():
        func.edge_weight.copy_(pr.w)
    z, taken = solve(func, pr.x, [0.0, n * DT], graph)
    assert taken == 1 and torch.equal(z[1], pr.reference(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 7))
def test_non_finite_and_negative_zero_in_frozen_rows(pr, n):
    """Today's kernel turns an infinite entry of such a row into NaN (inf - inf) and -0.0 into
    +0.0; the frozen tail runs the same epilogue on the same inputs, so it does too."""
    x = pr.x.clone()
    F = torch.from_numpy(pr.groups['F']).to(DEV)
    x[0, F[0], 0:8] = float('inf')
    x[0, F[1], 3] = float('-inf')
    x[0, F[2], 64:70] = float('nan')
    x[0, F[3], :] = -0.0
    x[0, F[1026], 127] = float('inf')
    x[0, F[5], 5] = -0.0
    want = solve_off(pr.func(), x, [0.0, n * DT], None)[1]
    z, taken = solve(pr.func(), x, [0.0, n * DT], None)
    assert taken == 1
    torch.testing.assert_close(z[1], want, rtol=0, atol=0, equal_nan=True)
    assert bool(torch.isnan(z[1][0, F[0], 0:8]).all()) and bool(torch.isnan(z[1][0, F[1], 3]))
    assert not bool(torch.signbit(z[1][0, F[3]]).any())  # -0.0 became +0.0, as it does in the full launch
    rest = torch.ones(N, dtype=torch.bool, device=DEV)
    rest[F[:6]] = False
    rest[F[1026]] = False
    assert torch.equal(z[1][0, rest], pr.reference(n)[0, rest])


def test_layout_order_key_cpu():
    """ops.layout_order on the CPU: in-degree non-increasing, the self-loop-only rows of
    in-degree 1 last in their class — with no row of in-degree 0, exactly the rows [n_live, R) —
    and order / new_id inverse permutations."""
    rng = np.random.default_rng(0)
    R = 3001
    deg = torch.from_numpy(rng.integers(1, 6, size=R))
    cand = torch.from_numpy(rng.random(R) < 0.4)  # self-loop-only rows, some gathered by others too
    order = ops.layout_order(deg.view(1, R), cand.view(1, R)).view(R)
    new_id = torch.empty_like(order)
    new_id[order] = torch.arange(R)
    ar = torch.arange(R)
    assert torch.equal(new_id[order], ar) and torch.equal(order[new_id], ar)
    d = deg[order]
    assert bool((d[1:] <= d[:-1]).all())
    frozen = cand & (deg == 1)
    nf = int(frozen.sum())
    assert 0 < nf < R
    assert torch.equal(torch.sort(order[R - nf:]).values, frozen.nonzero().view(-1))
    # stable: inside every (in-degree, frozen) class the rows keep their order
    for lo, hi in ((0, R - nf), (R - nf, R)):
        seg = order[lo:hi]
        for v in d[lo:hi].unique().tolist():
            s = seg[d[lo:hi] == v]
            assert bool((s[1:] > s[:-1]).all())
    # rows of in-degree 0 sort behind the candidates
    deg0 = deg.clone()
    deg0[:7] = 0
    o0 = ops.layout_order(deg0.view(1, R), cand.view(1, R)).view(R)
    assert set(o0[R - 7:].tolist()) == set(range(7))
    # the same graph-only classification, from a CSR
    rowptr = torch.tensor([0, 1, 1, 3, 4, 5], dtype=torch.int32)
    col = torch.tensor([0, 2, 0, 1, 4], dtype=torch.int32)
    assert ops.self_loop_only_rows(rowptr, col, 5, 5).tolist() == [True, False, False, False, True]
