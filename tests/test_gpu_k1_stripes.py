"""K1's column stripes (agg_stripe_kernel, csrc/aggregate.hpp): on a large
graph the headline geometry — plain weights, fp32 rows of 65-128 columns, stage kinds 0 and 1 —
has every workgroup aggregate 128 / S columns of all its rows and deals the stripes to the XCDs.
The mapping must change no bit: every comparison here is torch.equal against the same library
with the stripes switched off (gnpde_k1_stripes_set(0): the setting GNPDE_K1_STRIPES=0 gives),
and every striped run asserts on the library's counter of striped launches, so a launch that
quietly took the unstriped kernel fails.

Row lengths 0 .. 700 under both plan orders, split at chunk = 256 (hubs of 2 and 3 chunks) and
at chunk = 16 (hubs of 2, 3, 4, 5, 16, 17 and 44 chunks; a row of at most `chunk` edges is one
item, so a hub has at least two chunks), in graphs whose items fill 1, 7, 8, 9 and 94 item
blocks of S = 4 (32 items each; 2, 14, 16, 17 and 188 of S = 2): workgroups without work behind
the last item block in every stripe, and a last block that is partly filled.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import gnpde
from gnpde import _lib, integrator as gi, ops
from test_gpu_k1_pipeline import ALPHA, BETA, RTOL, T, rel
from test_gpu_long_items import GOLDEN_ROWS, build_graph
import test_gpu_frozen_rows as FR
import test_gpu_long_items as LI

pytestmark = pytest.mark.gpu
DEV = "cuda"
ORDERS = ("classes", "rows")
LENGTHS = (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 255, 256, 257, 700, 80)  # 80: five chunks of 16
ITEMS = (30, 219, 256, 270, 3000)  # item blocks of 32 items: 1, 7, 8 (a full last block), 9, 94
STRIPES = (4, 2)


@contextlib.contextmanager
def stripes(s):
    """The library's stripe setting forced to ``s`` (0, 2, 4) for every launch of the geometry."""
    _lib.call("gnpde_k1_stripes_set", s)
    try:
        yield
    finally:
        _lib.call("gnpde_k1_stripes_set", -1)


def striped_launches():
    return int(_lib.fn("gnpde_k1_striped_launches")())


def run(s, fn, launches=None):
    """fn() under stripe setting ``s``; a striped run must have issued striped launches
    (``launches`` of them, when given), an unstriped run none."""
    with stripes(s):
        before = striped_launches()
        out = fn()
        torch.cuda.synchronize()
        n = striped_launches() - before
    if s == 0:
        assert n == 0
    else:
        assert n > 0 if launches is None else n == launches, (s, n, launches)
    return out


def n_items_of(L, chunk):
    return 1 if L <= chunk else -(-L // chunk)


def lengths_for(target, chunk):
    """Row lengths, cycling through LENGTHS, whose plan at ``chunk`` holds exactly ``target`` items."""
    lens, used, idle, i = [], 0, 0, 0
    while used < target and idle < len(LENGTHS):
        L = LENGTHS[i % len(LENGTHS)]
        i += 1
        k = n_items_of(L, chunk)
        if used + k <= target:
            lens.append(L)
            used += k
            idle = 0
        else:
            idle += 1
    lens += [1] * (target - used)
    return np.asarray(lens)


class Graph(object):
    """Rows of the given lengths in a shuffled order; every non-empty row holds its self loop."""

    def __init__(self, target, chunk):
        rng = np.random.default_rng(1000 * chunk + target)
        lens = lengths_for(target, chunk)
        lens = lens[rng.permutation(lens.size)]
        self.lens, self.N, self.chunk = lens, lens.size, chunk
        src = np.repeat(np.arange(self.N), lens)
        dst = rng.integers(0, self.N, size=src.size)
        first = np.cumsum(lens) - lens
        dst[first[lens > 0]] = np.arange(self.N)[lens > 0]
        p = rng.permutation(src.size)
        self.ei = np.stack([src[p], dst[p]])[None]
        self.w = rng.uniform(0.1, 1.0, size=(1, src.size)).astype(np.float32) / 8.0
        self.graphs = {}

    def graph(self, order):
        if order not in self.graphs:
            g = build_graph(self.ei, self.N, order, chunk=self.chunk)
            assert g.csr.plan.chunk == self.chunk
            self.graphs[order] = (g, g.gather_weights(T(self.w)))
        return self.graphs[order]

    def state(self, C, seed=0):
        r = np.random.default_rng(77 + C + seed)
        return [T(r.standard_normal((1, self.N, C)).astype(np.float32)) for _ in range(4)]


_graphs = {}


def graph_of(target, chunk):
    if (target, chunk) not in _graphs:
        _graphs[(target, chunk)] = Graph(target, chunk)
    return _graphs[(target, chunk)]


def scalars():
    return torch.tensor(ALPHA, device=DEV), torch.tensor(BETA, device=DEV)


def launch(g, wc, kind, x, x0, base, k0):
    """One K1 launch of stage kind 0 (store f) or 1 (one fixed-grid stage output with its base
    and two operands, the widest the prefetching epilogue takes)."""
    a, b = scalars()
    if kind == 0:
        return ops.spmm_rhs(g, wc, x, x0, a, b, add_source=True)
    out = torch.full_like(x, float("nan"))
    st = ops.Stage(outs=[(out, base, 1.0, 0.125, [(k0, 0.375), (x, -0.25)])])
    assert ops.spmm_rhs(g, wc, x, x0, a, b, add_source=True, stage=st) is None
    return out


def check_graph(gr, chunk, nblocks):
    g, _ = gr.graph("classes")
    plan = g.csr.plan
    assert plan.n_items == nblocks[0] and -(-plan.n_items // 32) == nblocks[1]
    if plan.n_heavy:
        nch = set(plan.heavy[:4 * plan.n_heavy].view(-1, 4)[:, 2].tolist())
        assert min(nch) >= 2
        return nch
    return set()


@pytest.mark.parametrize("chunk", (256, 16))
@pytest.mark.parametrize("target,blocks", list(zip(ITEMS, (1, 7, 8, 9, 94))))
def test_row_lengths_and_item_blocks(target, blocks, chunk):
    gr = graph_of(target, chunk)
    nch = check_graph(gr, chunk, (target, blocks))
    if target == 3000:  # every length occurs: all the hub sizes of this chunk
        assert set(LENGTHS) == set(gr.lens.tolist())
        assert nch == ({2, 3} if chunk == 256 else {2, 3, 4, 5, 16, 17, 44})
    x, x0, base, k0 = gr.state(128)
    for kind in (0, 1):
        outs = {}
        for order in ORDERS:
            g, wc = gr.graph(order)
            want = run(0, lambda: launch(g, wc, kind, x, x0, base, k0))
            assert bool(torch.isfinite(want).all())
            for s in STRIPES:
                got = run(s, lambda: launch(g, wc, kind, x, x0, base, k0), launches=1)
                assert torch.equal(got, want), (kind, order, s)
                again = run(s, lambda: launch(g, wc, kind, x, x0, base, k0), launches=1)  # the tickets were reset
                assert torch.equal(again, want), (kind, order, s, "second launch")
            outs[order] = want
        assert torch.equal(outs["classes"], outs["rows"])


@pytest.mark.parametrize("kind", (0, 1))
@pytest.mark.parametrize("C", (128, 96, 68))
def test_widths(C, kind):
    """C = 96: the last stripe of S = 4 holds no column; C = 68: the third holds one 16-byte slice
    (and the second stripe of S = 2 one): their other lanes load and store nothing."""
    for chunk in (256, 16):
        gr = graph_of(3000, chunk)
        x, x0, base, k0 = gr.state(C)
        for order in ORDERS:
            g, wc = gr.graph(order)
            want = run(0, lambda: launch(g, wc, kind, x, x0, base, k0))
            for s in STRIPES:
                got = run(s, lambda: launch(g, wc, kind, x, x0, base, k0), launches=1)
                assert torch.equal(got, want), (C, kind, chunk, order, s)


def test_other_geometries_stay_unstriped():
    """Widths outside 65-128 columns, rows that are not 16-byte slices and the adaptive solvers'
    wide epilogue keep their kernels whatever the setting."""
    gr = graph_of(270, 16)
    g, wc = gr.graph("classes")
    a, b = scalars()
    with stripes(4):
        before = striped_launches()
        for C in (64, 130, 132, 256):
            x, x0, _, _ = gr.state(C)
            ops.spmm_rhs(g, wc, x, x0, a, b, add_source=True)
        x, x0, _, _ = gr.state(128)
        ops.spmm_rhs(g, wc, x.bfloat16(), x0.bfloat16(), a, b, add_source=True)
        torch.cuda.synchronize()
        assert striped_launches() == before
        ops.spmm_rhs(g, wc, x, x0, a, b, add_source=True)
        assert striped_launches() == before + 1


def test_decision_by_shape():
    """Unset, the launch code stripes the fused-stage launches (stage kind 1) of large graphs' live items only;
    the forced settings take every size and both stage kinds."""
    f = _lib.fn("gnpde_k1_stripes_for")
    if "GNPDE_K1_STRIPES" not in os.environ:
        live = _lib.EPI_RHS | _lib.LIVE_ITEMS
        assert f(4500, 128, 1, live) == 0 and f(65536, 128, 1, live) == 2 and f(169343, 128, 0, live) == 0
        assert f(169343, 128, 1, _lib.EPI_RHS) == 0  # not the live items of a node layout: the old path
    for s in (0, 2, 4):
        with stripes(s):
            assert all(f(n, 128, kind, 1) == s for n in (10, 1 << 20) for kind in (0, 1))
    assert _lib.call_rc("gnpde_k1_stripes_set", 3) == _lib.EINVAL


# ------------------------------------------------------------------ the rk4 in-place solve
@pytest.mark.parametrize("n", (1, 2, 7))
def test_rk4_inplace_solve_with_layout_and_frozen_rows(n):
    """The in-place three-buffer rk4 solve over the node layout with frozen rows present
    (tests/test_gpu_frozen_rows.py's problem: C = 128, a hub row): eager and graph-replayed,
    equal bits between the two and to the unstriped solve; the caller's y0 comes back untouched.
    Every launch of a step but the solve's last (the frozen tail's, which stays unstriped) is
    striped: 4 n - 1 of them."""
    keep = ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES
    ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES = 0, 0
    try:
        if not FR._problem:
            FR._problem.append(FR.Problem())
        pr = FR._problem[0]
        assert gi.FROZEN_ROWS and gi.RK4_INPLACE
        y0 = pr.x.clone()
        times = [0.0, n * FR.DT]

        def solve(graph):
            z, taken = FR.solve(pr.func(), pr.x, times, graph)
            assert taken == 1
            return z[1]

        want = run(0, lambda: solve(False))
        for s in STRIPES:
            eager = run(s, lambda: solve(False), launches=4 * n - 1)
            replayed = run(s, lambda: solve(True))
            assert torch.equal(eager, want) and torch.equal(replayed, eager), (n, s)
            assert torch.equal(pr.x, y0)
    finally:
        ops.LAYOUT_MIN_ROWS, ops.LAYOUT_MIN_BYTES = keep


def test_default_path_stripes_the_live_item_launches():
    """Nothing forced: a graph large enough for the node layout and for the launch code's bar
    (67,000 live rows x 128 columns >= 65,536 x 128; 5,000 frozen rows) solved by the no-grad
    in-place rk4.  ops.spmm_rhs marks the launches that leave the frozen rows out with
    GNPDE_LIVE_ITEMS and the launch code stripes exactly those: 4 n - 1 = 7 of the 8 launches of two
    steps (the solve's last launch, the frozen tail's, stays unstriped).  Without the flag from
    ops.py the counter stays at 0 and this fails.  Same bits as with the stripes switched off."""
    L, F, C, n = 67000, 5000, 128, 2
    N = L + F
    assert N >= ops.LAYOUT_MIN_ROWS and N * C * 4 >= ops.LAYOUT_MIN_BYTES and F >= ops.FROZEN_MIN_ROWS
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    ids = torch.randperm(N, generator=gen, device=DEV)
    live, frozen = ids[:L], ids[L:]
    src = torch.cat([frozen, live, live.repeat(2)])
    dst = torch.cat([frozen, live, live[torch.randint(0, L, (2 * L,), generator=gen, device=DEV)]])
    w = torch.cat([torch.ones(F, device=DEV), torch.full((L,), 0.4, device=DEV), torch.full((2 * L,), 0.1, device=DEV)])
    x = torch.randn(1, N, C, generator=gen, device=DEV)
    y0 = x.clone()

    def func():
        f = gnpde.LaplacianODEFunc(C, C, dict(FR.OPT, hidden_dim=C), DEV).to(DEV)
        with torch.no_grad():
            f.alpha_train.fill_(0.3)
        f.edge_index, f.edge_weight = torch.stack([src, dst])[None], w[None].clone()
        return f

    f = func()
    lay = f.node_layout(x)
    assert lay is not None and lay.frozen is not None and lay.frozen.n_live_items >= 65536
    flags = _lib.EPI_RHS | _lib.ALPHA_SIGMOID
    unforced = "GNPDE_K1_STRIPES" not in os.environ  # (the variable forces one setting on every launch)
    if unforced:
        assert _lib.fn("gnpde_k1_stripes_for")(lay.frozen.n_live_items, C, 1, flags | _lib.LIVE_ITEMS) == 2
        assert _lib.fn("gnpde_k1_stripes_for")(lay.frozen.n_live_items, C, 1, flags) == 0
    before = striped_launches()
    z, taken = FR.solve(f, x, [0.0, n * FR.DT], False)
    assert taken == 1
    if unforced:
        assert striped_launches() - before == 4 * n - 1
    want = run(0, lambda: FR.solve(func(), x, [0.0, n * FR.DT], False)[0][1])
    assert torch.equal(z[1], want) and torch.equal(x, y0)


# ------------------------------------------------------------------ pinned rows, accuracy
@pytest.fixture(scope="module")
def world():
    return LI.World()


@pytest.mark.parametrize("C", LI.SCHED_C)
def test_pinned_rows_with_stripes_forced_on(world, C):
    """tests/golden/k1_pipeline/long_items_rows.npz (64 rows, the three-chunk hubs among them, of
    the RHS and of three rk4 steps, recorded before the loop was pipelined) with stripes forced on."""
    host = world.host
    x, x0 = host.state(C)
    gold = np.load(GOLDEN_ROWS)
    rows = host.golden_rows()
    assert np.array_equal(gold["rows"], rows)
    idx = torch.from_numpy(rows).to(DEV)
    for s in STRIPES:
        for order in ORDERS:
            g = world.graph(order)
            f = run(s, lambda: LI.rhs_plain(host, g, x, x0), launches=1)
            assert torch.equal(f[0][idx].cpu(), torch.from_numpy(gold["rhs_%d" % C])), (s, order)
        z = run(s, lambda: LI.solve(LI.make_func(host, C, x0), x))
        assert torch.equal(z[0][idx].cpu(), torch.from_numpy(gold["rk4_%d" % C])), s


def test_accuracy_vs_float64(world):
    """Three striped rk4 steps at C = 128 over 256-edge items against float64 on the host, at the
    tolerance of tests/test_gpu_long_items.py (RTOL = 1e-5: max |error| over max |reference|)."""
    host = world.host
    x, x0 = host.state(128)
    z = run(2, lambda: LI.solve(LI.make_func(host, 128, x0), x))  # S = 2: what a large graph takes by default
    err = rel(z, LI.rk4_64(host, LI.D(x), LI.D(x0), 'rk4'))
    print("striped rk4 x%d rel err %.3e" % (LI.STEPS, err))
    assert err <= RTOL
