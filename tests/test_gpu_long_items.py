"""The kernels that consume K1's plan, run at the item length of the large graphs.

ops.auto_chunk splits the rows of every graph below ops.SMALL_GRAPH_ROWS at ops.SMALL_CHUNK = 16
edges, so the small-graph tests of this suite hand agg_kernel (csrc/aggregate.hpp), the flash
kernels (csrc/flash.hip) and compact_items_kernel (csrc/weights.hip) items of at most 16 edges.
Here the graph of tests/test_gpu_k1_pipeline.py (the same length multiset: rows of 0 .. 700 edges)
is built with ``chunk=256`` — opt['gnpde_chunk'] = 256 through the module paths — as the headline
graphs are: rows of 33 .. 256 edges are ONE item each (second and later trips of the SL-edge chunk
loop, the non-LAST chunks and the next-chunk column prefetch of the headline schedule), rows of
257 and 700 edges are hub chunks of 129 / 128 and 234 / 234 / 232 edges.  Every graph is built
under both plan orders: "classes" (the default: a wavefront's row slots hold items of one
power-of-two length class) and "rows" (the builder's row order: a 256-edge row beside an empty
one).  The fixture asserts all of that on the plan it reads back.

References are float64 on the host (a sparse matrix product; the oracles of the attention
functions).  Tolerances are the project's own (tests/test_gpu_parity.py): RTOL = 1e-5 for fp32,
BF16_ROUND = 4e-3 against the reference on the same bf16-rounded inputs and BF16_TOL = 2e-2
against the reference on the unrounded ones; max |error| over max |reference|.  A serial fp32 fmaf
chain over a 256-edge row is a few 1e-7 from float64 (the kernels measure 1e-7 .. 5e-7 on this
graph), so RTOL leaves a correct kernel 20x of room and still sees one dropped edge (~1e-2).
"""
import os

import numpy as np
import pytest
import torch

import gat_oracle as G
import gnpde
import gnpde_oracle as O
from conftest import GOLDEN
from gnpde import _lib, integrator as gi, ops
from test_gpu_k1_pipeline import ALPHA, BETA, BF16_ROUND, BF16_TOL, DT, LENGTHS, OPT, RTOL, STEPS, T, _repeats, rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 256
ORDERS = ("classes", "rows")
SIG = 1.0 / (1.0 + np.exp(-ALPHA))
GOLDEN_ROWS = os.path.join(GOLDEN, "k1_pipeline", "long_items_rows.npz")
F32, BF16 = torch.float32, torch.bfloat16


def n_items_of(lens):
    """Work items of the plan (csrc/graph.hip): one per row, ceil(len / CHUNK) for a longer row."""
    return int(np.where(lens > CHUNK, -(-lens // CHUNK), 1).sum())


class Host(object):
    """The graph and its inputs on the host, from fixed seeds."""

    def __init__(self):
        rng = np.random.default_rng(20251)
        lens = np.concatenate([np.full(_repeats(L), L) for L in LENGTHS])
        lens = lens[rng.permutation(lens.size)]
        if n_items_of(lens) % 2 == 0:  # an odd item count: the last wavefront's last row slot is empty
            lens = np.concatenate([lens, [0]])
        j = np.flatnonzero(lens == 0)[0]  # row 0 has no edge: it is among the rows nobody reads
        lens[j], lens[0] = lens[0], 0
        N = lens.size
        empty = np.flatnonzero(lens == 0)
        # rows of in-degree 0 (empty rows: every other row holds its self loop), row 0 among them
        self.unread = np.sort(np.concatenate([[0], rng.choice(empty[empty > 0], size=39, replace=False)]))
        readable = np.setdiff1d(np.arange(N), self.unread)
        src = np.repeat(np.arange(N), lens)
        dst = readable[rng.integers(0, readable.size, size=src.size)]
        first = np.cumsum(lens) - lens
        dst[first[lens > 0]] = np.arange(N)[lens > 0]  # every non-empty row holds its self loop
        p = np.random.default_rng(7).permutation(src.size)
        self.ei = np.stack([src[p], dst[p]])[None]
        self.lens, self.N, self.E = lens, N, src.size
        self.w = rng.uniform(0.1, 1.0, size=(1, self.E)).astype(np.float32) / 8.0  # row sums of O(1)
        self.A = self.matrix(self.ei, self.w)
        self.At = self.A.t().coalesce()

    def matrix(self, ei, w):
        return torch.sparse_coo_tensor(torch.from_numpy(np.ascontiguousarray(ei[0])), torch.from_numpy(w[0]).double(),
                                       (self.N, self.N)).coalesce()

    def state(self, C, B=1):
        r = np.random.default_rng(1000 + C + 7919 * (B - 1))
        return (r.standard_normal((B, self.N, C)).astype(np.float32),
                r.standard_normal((B, self.N, C)).astype(np.float32))

    def golden_rows(self):
        """64 rows: every row of three hub chunks, and 61 of the others."""
        hubs = np.flatnonzero(self.lens > 2 * CHUNK)
        rest = np.setdiff1d(np.arange(self.N), hubs)
        return np.sort(np.concatenate([hubs, np.random.default_rng(64).choice(rest, size=64 - hubs.size,
                                                                             replace=False)]))


def build_graph(ei, N, order, chunk=CHUNK):
    """GraphCSR (CSR and CSC with their plans) under plan order ``order``."""
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "PLAN_ORDER", order)  # build_plan reads it at call time
        g = ops.GraphCSR(T(ei), N, chunk=chunk)
        g.csc  # noqa: B018 — the CSC's plan is built on first use: under the same order
    return g


def plan_items(grouped):
    plan = grouped.plan
    return plan.items[:4 * plan.n_items].view(-1, 4).cpu().numpy()


def check_structure(g, host, order, B):
    """What this module claims about its graph, read back from the device plan."""
    assert g.chunk == CHUNK and g.csr.plan.chunk == CHUNK
    it = plan_items(g.csr)
    ln, own = it[:, 2] - it[:, 1], it[:, 3] < 0
    lens = np.tile(host.lens, B)
    rowptr = g.csr.rowptr.cpu().numpy()
    assert np.array_equal(np.diff(rowptr), lens)
    cover = np.zeros(g.nnz, np.int64)
    for r, b0, b1, _ in it:
        assert rowptr[r] <= b0 <= b1 <= rowptr[r + 1]
        cover[b0:b1] += 1
    assert np.all(cover == 1) and ln.max() == CHUNK
    # rows of up to 256 edges own their row in ONE item: 33 .. 256 edges is what a 16-edge split never gives
    assert np.array_equal(np.sort(ln[own]), np.sort(lens[lens <= CHUNK]))
    assert set((33, 63, 64, 65, 255, 256)) <= set(ln[own].tolist())
    # the 257- and 700-edge rows are hub chunks (two of 129 / 128, three of 234 / 234 / 232 edges)
    hubs = np.flatnonzero(lens > CHUNK)
    assert set(lens[hubs].tolist()) == {257, 700} and g.csr.plan.n_heavy == hubs.size
    assert np.array_equal(np.unique(it[~own, 0]), hubs)
    assert set(ln[~own].tolist()) == {128, 129, 232, 234}
    if B == 1:
        assert g.csr.plan.n_items % 2 == 1  # two row slots per wavefront: the last one of the launch is empty
    if order == "rows":
        assert np.all(np.diff(it[:, 0]) >= 0)  # the builder's order: rows as the permutation left them
        n2 = it.shape[0] // 2 * 2
        lo, hi = np.minimum(ln[0:n2:2], ln[1:n2:2]), np.maximum(ln[0:n2:2], ln[1:n2:2])
        # the two row slots of a wavefront (GL = 32, RPW = 2): a row that ends chunks before its partner's
        assert ((hi >= 65) & (lo >= 1) & (lo <= 4)).any() and ((hi >= 65) & (lo == 0)).any()
    else:
        cls = np.floor(np.log2(np.maximum(ln, 1)))
        assert np.all(np.diff(cls) <= 0)  # length classes, longest first


class World(object):
    """The host graph and its device graphs, each built once."""

    def __init__(self):
        self.host = Host()
        self.graphs = {}
        for order in ORDERS:  # the structural claims hold before any kernel test runs
            self.graph(order)

    def graph(self, order, B=1, flip=False):
        key = (order, B, flip)
        if key not in self.graphs:
            ei = self.host.ei[:, ::-1] if flip else self.host.ei
            g = build_graph(np.repeat(ei, B, axis=0), self.host.N, order)
            if not flip:
                check_structure(g, self.host, order, B)
            else:  # the flipped graph: the long items are the CSC's (the transposed aggregation)
                ln = np.diff(plan_items(g.csc)[:, 1:3], axis=1)
                assert g.chunk == CHUNK and ln.max() == CHUNK and g.csc.plan.n_heavy == 15
            self.graphs[key] = g
        return self.graphs[key]


@pytest.fixture(scope="module")
def world():
    return World()


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def agg64(host, x, transpose=False):
    """A x (or A^T x) in fp64: x [B,N,C], the same graph in every batch element."""
    A = host.At if transpose else host.A
    return torch.stack([torch.sparse.mm(A, x[b]) for b in range(x.shape[0])])


def rhs64(host, x, x0, beta=BETA):
    """sigma(alpha) (A x - x) + beta x0 in fp64."""
    f = SIG * (agg64(host, x) - x)
    return f + beta * x0 if x0 is not None else f


def scalars():
    return torch.tensor(ALPHA, device=DEV), torch.tensor(BETA, device=DEV)


def twice(fn):
    """Two runs of fn: equal bits."""
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    return a


def check(name, got, want, dtype, want_rounded=None):
    """The project's bars: fp32 against fp64 at RTOL; bf16 at BF16_ROUND against the reference on the
    bf16-rounded inputs and BF16_TOL against the reference on the unrounded ones."""
    if dtype == F32:
        err = rel(got, want)
        print("%s fp32 rel err %.3e" % (name, err))
        assert err <= RTOL, (name, err)
    else:
        err, err_r = rel(got, want), rel(got, want_rounded)
        print("%s bf16 rel err %.3e (rounded inputs %.3e)" % (name, err, err_r))
        assert err_r <= BF16_ROUND and err <= BF16_TOL, (name, err, err_r)


# ------------------------------------------------------------------ 1. plain-weight K1 against float64
K1_CASES = [(C, F32) for C in (7, 16, 32, 64, 80, 128, 162, 256, 512, 1024)] + \
           [(C, BF16) for C in (64, 128, 162, 256)]


def _ids(cases):
    return ["%d-%s" % (C, "bf16" if dt == BF16 else "fp32") for C, dt in cases]


@pytest.mark.parametrize("C,dtype", K1_CASES, ids=_ids(K1_CASES))
def test_plain_k1_vs_fp64(world, C, dtype):
    """ops.spmm_rhs over 256-edge items at every lane geometry of launch_agg_vec below its 96 MB
    branch: the RHS with its source term, the plain aggregation, and the transposed (CSC)
    aggregation — of this graph (short CSC items) and of the flipped graph (the CSC holds the long
    items: what the adjoint runs).  Two runs equal bits; the two plan orders equal bits (ops.py:
    "Results do not depend on it"); the rows without edges on their own."""
    host = world.host
    x, x0 = host.state(C)
    xd, x0d = T(x).to(dtype), T(x0).to(dtype)
    a, b = scalars()
    x64, x064 = D(x), D(x0)
    xr, x0r = xd.double().cpu(), x0d.double().cpu()  # the bf16-rounded inputs (fp32: the same values)
    want = {"rhs": (rhs64(host, x64, x064), rhs64(host, xr, x0r)),
            "agg": (agg64(host, x64), agg64(host, xr)),
            "aggT": (agg64(host, x64, True), agg64(host, xr, True))}
    want["aggT_long"] = want["agg"]  # (A^T)^T x over the flipped graph's CSC
    empty = np.flatnonzero(host.lens == 0)
    got = {}
    for order in ORDERS:
        g, gf = world.graph(order), world.graph(order, flip=True)
        wc, wt, wft = g.gather_weights(T(host.w)), g.gather_weights(T(host.w), transpose=True), \
            gf.gather_weights(T(host.w), transpose=True)
        got[order] = {
            "rhs": twice(lambda: ops.spmm_rhs(g, wc, xd, x0d, a, b, rhs=True, add_source=True)),
            "agg": twice(lambda: ops.spmm_rhs(g, wc, xd, rhs=False)),
            "aggT": twice(lambda: ops.spmm_rhs(g, wt, xd, rhs=False, transpose=True)),
            "aggT_long": twice(lambda: ops.spmm_rhs(gf, wft, xd, rhs=False, transpose=True)),
        }
    for kind, (w64, w64r) in want.items():
        f = got["classes"][kind]
        assert f.dtype == dtype
        assert torch.equal(f, got["rows"][kind]), "%s: the plan order changed bits" % kind
        check("C=%d %s" % (C, kind), f, w64, dtype, w64r)
        # the rows that aggregate nothing, whatever their wavefront's other row slot did
        none = host.unread if kind == "aggT" else empty
        idx = torch.from_numpy(none).to(DEV)
        if kind == "rhs":
            check("C=%d rhs, empty rows" % C, f[0][idx], w64r[0][none], F32 if dtype == F32 else BF16, w64r[0][none])
        else:
            assert not bool(f[0][idx].any()), "%s: a row without edges is not zero" % kind


# ------------------------------------------------------------------ 2. the pipelined loop, bitwise
SCHED_C = (68, 80, 100, 128)  # fp32 rows of 65-128 columns: agg_kernel's SCHED path; 68, 80, 100 leave idle lanes


def widen(a, C, seed):
    """a [1,N,C] in the first C of 256 columns, other values beside it."""
    out = np.random.default_rng(seed).standard_normal(a.shape[:2] + (256,)).astype(np.float32)
    out[..., :C] = a
    return out


def make_func(host, C, x0, dtype=F32, alloc=False, flip=False, add_source=True):
    func = gnpde.LaplacianODEFunc(C, C, dict(OPT, hidden_dim=C, gnpde_chunk=CHUNK, add_source=add_source), DEV).to(DEV)
    with torch.no_grad():
        func.alpha_train.fill_(ALPHA)
        func.beta_train.fill_(BETA)
    func.edge_index, func.edge_weight = T(host.ei[:, ::-1] if flip else host.ei), T(host.w)
    func.x0 = T(x0).to(dtype)
    if alloc:  # a module that places its own state: the integrator keeps the ping-pong scheme for it
        func.alloc_state = lambda like: torch.empty_like(like, memory_format=torch.contiguous_format)
    return func


def solve(func, x, method='rk4', graph=False, dtype=F32):
    with torch.no_grad():
        z = gnpde.odeint(func, T(x).to(dtype), torch.tensor([0.0, STEPS * DT], device=DEV), method=method,
                         options={'step_size': DT, 'gnpde_graph': graph})
    torch.cuda.synchronize()
    assert func.graph_for(z[1]).chunk == CHUNK  # the module path honours opt['gnpde_chunk']
    return z[1]


def rhs_plain(host, g, x, x0):
    a, b = scalars()
    return ops.spmm_rhs(g, g.gather_weights(T(host.w)), T(x), T(x0), a, b, rhs=True, add_source=True)


def rk4_variants(host, C, x, x0):
    """Three fused rk4 steps: the in-place three-buffer solve, and the solve of a module with alloc_state."""
    f_in, f_pp = make_func(host, C, x0), make_func(host, C, x0, alloc=True)
    probe = T(x)
    assert gi._steps_inplace('rk4', f_in, probe) and not gi._steps_inplace('rk4', f_pp, probe)
    return solve(f_in, x), solve(f_pp, x)


@pytest.mark.parametrize("C", SCHED_C)
def test_pipelined_loop_equals_the_one_batch_loop_bitwise(world, C):
    """The SCHED loop (C columns, two 32-lane row slots, pipelined half batches) against the generic
    one-batch loop (the same C columns inside 256: GL = 64, one row per wavefront).  Both sum a
    row's edges in CSR order with one fmaf per edge and column, so every row that is ONE item, or
    a hub of two chunks (0 + c0 + c1 either way), has equal bits, under either plan order.

    Not the hubs of three chunks, and that is no defect: hub_sum (csrc/aggregate.hpp) gives the
    chunk partials of a hub to 64 / GL lane groups — chunks g, g + G, ... each, joined by an xor
    tree — so two 32-lane groups form (c0 + c2) + c1 where the one 64-lane group of C = 256 forms
    (c0 + c1) + c2.  The three 700-edge rows therefore differ in the last bit between the two
    widths, and through them every row of an rk4 solve after a step.  Those are pinned instead:
    tests/golden/k1_pipeline/long_items_rows.npz holds, per width, 64 rows (the three hubs among
    them) of the RHS and of three rk4 steps as the library of commit cf70049 computed them at
    chunk = 256 — before the loop was pipelined and before the in-place rk4 solve (recorded with
    that library and its package: rhs_plain / solve of this module, out-of-place steps)."""
    host = world.host
    x, x0 = host.state(C)
    xw, x0w = widen(x, C, 1), widen(x0, C, 2)
    three = torch.from_numpy(host.lens > 2 * CHUNK).to(DEV)
    assert int(three.sum()) == 3
    f = {}
    for order in ORDERS:
        g = world.graph(order)
        f[order] = twice(lambda: rhs_plain(host, g, x, x0))
        fw = rhs_plain(host, g, xw, x0w)[..., :C]
        same = f[order] == fw
        print("C=%d %s: rows differing from the C=256 loop: %s" % (
            C, order, torch.nonzero(~same.all(dim=2)[0]).flatten().tolist()))
        assert bool(same[0][~three].all())
    assert torch.equal(f["classes"], f["rows"])
    gold = np.load(GOLDEN_ROWS)
    rows = host.golden_rows()
    assert np.array_equal(gold["rows"], rows)
    idx = torch.from_numpy(rows).to(DEV)
    assert torch.equal(f["classes"][0][idx].cpu(), torch.from_numpy(gold["rhs_%d" % C]))
    # three fused rk4 steps: the in-place solve and the ping-pong solve, equal bits, and the pinned rows
    z_in, z_pp = rk4_variants(host, C, x, x0)
    assert torch.equal(z_in, z_pp)
    want = torch.from_numpy(gold["rk4_%d" % C])
    assert want.shape == (64, C) and want.dtype == torch.float32
    assert torch.equal(z_in[0][idx].cpu(), want)
    err = rel(z_in, rk4_64(host, D(x), D(x0), 'rk4'))
    print("C=%d rk4 x%d rel err %.3e" % (C, STEPS, err))
    assert err <= RTOL


# ------------------------------------------------------------------ 3. rows that no edge reads
@pytest.mark.parametrize("C,dtype", [(80, F32), (128, F32), (64, F32), (162, F32), (128, BF16), (162, BF16)],
                         ids=_ids([(80, F32), (128, F32), (64, F32), (162, F32), (128, BF16), (162, BF16)]))
def test_unread_rows_are_never_summed(world, C, dtype):
    """Rows of in-degree 0, row 0 among them (a lane without an edge re-reads the row of lane 0's
    column id, and a slot without edges holds column id 0): NaN or +Inf in them changes no bit of
    A x in any row — a load that is not summed is skipped by a select, not multiplied by a zero weight."""
    host = world.host
    assert host.unread[0] == 0 and not np.isin(host.ei[0, 1], host.unread).any()
    x, _ = host.state(C)
    xd = T(x).to(dtype)
    idx = torch.from_numpy(host.unread).to(DEV)
    for order in ORDERS:
        g = world.graph(order)
        wc = g.gather_weights(T(host.w))
        clean = ops.spmm_rhs(g, wc, xd, rhs=False)
        assert bool(torch.isfinite(clean).all())
        for poison in (float("nan"), float("inf")):
            xp = xd.clone()
            xp[0, idx] = poison
            got = ops.spmm_rhs(g, wc, xp, rhs=False)
            torch.cuda.synchronize()
            assert torch.equal(got, clean), "%s order, %s in the unread rows" % (order, poison)


# ------------------------------------------------------------------ 4. stage epilogues on long items
def rk4_64(host, x, x0, method, steps=STEPS, dt=DT, rhs=None):
    """``steps`` steps of euler / midpoint / the 3/8-rule rk4 (torchdiffeq) in fp64."""
    f = rhs if rhs is not None else (lambda v: rhs64(host, v, x0))
    y = x
    for _ in range(steps):
        if method == 'euler':
            y = y + dt * f(y)
        elif method == 'midpoint':
            y = y + dt * f(y + 0.5 * dt * f(y))
        else:
            k1 = f(y)
            k2 = f(y + dt * k1 / 3.0)
            k3 = f(y + dt * (k2 - k1 / 3.0))
            k4 = f(y + dt * (k1 - k2 + k3))
            y = y + (k1 + 3.0 * (k2 + k3) + k4) * dt * 0.125
    return y


STAGE_CASES = [(128, F32), (64, F32), (162, F32), (16, F32), (162, BF16)]


@pytest.mark.parametrize("method", ["euler", "midpoint", "rk4"])
@pytest.mark.parametrize("C,dtype", STAGE_CASES, ids=_ids(STAGE_CASES))
def test_fixed_grid_stages_vs_fp64(world, C, dtype, method):
    """LaplacianODEFunc with gnpde_chunk = 256: the fused stage epilogues of the fixed-grid steps
    (the headline, a narrow, a padded, a several-rows-per-wavefront and the bf16 three-row geometry)
    after long items and hub combines; eager and graph-replayed steps equal bits."""
    host = world.host
    x, x0 = host.state(C)
    z = solve(make_func(host, C, x0, dtype), x, method, graph=False, dtype=dtype)
    zg = solve(make_func(host, C, x0, dtype), x, method, graph=True, dtype=dtype)
    assert torch.equal(z, zg)
    err = rel(z.float(), rk4_64(host, D(x), D(x0), method))
    print("C=%d %s %s x%d rel err %.3e" % (C, dtype, method, STEPS, err))
    assert err <= (RTOL if dtype == F32 else BF16_TOL)


@pytest.mark.parametrize("C", [128, 64])
def test_dopri5_wide_epilogue_vs_oracle_steps(world, C):
    """dopri5 as the integrator runs it by default — the wide stage epilogue with the error rows,
    the Krylov step, the dense output folded into the step's last launch — on 256-edge items:
    the oracle's accepted / rejected step sequence and its values (the bounds of
    test_gpu_adaptive.test_fused_adaptive_vs_oracle_steps), output times inside steps."""
    assert gi.KRYLOV_STEP and gi.DENSE_FOLD and gi.AFFINE_STAGE
    host = world.host
    x, x0 = host.state(C)
    func = make_func(host, C, x0)
    ts = [0.0, 0.05, 0.5, 1.0, 2.0, 4.0]  # that test's tolerances; a longer span, so that several steps run
    with torch.no_grad():
        got = gi.odeint(func, T(x), torch.tensor(ts, dtype=torch.float64, device=DEV), rtol=1e-3, atol=1e-4,
                        method='dopri5')
    n_got = gi.odeint.last_n_steps
    assert func.graph_for(T(x)).chunk == CHUNK
    x064 = D(x0)
    f = lambda t, y: rhs64(host, torch.from_numpy(y), x064).numpy()  # noqa: E731
    want, n_want = O.odeint_adaptive(f, x, ts, 'dopri5', 1e-3, 1e-4)
    err = rel(got, torch.from_numpy(want))
    print("C=%d dopri5: %d steps (oracle %d), rel err %.3e" % (C, n_got, n_want, err))
    assert n_got == n_want
    assert err <= RTOL


@pytest.mark.parametrize("add_source", [False, True])
@pytest.mark.parametrize("C", [128, 64])
def test_fused_rk4_backward_vs_fp64_autograd(world, C, add_source):
    """The fused fixed-grid backward of rk4 (integrator._LaplacianFixedGridFn: the transposed
    aggregation with the one-output adjoint stages, stage kind 3) over the FLIPPED graph, whose CSC
    holds the 256-edge items and the hubs, against float64 autograd through the same steps on the
    host: the solution at RTOL, the gradients to the state, alpha_train and beta_train at the
    project's gradient bar of 1e-4 (measured: 1e-7 .. 3e-7)."""
    host = world.host
    x, x0 = host.state(C)
    r = np.random.default_rng(77 + C)
    g1, g2 = r.standard_normal((2, 1, host.N, C)).astype(np.float32)
    func = make_func(host, C, x0, flip=True, add_source=add_source)
    assert gi.FUSED_BACKWARD and func.fixed_grid_backward_ok()
    xi = T(x).requires_grad_(True)
    t = torch.tensor([0.0, DT, 3 * DT], device=DEV)
    y = gnpde.odeint(func, xi, t, method='rk4', options={'step_size': DT})
    assert "_LaplacianFixedGridFn" in type(y.grad_fn).__name__  # the fused discrete adjoint, not per-RHS autograd
    ((y[1] * T(g1)).sum() + (y[2] * T(g2)).sum()).backward()
    torch.cuda.synchronize()
    g = func.graph_for(xi)
    assert g.chunk == CHUNK and g.csc.plan.n_heavy == 15
    # float64 autograd on the host: the flipped graph aggregates with A^T
    xr = D(x).requires_grad_(True)
    al = torch.tensor(ALPHA, dtype=torch.float64, requires_grad=True)
    be = torch.tensor(BETA, dtype=torch.float64, requires_grad=True)
    x064 = D(x0)

    def rhs(v):
        out = torch.sigmoid(al) * (agg64(host, v, transpose=True) - v)
        return out + be * x064 if add_source else out

    y1 = rk4_64(host, xr, None, 'rk4', steps=1, rhs=rhs)
    y3 = rk4_64(host, y1, None, 'rk4', steps=2, rhs=rhs)
    ((y1 * D(g1)).sum() + (y3 * D(g2)).sum()).backward()
    ey = max(rel(y[1], y1.detach()), rel(y[2], y3.detach()))
    ex = rel(xi.grad, xr.grad)
    ea = abs(float(func.alpha_train.grad) - float(al.grad)) / max(1.0, abs(float(al.grad)))
    print("C=%d add_source=%s: y %.3e, grad x %.3e, grad alpha %.3e" % (C, add_source, ey, ex, ea))
    assert ey <= RTOL and ex <= 1e-4 and ea <= 1e-4
    if add_source:
        eb = abs(float(func.beta_train.grad) - float(be.grad)) / max(1.0, abs(float(be.grad)))
        print("grad beta %.3e" % eb)
        assert eb <= 1e-4


# ------------------------------------------------------------------ 5. weight policies inside K1
def qk(C, att, seed, scale):
    r = np.random.default_rng(seed)
    Wq, Wk = [(r.standard_normal((att, C)) * scale).astype(np.float32) for _ in range(2)]
    bq, bk = [(r.standard_normal(att) * scale).astype(np.float32) for _ in range(2)]
    return Wq, bq, Wk, bk


def fused_and_separate(world, run, want, name, bits=True):
    """``run(g, fuse)`` under both plan orders: the fused policy against the oracle at RTOL, bit-equal to
    itself under the other order and (``bits``) to the separate weights pass + the plain K1."""
    outs = []
    for order in ORDERS:
        g = world.graph(order)
        fused = twice(lambda: run(g, True))
        separate = run(g, False)
        if bits:
            assert torch.equal(fused, separate), "%s (%s): fused and separate weights differ" % (name, order)
        else:
            assert rel(fused, separate.double().cpu()) <= RTOL
        outs.append(fused)
    assert torch.equal(outs[0], outs[1])
    err = rel(outs[0], torch.from_numpy(want))
    print("%s rel err %.3e" % (name, err))
    assert err <= RTOL


@pytest.mark.parametrize("C", [128, 80, 64])
@pytest.mark.parametrize("heads", [2, 4])
def test_reference_scores_policy_in_k1(world, heads, C, monkeypatch):
    """RefDstSoftmaxWeights (norm_idx 1; two heads: the packed statistics records) formed in K1's
    gather loop over 256-edge items.  "Same bits as the separate weights pass" (ops.attn_rhs) is a
    promise about the weights; the sums are the plain K1's wherever the two take one lane geometry:
    rows of more than 64 columns.  Up to 64 columns the plain weights take the narrow-row
    geometries (two 32-lane row slots of two edge groups at C = 64) and this policy, by design, the
    one-row 16-lane geometry (four edge groups; takes_narrow_rows in csrc/aggregate.hpp), so a row's
    edges are dealt to other partial sums: C = 64 is held to RTOL, against the oracle and between
    the two paths."""
    host = world.host
    x, _ = host.state(C)
    Wq, bq, Wk, bk = qk(C, 8 * heads, 5 + heads, 0.02)
    want = O.transformer_rhs(host.ei, x, None, Wq, bq, Wk, bk, heads, 1, ALPHA, 0.0)
    seen = []
    orig = ops.spmm_rhs
    monkeypatch.setattr(ops, "spmm_rhs", lambda g, w, *a, **k: (seen.append(type(w)), orig(g, w, *a, **k))[1])

    def run(g, fuse):
        ns = ops.node_scores(g, T(x), T(Wq), T(bq), T(Wk), T(bk), heads)
        return ops.attn_rhs(g, ns, None, None, 1, T(x), alpha=scalars()[0], fuse=fuse)

    fused_and_separate(world, run, want, "reference scores h=%d C=%d" % (heads, C), bits=C > 64)
    assert ops.RefDstWeights in seen and torch.Tensor in seen  # both paths ran


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("heads", [2, 8])
@pytest.mark.parametrize("norm_idx", [0, 1])
def test_gat_policy_in_k1(world, norm_idx, heads, C, monkeypatch):
    """GatSoftmaxWeights of either grouping formed in K1's gather loop over 256-edge items."""
    host = world.host
    x, _ = host.state(C)
    r = np.random.default_rng(31 + heads + norm_idx)
    att = 8 * heads
    W = (r.standard_normal((C, att)) * 0.3 / np.sqrt(C / 12.0)).astype(np.float32)
    av = (r.standard_normal(2 * att // heads) * 0.5).astype(np.float32)
    want = G.gat_rhs(host.ei, x, None, W, av, heads, norm_idx, 0.2, ALPHA, 0.0)
    seen = []
    orig = ops.spmm_rhs
    monkeypatch.setattr(ops, "spmm_rhs", lambda g, w, *a, **k: (seen.append(type(w)), orig(g, w, *a, **k))[1])

    def run(g, fuse):
        ns = ops.gat_scores(g, T(x), T(W), T(av), heads, 0.2)
        return ops.attn_rhs(g, ns, None, None, norm_idx, T(x), alpha=scalars()[0], fuse=fuse)

    fused_and_separate(world, run, want, "GAT norm_idx=%d h=%d C=%d" % (norm_idx, heads, C))
    assert ops.GatWeights in seen and torch.Tensor in seen


@pytest.mark.parametrize("C", [128, 64])
@pytest.mark.parametrize("heads", [2, 4])
def test_squareplus_policy_in_k1(world, heads, C, monkeypatch):
    """RefDstSquareplusWeights (reference scores, norm_idx 1) formed in K1's gather loop over
    256-edge items, against the squareplus composition of the oracle."""
    host = world.host
    x, _ = host.state(C)
    Wq, bq, Wk, bk = qk(C, 8 * heads, 9 + heads, 0.02)
    want = O.transformer_rhs(host.ei, x, None, Wq, bq, Wk, bk, heads, 1, ALPHA, 0.0, square_plus=True)
    seen = []
    orig = ops.spmm_rhs
    monkeypatch.setattr(ops, "spmm_rhs", lambda g, w, *a, **k: (seen.append(type(w)), orig(g, w, *a, **k))[1])

    def run(g, fuse):
        ns = ops.node_scores(g, T(x), T(Wq), T(bq), T(Wk), T(bk), heads)
        return ops.squareplus_rhs(g, ns, 1, T(x), alpha=scalars()[0], fuse=fuse)

    fused_and_separate(world, run, want, "squareplus h=%d C=%d" % (heads, C))
    assert ops.RefDstSquareplusWeights in seen and torch.Tensor in seen


# ------------------------------------------------------------------ 6. the flash kernels
FLASH_SHAPES = [(128, 2, 32), (64, 2, 16), (160, 4, 32), (36, 2, 8)]
BF16_OUT = 2.0 ** -7  # a bf16 result against fp64 of the same bf16 inputs: the bound of test_gpu_flash.py (bf16
# keeps 8 significant bits; the element that sets the maximum error need not be the largest one)


def flash(g, x, x0, proj, h, norm_idx, fuse_direct=True):
    Wq, bq, Wk, bk = proj
    ns = ops.node_scores(g, x, T(Wq), T(bq), T(Wk), T(bk), h, 'scaled_dot', 'per_edge')
    a, b = scalars()
    if not fuse_direct:
        return ops.attn_rhs(g, ns, None, None, norm_idx, x, x0, a, b, add_source=True, fuse=False)
    mr = ops.softmax_stats(g, ns, 1, packed=True)[2] if norm_idx == 1 else None
    f = ops.attn_dot_rhs(g, ns, x, x0, a, b, add_source=True, mr=mr)
    assert f is not NotImplemented
    return f


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("norm_idx", [0, 1])
@pytest.mark.parametrize("C,h,att", FLASH_SHAPES)
def test_flash_rhs_on_long_items(world, C, h, att, norm_idx, B):
    """ops.attn_dot_rhs (dot_agg / dot_agg1 / dot_dst_agg kernels): the online-softmax
    running maximum carried over 256 edges of a row and across hub chunks."""
    assert _lib.fn("gnpde_attn_dot_supported")(h, att // h, C)
    host = world.host
    x, x0 = host.state(C, B)
    proj = qk(C, att, C + h, 0.1)
    ei = np.repeat(host.ei, B, axis=0)
    want = torch.from_numpy(O.transformer_rhs(ei, x, x0, *proj, h, norm_idx, ALPHA, BETA, score_mode='per_edge',
                                              add_source=True))
    outs = []
    for order in ORDERS:
        g = world.graph(order, B)
        f = twice(lambda: flash(g, T(x), T(x0), proj, h, norm_idx))
        fu = flash(g, T(x), T(x0), proj, h, norm_idx, fuse_direct=False)
        e, eu, d = rel(f, want), rel(fu, want), rel(f, fu.double().cpu())
        print("flash C=%d h=%d norm_idx=%d B=%d %s: fused %.3e, unfused %.3e, between %.3e" % (C, h, norm_idx, B, order,
                                                                                         e, eu, d))
        assert e <= RTOL and eu <= RTOL and d <= RTOL
        outs.append(f)
    assert torch.equal(outs[0], outs[1])
    if norm_idx == 0:  # a bf16 state: source-grouped softmax only
        xb, x0b = T(x).to(BF16), T(x0).to(BF16)
        wb = torch.from_numpy(O.transformer_rhs(ei, xb.float().cpu().numpy(), x0b.float().cpu().numpy(), *proj, h, 0,
                                                ALPHA, BETA, score_mode='per_edge', add_source=True))
        for order in ORDERS:
            g = world.graph(order, B)
            fb = twice(lambda: flash(g, xb, x0b, proj, h, 0))
            fub = flash(g, xb, x0b, proj, h, 0, fuse_direct=False)
            assert fb.dtype == BF16 and fub.dtype == BF16
            e, d = rel(fb.float(), wb), rel(fb.float(), fub.double().cpu())
            print("flash bf16 C=%d h=%d B=%d %s: fused %.3e, between %.3e" % (C, h, B, order, e, d))
            assert e <= BF16_OUT and d <= BF16_OUT


@pytest.mark.parametrize("norm_idx", [0, 1])
def test_flash_rising_scores_along_long_rows(world, norm_idx):
    """The adversarial order for an online softmax: scores of hundreds (wscale 1.0) that RISE along
    every row's CSR order (each row's destinations sorted by the score of head 0), so the running
    maximum moves in every batch of a 256-edge item and across hub chunks, and a row's first edges
    are rescaled many times.  Against float64 at RTOL."""
    host = world.host
    C, h, att = 128, 2, 32
    x, x0 = host.state(C)
    proj = qk(C, att, 99, 1.0)
    s = O.attention_scores(x, host.ei, *proj, h, score_mode='per_edge')[0, :, 0]
    src, dst = host.ei[0]
    o = np.lexsort((s, src))  # rows in order, ascending score of head 0 inside a row
    ei = np.stack([src[o], dst[o]])[None]
    assert np.abs(s).max() > 300.0
    g = build_graph(ei, host.N, "classes")
    assert g.chunk == CHUNK and np.array_equal(g.csr.col.cpu().numpy(), dst[o])  # the CSR keeps that order
    want = torch.from_numpy(O.transformer_rhs(ei, x, x0, *proj, h, norm_idx, ALPHA, BETA, score_mode='per_edge',
                                              add_source=True))
    d32 = rel(torch.from_numpy(O.transformer_rhs_f32(ei, x, *proj, h, norm_idx, ALPHA)),
              torch.from_numpy(O.transformer_rhs(ei, x, None, *proj, h, norm_idx, ALPHA, 0.0, score_mode='per_edge')))
    f = twice(lambda: flash(g, T(x), T(x0), proj, h, norm_idx))
    fu = flash(g, T(x), T(x0), proj, h, norm_idx, fuse_direct=False)
    e, eu = rel(f, want), rel(fu, want)
    print("rising scores norm_idx=%d, max|s| %.0f: fused %.3e, unfused %.3e, the reference's own fp32 run %.3e"
          % (norm_idx, np.abs(s).max(), e, eu, d32))
    assert e <= RTOL and eu <= RTOL


# ------------------------------------------------------------------ 7. compacted items
@pytest.mark.parametrize("pct", [0.19, 0.43])
def test_compacted_long_items(world, pct):
    """ops.compact_weights over 256-edge items: ``pct`` of the weights zeroed at random, and whole
    32-edge chunks (a row slot's chunk in the headline geometry) of some long rows.  The compacted
    items hold exactly the retained edges of each item, in order; K1 over them equals K1 over the
    masked full weights bit for bit at C = 128 (one edge group per row slot: one sequence per row,
    a dropped edge added an exact 0) and within 1e-6 at C = 32 (several edge groups per slot: the
    rule in test_gpu_parity.test_hard_attention_compacted_graph_bit_equal)."""
    host = world.host
    a, b = scalars()
    for order in ORDERS:
        g = world.graph(order)
        rowptr = g.csr.rowptr.cpu().numpy()
        r = np.random.default_rng(int(pct * 100))
        keep = r.random(g.nnz) >= pct
        for k, row in enumerate(np.flatnonzero(host.lens >= 64)):
            n32 = host.lens[row] // 32
            for c in {k % n32, (3 * k + 1) % n32}:  # first, middle and last chunks all occur
                keep[rowptr[row] + 32 * c:rowptr[row] + 32 * c + 32] = False
        full = (g.gather_weights(T(host.w)) * torch.from_numpy(keep).to(DEV)).contiguous()
        cw = ops.compact_weights(g.csr, full, False)
        it0, it1 = plan_items(g.csr), cw.items[:4 * g.csr.plan.n_items].view(-1, 4).cpu().numpy()
        col, fw, ccol, cwc = g.csr.col.cpu().numpy(), full.cpu().numpy(), cw.col.cpu().numpy(), cw.w.cpu().numpy()
        assert (it0[:, [0, 1, 3]] == it1[:, [0, 1, 3]]).all()
        emptied = 0
        for (_, b0, e0, _), (_, b1, e1, _) in zip(it0, it1):
            kp = fw[b0:e0] != 0
            assert e1 - b1 == int(kp.sum())
            assert (ccol[b1:e1] == col[b0:e0][kp]).all() and (cwc[b1:e1] == fw[b0:e0][kp]).all()
            emptied += int(e0 - b0 >= 64 and e1 - b1 <= e0 - b0 - 32)
        assert emptied >= 100  # long items lost whole chunks
        for C in (128, 32):
            x, x0 = host.state(C)
            fc = twice(lambda: ops.spmm_rhs(g, cw, T(x), T(x0), a, b, add_source=True))
            fm = ops.spmm_rhs(g, full, T(x), T(x0), a, b, add_source=True)
            if C == 128:
                assert torch.equal(fc, fm), order
            else:
                d = rel(fc, fm.double().cpu())
                print("compacted C=32 pct=%.2f %s: %.3e from the masked full graph" % (pct, order, d))
                assert d <= 1e-6
            Am = host.matrix(host.ei, masked_coo(host, g, keep))
            want = SIG * (torch.sparse.mm(Am, D(x)[0]) - D(x)[0]) + BETA * D(x0)[0]
            assert rel(fc[0], want) <= RTOL


def masked_coo(host, g, keep):
    """The COO weights with the CSR-order mask ``keep`` applied."""
    w = host.w.copy()
    perm = g.csr.perm.cpu().numpy()
    w[0, perm[~keep]] = 0.0
    return w
