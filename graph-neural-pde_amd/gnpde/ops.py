"""Tensor-level wrappers over the C ABI (include/gnpde.h).

Everything here runs on the GPU through libgnpde.so; there is no CPU path.
Tensors must live on a ROCm device; every launch goes onto torch's current
stream, so the calls compose with torch ops and are hipGraph-capturable (the
graph build / plan functions are once-per-graph and synchronous).

Layout: node features [B,N,C] fp32 row-major, viewed as
[R=B*N, C]; graphs are block-diagonal over the batch as an int32 CSR
(rowptr[R+1], col[nnz] global node ids, perm[nnz] CSR pos -> COO edge id).
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._cache import _tensor_key

# hub-splitting threshold (edges per K1 work item).  With the longest-first item
# order below, full-bench A/B on G-arxiv: 128 -> 8,048-8,200, 256 -> 8,485-8,496,
# 384 -> 8,434-8,450 RHS/s (in row order 128 was best: 121 against 128 us per RHS)
DEFAULT_CHUNK = int(os.environ.get("GNPDE_CHUNK", 256))
# Small graphs (fewer rows than SMALL_GRAPH_ROWS, configs[1]'s Cora-sized graph) are
# latency-bound: the launch is one round of short work items and its time is the
# longest item's chain of dependent loads, so their rows split at SMALL_CHUNK edges
# (the Cora-sized transformer's K1: 38 us at 256-edge items, 16 at 32; its dopri5
# step 0.358 ms at 32, 0.348 at 16, 0.428 at 64: gpurun_out/r05m, r05p).
# GNPDE_CHUNK set in the environment applies to every graph.
SMALL_GRAPH_ROWS = 50000
SMALL_CHUNK = int(os.environ.get("GNPDE_SMALL_CHUNK", 16))


SEG_LONG_SPLIT = os.environ.get("GNPDE_SEG_LONG_SPLIT", "1") != "0"  # small graphs: one-pass long items


def auto_chunk(R, chunk=None):
    """The hub-row split of a graph of R rows: ``chunk`` if given, else the
    environment's GNPDE_CHUNK, else SMALL_CHUNK below SMALL_GRAPH_ROWS rows and
    DEFAULT_CHUNK above."""
    if chunk is not None:
        return int(chunk)
    if "GNPDE_CHUNK" in os.environ:
        return DEFAULT_CHUNK
    return SMALL_CHUNK if R < SMALL_GRAPH_ROWS else DEFAULT_CHUNK
STATS_CHUNK = 64     # items of the softmax-statistics kernel (8 lanes per item)
# K1 work items ordered by power-of-two length class, longest first, row order inside a class
# ("classes", the default since round 2: tools/stripe_sweep2.sh, profiles/r02c_plan_order_sweep.jsonl —
# rk4 step G-arxiv C = 128 / 16: 0.429 / 0.121 ms against 0.435 / 0.128 with a plain longest-first
# sort ("lpt", round 1: 8,130-8,205 against 7,917-7,932 RHS/s in row order), G-rmat at 32 columns
# 2.59 against 2.63 ms).
# GNPDE_PLAN_ORDER=rows keeps the builder's row order; =classes sorts by power-of-two length class
# only (row order inside a class); =hubs puts the hub chunks first.  Results do not depend on it.
PLAN_ORDER = os.environ.get("GNPDE_PLAN_ORDER", "classes")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_gpu(t, name, dtype=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("gnpde: %s must be a ROCm device tensor (the native path has no CPU fallback); got %s"
                           % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise TypeError("gnpde: %s must be %s, got %s" % (name, dtype, t.dtype))


def _rows(x, name, dtype=torch.float32):
    """[B,N,C] or [R,C] -> contiguous [R,C] view (fp32 unless stated)."""
    _require_gpu(x, name, dtype)
    x = x.contiguous()
    return x.reshape(-1, x.shape[-1])


STATE_DTYPES = (torch.float32, torch.bfloat16)  # K1 storage types (fp32 math either way)


# --------------------------------------------------------------------------- graph
class _TicketOrder(object):
    """Launch ordering of a plan whose kernels keep arrival tickets in it (K1's
    hub rows, the statistics kernel's long groups: heavy[].w, include/gnpde.h):
    two launches on one plan must never overlap.  A launch on a different stream
    than the plan's previous one first waits for everything already queued on
    that stream (an event; free for the usual single-stream use).  During graph
    capture the capture itself orders the launches."""
    last_stream = None
    n_heavy = 0

    def order_launch(self, dev):
        if self.n_heavy == 0:
            return
        s = torch.cuda.current_stream(dev)
        last = self.last_stream
        if last is not None and last != s and not torch.cuda.is_current_stream_capturing():
            ev = torch.cuda.Event()
            ev.record(last)
            s.wait_event(ev)
        self.last_stream = s


class Plan(_TicketOrder):
    """Wavefront work items over a grouped CSR (gnpde_plan_build)."""

    def __init__(self, items, heavy, n_items, n_heavy, n_slots, chunk):
        self.items, self.heavy = items, heavy
        self.n_items, self.n_heavy, self.n_slots = n_items, n_heavy, n_slots
        self.chunk = chunk
        self.last_stream = None


class GroupedCSR(object):
    """Edges grouped by one endpoint: key_row 0 -> aggregation CSR (by source),
    key_row 1 -> CSC (by destination)."""

    def __init__(self, rowptr, col, perm, R, nnz, key_row, plan):
        self.rowptr, self.col, self.perm = rowptr, col, perm
        self.R, self.nnz, self.key_row, self.plan = R, nnz, key_row, plan
        self._rowidx = None
        self._stats_plan = None
        self._seg_plans = {}

    @property
    def rowidx(self):
        """Row of every CSR position (edge-parallel kernels)."""
        if self._rowidx is None:
            ri = torch.empty(max(self.nnz, 1), dtype=torch.int32, device=self.rowptr.device)
            _lib.call("gnpde_csr_rowidx", _ptr(self.rowptr), self.R, self.nnz, _ptr(ri), _stream(ri.device))
            self._rowidx = ri
        return self._rowidx

    def seg_plan(self, eb, long_items=False, long_max=None):
        """Edge-block plan of the segmented-softmax kernel (K2) for blocks of at
        most ``eb`` edges (SegPlan), built once per grouped CSR and block size.
        long_items=True (reference-score statistics): groups longer than eb
        as long items of at most ``long_max`` edges (default seg_long_max())
        instead of eb-edge chunks + a fixup launch."""
        key = (eb, bool(long_items), long_max)
        if key not in self._seg_plans:
            self._seg_plans[key] = build_seg_plan(self.rowptr, eb, long_items, long_max)
        return self._seg_plans[key]

    def seg_plan_rows(self, r0, r1, eb, long_items=False, long_max=None):
        """seg_plan over the groups [r0, r1) only (their group ids the CSR's): the
        statistics of one rank's block of destination rows (softmax_stats(rows=))."""
        key = ('rows', int(r0), int(r1), eb, bool(long_items), long_max)
        if key not in self._seg_plans:
            self._seg_plans[key] = build_seg_plan(self.rowptr[int(r0):int(r1) + 1], eb, long_items, long_max,
                                                  group_offset=r0)
        return self._seg_plans[key]

    @property
    def stats_plan(self):
        """Plan with small chunks for the 8-lanes-per-group statistics kernel."""
        if self._stats_plan is None:
            self._stats_plan = build_plan(self.rowptr, self.R, self.nnz, STATS_CHUNK)
        return self._stats_plan


def validate_edge_index(edge_index, num_nodes):
    _require_gpu(edge_index, "edge_index", torch.int64)
    if edge_index.dim() != 3 or edge_index.shape[1] != 2:
        raise ValueError("edge_index must be [B,2,E], got %s" % (tuple(edge_index.shape),))
    if edge_index.numel():
        lo, hi = int(edge_index.min()), int(edge_index.max())  # once per graph
        if lo < 0 or hi >= num_nodes:
            raise IndexError("edge_index values must be in [0, %d), got [%d, %d]" % (num_nodes, lo, hi))


def build_plan(rowptr, R, nnz, chunk=DEFAULT_CHUNK):
    dev = rowptr.device
    cap_items = R + 2 * (nnz // chunk) + 2
    cap_heavy = nnz // chunk + 2
    items = torch.empty(cap_items * 4, dtype=torch.int32, device=dev)
    heavy = torch.empty(cap_heavy * 4, dtype=torch.int32, device=dev)
    ws_bytes = _lib.fn("gnpde_plan_workspace_bytes")(R)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    n_it, n_hv, n_sl = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("gnpde_plan_build", _ptr(rowptr), R, chunk, _ptr(items), cap_items, _ptr(heavy), cap_heavy,
              ctypes.byref(n_it), ctypes.byref(n_hv), ctypes.byref(n_sl), _ptr(ws), ws_bytes, _stream(dev))
    if PLAN_ORDER != "rows" and n_it.value > 1:
        it = items[:n_it.value * 4].view(-1, 4)
        ln = (it[:, 2] - it[:, 1]).long()
        if PLAN_ORDER == "classes":
            # length classes (powers of two) longest first, row order inside a class: the
            # wavefronts dispatched last are short, and neighbouring items touch neighbouring rows
            key = -torch.floor(torch.log2(ln.clamp(min=1).double())).long()
        elif PLAN_ORDER == "hubs":
            key = (it[:, 3] < 0).long()  # hub chunks first, then every row in row order
        else:
            key = -ln  # longest items first (stable): the wavefronts dispatched last are the short ones
        order = torch.argsort(key, stable=True)
        it.copy_(it[order])
    return Plan(items, heavy, n_it.value, n_hv.value, n_sl.value, chunk)


class SegPlan(_TicketOrder):
    """Work items of gnpde_seg_softmax_f32 (include/gnpde.h): ``items`` int4
    {e_begin, e_end, -1, first_group} — consecutive whole groups packed greedily
    up to ``eb`` edges — and ``chunk_items`` {e_begin, e_end, slot, group}
    covering groups of more than eb edges in eb-edge chunks, ``heavy`` {group,
    first_slot, n_chunks, 0} per long group."""

    def __init__(self, eb, items, n_items, chunk_items, n_chunk, heavy, n_heavy, n_hub=0, n_long=0):
        self.eb = eb
        self.items, self.n_items = items, n_items
        # reference statistics: hub chunk items, then long items (one wavefront
        # each) at the front of ``items``
        self.n_hub, self.n_long = n_hub, n_long
        self.chunk_items, self.n_chunk = chunk_items, n_chunk
        self.heavy, self.n_heavy = heavy, n_heavy
        self.n_slots = n_chunk
        self.last_stream = None


def seg_long_max():
    """Edges of a long statistics item (gnpde_seg_long_edges, csrc/attention.hip kSegLongMax)."""
    return int(_lib.fn("gnpde_seg_long_edges")())


def build_seg_plan(rowptr, eb, long_items=False, long_max=None, group_offset=0):
    """gnpde_seg_plan_build on a host copy of rowptr (once per graph and block size).
    long_items=True (the reference statistics over the CSC): every group longer
    than eb becomes LONG item {e_begin, e_end, -2, group} (one wavefront) when it
    has at most seg_long_max() edges, else seg_long_max()-edge HUB CHUNK items
    {e_begin, e_end, slot, hub} with a hub table entry {group, first_slot,
    n_chunks, 0} (``heavy``: arrival tickets, the last chunk merges); hub chunks
    first (longest hubs first), then long items longest first, then the packed
    short items.  ``rowptr`` may be a row range [r0, r1] of a grouped CSR (edge
    positions stay absolute): ``group_offset`` = r0 then turns the plan's group ids
    into the CSR's (the statistics of one rank's destination rows, gnpde.dist)."""
    rp = np.ascontiguousarray(rowptr.cpu().numpy().astype(np.int32))
    R = rp.shape[0] - 1
    nnz = int(rp[-1])
    cap_i, cap_c, cap_h = max(R, 1), nnz // eb + R + 1, nnz // eb + 2
    items = np.zeros((cap_i, 4), np.int32)
    chunks = np.zeros((cap_c, 4), np.int32)
    heavy = np.zeros((cap_h, 4), np.int32)
    ni, nc, nh = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call("gnpde_seg_plan_build", rp.ctypes.data, R, eb, items.ctypes.data, cap_i, chunks.ctypes.data, cap_c,
              heavy.ctypes.data, cap_h, ctypes.byref(ni), ctypes.byref(nc), ctypes.byref(nh))
    dev = rowptr.device

    def dev32(a, n):
        return torch.from_numpy(np.ascontiguousarray(a[:max(n, 1)]).reshape(-1)).to(dev)

    go = int(group_offset)
    items[:ni.value, 3] += go  # first group of a short item
    if long_items:
        long_max = seg_long_max() if long_max is None else int(long_max)
        rows = heavy[:nh.value, 0].astype(np.int64)
        s0, s1 = rp[rows].astype(np.int64), rp[rows + 1].astype(np.int64)
        order = np.argsort(-(s1 - s0), kind="stable")
        hub_chunks, hubs = [], []
        for i in order:
            if s1[i] - s0[i] <= long_max:
                continue
            first = len(hub_chunks)
            for c0 in range(int(s0[i]), int(s1[i]), long_max):
                hub_chunks.append((c0, min(c0 + long_max, int(s1[i])), len(hub_chunks), len(hubs)))
            hubs.append((int(rows[i]) + go, first, len(hub_chunks) - first, 0))
        longs = [(int(s0[i]), int(s1[i]), -2, int(rows[i]) + go) for i in order if s1[i] - s0[i] <= long_max]
        front = np.asarray(hub_chunks + longs, np.int32).reshape(-1, 4)
        all_items = np.concatenate([front, items[:ni.value]], 0)
        table = np.asarray(hubs, np.int32).reshape(-1, 4)
        plan = SegPlan(eb, dev32(all_items, all_items.shape[0]), all_items.shape[0],
                       dev32(np.zeros((1, 4), np.int32), 0), 0, dev32(table, len(hubs)), len(hubs),
                       n_hub=len(hub_chunks), n_long=len(longs))
        plan.n_slots = len(hub_chunks)
        return plan

    chunks[:nc.value, 3] += go
    heavy[:nh.value, 0] += go
    # items and chunk items back to back in one buffer: K2 then covers both in one launch
    both = dev32(np.concatenate([items[:ni.value], chunks[:max(nc.value, 1)]], 0), ni.value + max(nc.value, 1))
    it_view = both[:max(ni.value, 1) * 4] if ni.value else dev32(items, 0)
    ch_view = both[ni.value * 4:]
    return SegPlan(eb, it_view, ni.value, ch_view, nc.value, dev32(heavy, nh.value), nh.value)


def build_grouped(edge_index, num_nodes, key_row, chunk=DEFAULT_CHUNK, plan=True):
    """COO [B,2,E] -> block-diagonal CSR grouped by edge_index[:, key_row] (+ plan)."""
    B, _, E = edge_index.shape
    N = int(num_nodes)
    R, nnz = B * N, B * E
    dev = edge_index.device
    ei = edge_index.contiguous()
    rowptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    perm = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    ws_bytes = _lib.fn("gnpde_csr_workspace_bytes")(B, E, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.call("gnpde_csr_build", _ptr(ei), B, E, N, key_row, _ptr(rowptr), _ptr(col), _ptr(perm), _ptr(ws), ws_bytes,
              _stream(dev))
    plan = build_plan(rowptr, R, nnz, chunk) if plan else None
    return GroupedCSR(rowptr, col, perm, R, nnz, key_row, plan)


# --------------------------------------------------------------------------- graph normalisation
def add_self_loops(edge_index, edge_weight, fill_value, num_nodes):
    """gnpde_add_self_loops: non-loop edges in COO order, then one loop per node
    with its last existing loop's weight or fill_value (intended semantics of
    src/utils.py:16-42).  -> (edge_index [B,2,K+N] int64, weights [B,K+N] fp32)."""
    validate_edge_index(edge_index, num_nodes)  # the kernels index per-node arrays with these ids
    B, _, E = edge_index.shape
    N = int(num_nodes)
    ei = edge_index.contiguous()
    dev = ei.device
    w = None
    if edge_weight is not None:
        _require_gpu(edge_weight, "edge_weight", torch.float32)
        w = edge_weight.contiguous()
        if tuple(w.shape) != (B, E):
            raise ValueError("edge_weight shape %s != [%d,%d]" % (tuple(w.shape), B, E))
    ws_bytes = _lib.fn("gnpde_self_loops_workspace_bytes")(B, E, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    counts = (ctypes.c_int64 * B)()
    _lib.call("gnpde_self_loops_count", _ptr(ei), B, E, counts, _ptr(ws), ws_bytes, _stream(dev))
    ks = sorted(set(int(c) for c in counts))
    if len(ks) != 1:
        raise ValueError("batched edge lists have different lengths after self-loop insertion %s; the [B,2,E] "
                         "format needs equal counts per batch element" % sorted(k + N for k in ks))
    K = ks[0]
    ei_out = torch.empty(B, 2, K + N, dtype=torch.int64, device=dev)
    w_out = torch.empty(B, K + N, dtype=torch.float32, device=dev)
    _lib.call("gnpde_add_self_loops", _ptr(ei), _ptr(w), B, E, N, float(fill_value), K, _ptr(ei_out), _ptr(w_out),
              _ptr(ws), ws_bytes, _stream(dev))
    return ei_out, w_out


def norm_weights(edge_index, edge_weight, num_nodes, mode):
    """gnpde_norm_weights_f32: rw (norm_dim 0 / 1) or symmetric gcn weights, degrees
    summed in COO order over a grouped CSR (src/utils.py:177-194, :215-233)."""
    validate_edge_index(edge_index, num_nodes)  # the kernels index per-node arrays with these ids
    B, _, E = edge_index.shape
    N = int(num_nodes)
    ei = edge_index.contiguous()
    w = None
    if edge_weight is not None:
        _require_gpu(edge_weight, "edge_weight", torch.float32)
        w = edge_weight.contiguous()
    key_row = 0 if mode == _lib.NORM_RW_ROW else 1
    grouped = build_grouped(ei, N, key_row, plan=False)
    fac = torch.empty(B * N, dtype=torch.float32, device=ei.device)
    out = torch.empty(B, E, dtype=torch.float32, device=ei.device)
    _lib.call("gnpde_norm_weights_f32", _ptr(ei), _ptr(w), B, E, N, _ptr(grouped.rowptr), _ptr(grouped.perm), int(mode),
              _ptr(fac), _ptr(out), _stream(ei.device))
    return out


class GraphCSR(object):
    """All per-graph device structures the RHS needs, built once and reused by
    every RHS evaluation (the reference rebuilds a dense [B,N,N] per call)."""

    def __init__(self, edge_index, num_nodes, chunk=None, validate=True):
        if validate:
            validate_edge_index(edge_index, num_nodes)
        self.edge_index = edge_index
        self.B, _, self.E = edge_index.shape
        self.N = int(num_nodes)
        self.R = self.B * self.N
        self.nnz = self.B * self.E
        self.chunk = chunk = auto_chunk(self.R, chunk)
        self.csr = build_grouped(edge_index, self.N, 0, chunk)
        self._csc = None
        self._indeg = None

    @property
    def csc(self):
        if self._csc is None:
            self._csc = build_grouped(self.edge_index, self.N, 1, self.chunk)
        return self._csc

    @property
    def indeg(self):
        """In-degree per row: the CSC's row lengths (the reference scores' key sum is
        the only reader and runs with the CSC's statistics; a per-edge atomic count
        contends on the hub columns: 0.3-1.9 ms per graph)."""
        if self._indeg is None:
            rp = self.csc.rowptr
            self._indeg = (rp[1:] - rp[:-1]).to(torch.int32).contiguous()
        return self._indeg

    def gather_weights(self, w, transpose=False, out=None):
        """COO-order weights [B,E] or attention [B,E,h] -> CSR-order [nnz] (head mean);
        transpose=True gives CSC order.  ``out``: an existing [nnz] fp32 buffer to fill."""
        _require_gpu(w, "edge weights", torch.float32)
        w = w.contiguous()
        if w.dim() == 2:
            H = 1
        elif w.dim() == 3:
            H = w.shape[2]
        else:
            raise ValueError("weights must be [B,E] or [B,E,h]")
        if w.shape[0] != self.B or w.shape[1] != self.E:
            raise ValueError("weights shape %s does not match edge_index [%d,2,%d]" % (tuple(w.shape), self.B,
                                                                                        self.E))
        if out is None:
            out = torch.empty(max(self.nnz, 1), dtype=torch.float32, device=w.device)
        elif out.dtype != torch.float32 or out.numel() != max(self.nnz, 1) or not out.is_contiguous() or \
                out.device != w.device:
            raise ValueError("gather_weights: out must be a contiguous fp32 [%d] buffer on %s" % (max(self.nnz, 1),
                                                                                              w.device))
        perm = self.csc.perm if transpose else self.csr.perm
        _lib.call("gnpde_gather_weights_f32", _ptr(w), self.nnz, H, _ptr(perm), _ptr(out),
                  _stream(w.device))
        return out

    @property
    def node_layout(self):
        """The graph's locality numbering (NodeLayout), built once."""
        if getattr(self, '_layout', None) is None:
            self._layout = NodeLayout(self)
        return self._layout


# --------------------------------------------------------------------------- state layout
# The fixed-grid integrator keeps the state of a large graph in a locality
# numbering of its nodes for the whole solve (gnpde.integrator.odeint_fixed):
# permuted once on entry, back once on exit.  "degree": nodes by in-degree,
# descending (stable), per batch element — the rows the aggregation gathers most
# sit together at the front of the state.  G-arxiv rk4 step (tools/reorder_bench.py,
# profiles/r02b_reorder.jsonl): 420 -> 370 us; the same numbering applied to the
# item ORDER only (rows of x where they were) gains nothing, so it is where the
# gathered rows live, not when they are gathered.  "none" disables.
NODE_ORDER = os.environ.get("GNPDE_NODE_ORDER", "degree")
LAYOUT_MIN_ROWS = 32768          # below this the state sits in L2 / the Infinity Cache anyway
# and the two permutations would cost more than they save (GNPDE_LAYOUT_MIN_MB overrides)
LAYOUT_MIN_BYTES = int(float(os.environ.get("GNPDE_LAYOUT_MIN_MB", 16)) * (1 << 20))


# A solve leaves FROZEN rows out of its RHS launches (gnpde.integrator) when
# the graph has at least this many of them; below it there is nothing to gain.
FROZEN_MIN_ROWS = 1024


def self_loop_only_rows(rowptr, col, R, nnz):
    """bool [R]: the rows of a grouped CSR whose only edge is their own self loop (graph only:
    whatever its weight).  With weight 1 such a row has f = a*(1*x - x) = 0."""
    rp = rowptr.long()
    ln = rp[1:] - rp[:-1]
    if nnz == 0:
        return torch.zeros(R, dtype=torch.bool, device=rowptr.device)
    first = col[rp[:-1].clamp(max=nnz - 1)].long()
    return (ln == 1) & (first == torch.arange(R, device=rowptr.device))


def layout_order(deg, cand):
    """The NodeLayout's order of each batch element's nodes: ``deg`` [B,N] in-degrees, ``cand``
    [B,N] bool (self_loop_only_rows) -> the old local id at each new position.  In-degree
    descending, stable; inside the in-degree-1 class the candidates come last — a candidate of
    in-degree 1 is gathered by nothing but its own self loop, so with B = 1 and no row of
    in-degree 0 these rows are the state's last rows [n_live, R) (FrozenRows)."""
    key = -2 * deg.long() + (cand & (deg == 1)).long()
    return torch.argsort(key, dim=1, stable=True)


class FrozenRows(object):
    """The frozen rows of a NodeLayout's graph (B = 1): rows [n_live, n_rows), each with one
    edge, its own self loop, and in-degree 1 — no other row gathers them; their items are the
    plan's items [n_live_items, n_items), and ``pos`` the CSR positions of their edges.
    Graph-only: whether a solve may leave them out also needs every weight at ``pos`` to be
    exactly 1.0 (frozen_weights_unit)."""

    def __init__(self, plan, n_live, n_rows, n_live_items, pos):
        self.plan, self.n_live, self.n_rows, self.n_live_items, self.pos = plan, n_live, n_rows, n_live_items, pos


def frozen_weights_unit(fr, w_csr):
    """True when every frozen row's CSR-order weight is exactly 1.0f (one host read)."""
    return bool((w_csr.index_select(0, fr.pos) == 1.0).all())


class NodeLayout(object):
    """In-degree numbering of a GraphCSR's nodes and the same graph relabelled.

    ``order[k]`` = user row held at internal row k, ``new_id[i]`` = internal row
    of user row i (global rows, batch elements kept in their own row ranges).
    ``graph`` is the GraphCSR of ``new_id[edge_index]``: the COO edge order is
    unchanged (so COO-order weights apply as they are) and each row keeps its
    edges in COO order, so every output row is summed over the same edges in the
    same order — results are bit-identical to the user numbering."""

    def __init__(self, g):
        B, N, R = g.B, g.N, g.R
        dev = g.edge_index.device
        deg = g.indeg.view(B, N).long()
        cand = self_loop_only_rows(g.csr.rowptr, g.csr.col, R, g.nnz).view(B, N)
        local_order = layout_order(deg, cand)  # old local id at each new position
        base = (torch.arange(B, device=dev, dtype=torch.int64) * N).view(B, 1)
        self.order = (local_order + base).reshape(R)
        self.order32 = self.order.to(torch.int32)  # the stage epilogue's out_rows (last step of a solve)
        self.new_id = torch.empty_like(self.order)
        self.new_id[self.order] = torch.arange(R, device=dev, dtype=torch.int64)
        local_new = self.new_id.view(B, N) - base
        ei = g.edge_index
        eip = torch.gather(local_new, 1, ei.reshape(B, -1)).view(ei.shape)
        self.graph = GraphCSR(eip, N, chunk=g.chunk, validate=False)
        self.R = R
        self.frozen = self._frozen_rows(deg, cand) if B == 1 else None

    def _frozen_rows(self, deg, cand):
        """The FrozenRows of the relabelled graph, or None: the self-loop-only rows nobody else
        gathers must be the last rows (no row of in-degree 0 behind them) and their items the
        last of the plan.  Two host reads, once per graph."""
        R = self.R
        tail = cand & (deg == 1)
        nf, n0 = torch.stack([tail.sum(), (deg == 0).sum()]).tolist()
        plan = self.graph.csr.plan
        if nf == 0 or n0 != 0 or plan is None or plan.n_items < nf:
            return None
        it = plan.items[:plan.n_items * 4].view(-1, 4)[plan.n_items - nf:]
        rows = torch.arange(R - nf, R, device=it.device, dtype=it.dtype)
        if not bool(((it[:, 0] == rows) & (it[:, 3] < 0) & (it[:, 2] - it[:, 1] == 1)).all()):
            return None
        return FrozenRows(plan, R - nf, R, plan.n_items - nf, it[:, 1].long())

    def to_internal(self, y):
        """[B,N,C] (or [R,C]) in user order -> the same in internal order (new tensor)."""
        C = y.shape[-1]
        return y.reshape(-1, C).index_select(0, self.order).view(y.shape)

    def to_user(self, y):
        """[..., B, N, C] in internal order -> user order (new tensor)."""
        C = y.shape[-1]
        return y.reshape(-1, self.R, C).index_select(1, self.new_id).view(y.shape)


def layout_worthwhile(R, C, elem_size):
    return NODE_ORDER == "degree" and R >= LAYOUT_MIN_ROWS and R * C * elem_size >= LAYOUT_MIN_BYTES


# --------------------------------------------------------------------------- block weight producers
def mix_weights(att, edge_weight=None, gamma=None):
    """COO-order [B,E] weights from attention [B,E,h] (or [B,E]):
    mean_h(att) [* (1 - sigmoid(gamma)) + edge_weight * sigmoid(gamma)]
    (MixedODEblock.get_mixed_attention, src/block_mixed.py:29-33; gamma=None:
    the plain head mean of src/block_transformer_hard_attention.py:42,60)."""
    _require_gpu(att, "attention", torch.float32)
    att = att.contiguous()
    if att.dim() == 2:
        H = 1
    elif att.dim() == 3:
        H = att.shape[2]
    else:
        raise ValueError("attention must be [B,E] or [B,E,h]")
    B, E = att.shape[0], att.shape[1]
    if (gamma is None) != (edge_weight is None):
        raise ValueError("mix_weights: gamma and edge_weight go together")
    if edge_weight is not None:
        _require_gpu(edge_weight, "edge_weight", torch.float32)
        edge_weight = edge_weight.contiguous()
        if tuple(edge_weight.shape) != (B, E):
            raise ValueError("edge_weight shape %s != [%d,%d]" % (tuple(edge_weight.shape), B, E))
        gamma = _scalar(gamma, "gamma", att.device)
    out = torch.empty(B, E, dtype=torch.float32, device=att.device)
    _lib.call("gnpde_mix_weights_f32", _ptr(att), H, _ptr(edge_weight), _ptr(gamma), B * E, _ptr(out),
              _stream(att.device))
    return out


def group_normalize(grouped, w):
    """w[e] / (sum of w over e's group + 1e-16) in COO order, groups = rows of
    ``grouped`` (HardAttODEblock.renormalise_attention,
    src/block_transformer_hard_attention.py:32-35)."""
    _require_gpu(w, "weights", torch.float32)
    w = w.contiguous()
    if w.numel() != grouped.nnz:
        raise ValueError("group_normalize: %d weights for %d edges" % (w.numel(), grouped.nnz))
    out = torch.empty_like(w)
    nbytes = _lib.fn("gnpde_group_normalize_workspace_bytes")(grouped.nnz)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    _lib.call("gnpde_group_normalize_f32", _ptr(grouped.rowptr), _ptr(grouped.perm), grouped.R, grouped.nnz,
              _ptr(w), _ptr(out), _ptr(ws), nbytes, _stream(w.device))
    return out


def quantile(v, q):
    """torch.quantile(v, q) (linear interpolation) as a device scalar [1]."""
    _require_gpu(v, "values", torch.float32)
    v = v.contiguous().reshape(-1)
    n = v.numel()
    if n == 0:
        raise ValueError("quantile of an empty tensor")
    ws_bytes = _lib.fn("gnpde_quantile_workspace_bytes")(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
    out = torch.empty(1, dtype=torch.float32, device=v.device)
    _lib.call("gnpde_quantile_f32", _ptr(v), n, float(q), _ptr(out), _ptr(ws), ws_bytes, _stream(v.device))
    return out


def threshold_mask(v, thr):
    """(v with every entry <= *thr set to 0, device int64 count of the kept ones):
    the hard-attention sampling as weights over the full graph (gnpde_threshold_mask_f32)."""
    _require_gpu(v, "values", torch.float32)
    _require_gpu(thr, "threshold", torch.float32)
    v = v.contiguous()
    out = torch.empty_like(v)
    count = torch.empty(1, dtype=torch.int64, device=v.device)
    _lib.call("gnpde_threshold_mask_f32", _ptr(v), v.numel(), _ptr(thr), _ptr(out), _ptr(count), _stream(v.device))
    return out, count


# --------------------------------------------------------------------------- epilogue helpers
def _flags(rhs, alpha_sigmoid, add_source):
    f = 0
    if rhs:
        f |= _lib.EPI_RHS
        if alpha_sigmoid:
            f |= _lib.ALPHA_SIGMOID
        if add_source:
            f |= _lib.ADD_SOURCE
    return f


def _scalar(t, name, dev):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.tensor(float(t), dtype=torch.float32, device=dev)
    _require_gpu(t, name)
    if t.dtype != torch.float32:
        t = t.float()
    return t.reshape(1).contiguous()


class Stage(object):
    """Fused Runge-Kutta stage outputs of one RHS evaluation (gnpde_stage_epilogue_t):
    ``f_out`` receives f (optional); each entry of ``outs`` is
    (out, base, cb, cf, [(k_j, c_j), ...]) meaning out = cb*base + cf*f + sum_j c_j*k_j.
    ``base`` may be None, the RHS input x, or ``out`` itself (in place).  No
    output may alias the RHS input.  An output may be the same array as its base or
    as one of the k operands (same dtype and size: every element is read by the lane
    that writes it, before its store), but only without ``out_rows``.  The k operands
    of all outputs (and of the error term) are collected into the stage's shared
    operand table, each distinct tensor once (read once per row by the kernel).

    ``err`` (the adaptive solvers' embedded-pair error rows): (rows, (base, cb,
    cf, [(k_j, c_j)...]), y0, y1_out, atol, rtol) -> rows[r] = sum_c (e / tol)^2
    in fp64 with e the combination, tol = atol + rtol * max(|y0|, |y1|), y1 = the
    RHS input (y1_out = -1) or output ``y1_out``.

    ``dense`` (ABI 8, the plain-weight K1 only): the step's dense output folded into
    the launch — (slot, rows, t, dt, tab, table): ``slot`` a device int64 holding the
    output array's address, ``rows`` its int32 row map or None, ``t`` device fp64
    {step start, output time}, ``dt`` the device fp64 step size, ``tab`` device fp32
    scratch of STAGE_MAX_K + 3 (the launch's coefficients), ``table`` the
    basis coefficients: {'base': [5], 'f': [5], k tensor: [5]} over w = (cy0 + cy1 +
    cym, h cy1, h cym, cf0, cf1) of torchdiffeq's interpolant (include/gnpde.h).
    The launch that applies them has a ``slot``; an earlier launch of the step forms
    ``tab``: slot None and ``table`` the applying stage's ``dense_matrix()``.
    ``scale_rows`` (ABI 8, with ``err``): fp64 [R], rows[r] = sum_c (y0 / tol)^2."""

    def __init__(self, f_out=None, outs=(), out_rows=None, dot=None, err=None, scale=None, f_lin=0.0,
                 unscaled=(), dense=None, scale_rows=None):
        self.f_out = f_out
        # indices of the outputs whose cf / c_j do NOT take ``scale`` (ABI 6 unscaled_outs)
        self.unscaled = tuple(unscaled)
        # nonzero: the RHS value becomes x + scale*f_lin*f (the affine stage derivative, ABI 5)
        self.f_lin = float(f_lin)
        # a device fp32 0-d tensor multiplying every cf and c_j (not cb): the adaptive step size
        self.scale = scale
        self.outs = list(outs)
        self.out_rows = out_rows  # int32 [R] or None: row r's ``outs`` stores go to row out_rows[r]
        # (y, rows, coef, accumulate) or None: rows[r] (+)= coef * <f[r], y[r]> in fp64 (fp32 state)
        self.dot = dot
        self.err = err
        self.dense = dense
        self.scale_rows = scale_rows

    def _operands(self):
        """The distinct k tensors of every combination, in first-use order."""
        ks, seen = [], set()
        combos = [o[4] for o in self.outs] + ([self.err[1][3]] if self.err is not None else [])
        if self.dense is not None:
            if isinstance(self.dense[5], dict):
                combos.append([(k, 0.0) for k in self.dense[5] if isinstance(k, torch.Tensor)])
        for terms in combos:
            for k, _ in terms:
                if k.data_ptr() not in seen:
                    seen.add(k.data_ptr())
                    ks.append(k)
        return ks

    @property
    def wide(self):
        """True when the stage needs the adaptive solvers' wide epilogue (error rows,
        or more operands than the fixed-grid epilogues prefetch)."""
        return self.err is not None or len(self._operands()) > _lib.STAGE_PRE_K

    def tensors(self):
        ts = [self.f_out] if self.f_out is not None else []
        if self.dot is not None:
            ts.append(self.dot[0])
        for out, base, _cb, _cf, _ks in self.outs:
            ts.append(out)
            if base is not None:
                ts.append(base)
        if self.err is not None:
            if self.err[1][0] is not None:
                ts.append(self.err[1][0])
            ts.append(self.err[2])
        ts.extend(self._operands())
        return ts

    def struct(self, x_input, shift=0, like=None):
        """ctypes struct; every pointer is moved back by ``shift`` bytes (row-block
        buffers addressed with global row ids, dist.RowShardedLaplacian).
        ``x_input`` = the RHS input (None for a stage applied without one: ``like``
        then gives the row shape)."""
        ref = x_input if x_input is not None else like
        if len(self.outs) > _lib.STAGE_MAX_OUT:
            raise ValueError("at most %d stage outputs" % _lib.STAGE_MAX_OUT)
        ks = self._operands()
        if len(ks) > _lib.STAGE_MAX_K:
            raise ValueError("at most %d distinct k operands per stage" % _lib.STAGE_MAX_K)
        slot = {k.data_ptr(): j for j, k in enumerate(ks)}
        st = _lib.StageEpilogue()
        st.f_out = self.f_out.data_ptr() - shift if self.f_out is not None else None
        st.n_out = len(self.outs)
        st.nk = len(ks)
        for j, k in enumerate(ks):
            st.k[j] = k.data_ptr() - shift
        if self.out_rows is not None:
            if shift:
                raise ValueError("out_rows cannot be combined with shifted row-block buffers")
            _require_gpu(self.out_rows, "out_rows", torch.int32)
            if self.out_rows.numel() * ref.shape[-1] != ref.numel():
                raise ValueError("out_rows must hold one row index per RHS row")
            st.out_rows = self.out_rows.data_ptr()
        if self.dot is not None:
            y, rows, coef, accumulate = self.dot
            _require_gpu(rows, "dot rows", torch.float64)
            if rows.numel() * ref.shape[-1] != ref.numel() or shift:
                raise ValueError("dot rows must hold one fp64 per RHS row")
            st.dot_with, st.dot_rows = y.data_ptr(), rows.data_ptr()
            st.dot_coef, st.dot_accumulate = float(coef), int(bool(accumulate))

        def fill(o, out, base, cb, cf, terms):
            o.out = out.data_ptr() - shift if out is not None else None
            o.base = base.data_ptr() - shift if base is not None else None
            o.cb = float(cb)
            o.cf = float(cf)
            for k, c in terms:
                o.c[slot[k.data_ptr()]] += float(c)

        for i, (out, base, cb, cf, terms) in enumerate(self.outs):
            if x_input is not None and out.data_ptr() == x_input.data_ptr():
                raise ValueError("a stage output may not alias the RHS input")
            if out.data_ptr() in slot or (base is not None and out.data_ptr() == base.data_ptr()):
                # in place: every element is read by the lane that writes it, before its store
                if self.out_rows is not None:
                    raise ValueError("a stage output that aliases its base or an operand cannot take out_rows")
                for t in [base] + ks:
                    if t is not None and t.data_ptr() == out.data_ptr() and (t.dtype != out.dtype
                                                                             or t.numel() != out.numel()):
                        raise ValueError("a stage output may alias its base or an operand only as the same array "
                                         "(dtype and size)")
            fill(st.o[i], out, base, cb, cf, terms)
        if self.err is not None:
            rows, (base, cb, cf, terms), y0, y1_out, atol, rtol = self.err
            _require_gpu(rows, "error rows", torch.float64)
            if rows.numel() * ref.shape[-1] != ref.numel() or shift:
                raise ValueError("error rows must hold one fp64 per RHS row")
            st.err_rows = rows.data_ptr()
            fill(st.err, None, base, cb, cf, terms)
            st.err_y0 = y0.data_ptr()
            st.err_y1 = int(y1_out)
            st.atol, st.rtol = float(atol), float(rtol)
        if self.scale is not None:
            _require_gpu(self.scale, "coefficient scale", torch.float32)
            st.coef_scale = self.scale.data_ptr()
        st.f_lin = self.f_lin
        st.unscaled_outs = sum(1 << i for i in self.unscaled)
        if self.scale_rows is not None:
            _require_gpu(self.scale_rows, "scale rows", torch.float64)
            if self.err is None or self.dot is not None or self.scale_rows.numel() * ref.shape[-1] != ref.numel():
                raise ValueError("scale rows: one fp64 per RHS row, with err and without dot")
            st.scale_rows = self.scale_rows.data_ptr()
        if self.dense is not None:
            dslot, drows, dtt, ddt, dtab, table = self.dense
            _require_gpu(dtab, "dense coefficient scratch", torch.float32)
            if dtab.numel() < _lib.DENSE_SLOTS + 1:
                raise ValueError("dense: coefficient scratch of %d floats" % (_lib.DENSE_SLOTS + 1))
            st.dense_tab = dtab.data_ptr()
            if shift:
                raise ValueError("dense: unshifted buffers only")
            if dslot is not None:  # the launch that applies the coefficients
                _require_gpu(dslot, "dense slot", torch.int64)
                if not self.outs:
                    raise ValueError("dense: needs output 0 (its base is y0)")
                st.dense_out = dslot.data_ptr()
                if drows is not None:
                    _require_gpu(drows, "dense rows", torch.int32)
                    if drows.numel() * ref.shape[-1] != ref.numel():
                        raise ValueError("dense rows must hold one row index per RHS row")
                    st.dense_rows = drows.data_ptr()
            if dtt is not None:  # the times: the launch that forms the coefficients
                _require_gpu(dtt, "dense times", torch.float64)
                _require_gpu(ddt, "dense step", torch.float64)
                if dtt.numel() < 2:
                    raise ValueError("dense: two times")
                st.dense_t, st.dense_dt = dtt.data_ptr(), ddt.data_ptr()
            mat = table if not isinstance(table, dict) else self._dense_matrix(table, slot)
            for m in range(_lib.DENSE_BASIS):
                for q in range(_lib.DENSE_SLOTS):
                    st.dense_m[m][q] = float(mat[m][q])
        return st

    @staticmethod
    def _dense_matrix(table, slot):
        mat = [[0.0] * _lib.DENSE_SLOTS for _ in range(_lib.DENSE_BASIS)]
        for key, w in table.items():
            if isinstance(key, str):
                q = {'base': 0, 'f': _lib.DENSE_SLOTS - 1}[key]
            else:
                q = 1 + slot[key.data_ptr()]
            if len(w) != _lib.DENSE_BASIS:
                raise ValueError("dense: %d basis coefficients per operand" % _lib.DENSE_BASIS)
            for m, v in enumerate(w):
                mat[m][q] += float(v)
        return mat

    def dense_matrix(self):
        """The basis-coefficient matrix [DENSE_BASIS][DENSE_SLOTS] of this stage's dense
        table over its own operand slots (what the launch forming the coefficients carries)."""
        ks = self._operands()
        return self._dense_matrix(self.dense[5], {k.data_ptr(): j for j, k in enumerate(ks)})


def stage_apply(stage, f, x, like):
    """The stage epilogue as a pass of its own (gnpde_stage_apply_f32 / _bf16):
    ``f`` the RHS value (None: a plain combination), ``x`` the RHS input (None
    unless a base or the error tolerance reads it), ``like`` any row array of the
    stage (fixes the row count, width and storage type)."""
    dt = like.dtype
    if dt not in STATE_DTYPES:
        raise TypeError("stage_apply: state dtype %s" % dt)
    lr = _rows(like, "stage rows", dt)
    R, C = lr.shape
    for t in stage.tensors() + [v for v in (f, x) if v is not None]:
        _require_gpu(t, "stage tensor", dt)
        if not t.is_contiguous() or t.numel() != lr.numel():
            raise ValueError("stage tensors must be contiguous and shaped alike")
    st = stage.struct(x, like=lr)
    name = "gnpde_stage_apply_bf16" if dt == torch.bfloat16 else "gnpde_stage_apply_f32"
    _lib.call(name, R, C, C, _ptr(f), _ptr(x), ctypes.byref(st), _stream(lr.device))


def spmm_rhs(g, w_csr, x, x0=None, alpha=None, beta=None, rhs=True, alpha_sigmoid=True, add_source=False,
             out=None, transpose=False, stage=None, frozen=None):
    """K1: f = a*(A x - x) [+ b*x0] (or A x with rhs=False).  x [B,N,C] fp32, or
    bf16 storage (gnpde_spmm_rhs_bf16: x, x0, f and stage tensors bf16, sums in
    fp32).

    transpose=True aggregates over the CSC instead (A^T x; ``w_csr`` must then
    be in CSC order) — the backward of the RHS with respect to x.
    stage: a ``Stage`` -> the fused Runge-Kutta outputs are written instead of f
    (returns None).  The adaptive solvers' wide stages (Stage.wide) are fused
    with plain weights; with weights computed on the fly (RefDstWeights, GatWeights,
    RefDstSquareplusWeights) f is formed first and the stage applied in a second pass
    (stage_apply).
    frozen: (FrozenRows, home, steps) — a launch of an rk4 solve that leaves the graph's frozen
    rows out: home None runs the plan's other items only (nothing reads the frozen rows'
    stage inputs); home = the state the solve began with (the solve's last launch) also takes
    the frozen rows of ``home`` through ``steps`` steps' stage epilogues
    (gnpde_spmm_rhs_frozen_f32): the bits of ``steps`` full steps."""
    on_the_fly = (RefDstWeights, GatWeights, RefDstSquareplusWeights)
    if stage is not None and stage.wide and isinstance(w_csr, on_the_fly):
        f = spmm_rhs(g, w_csr, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                     add_source=add_source, transpose=transpose)
        stage_apply(stage, f, x, x)
        return None
    shape = x.shape
    dt = x.dtype if isinstance(x, torch.Tensor) and x.dtype in STATE_DTYPES else torch.float32
    xr = _rows(x, "x", dt)
    C = xr.shape[1]
    if xr.shape[0] != g.R:
        raise ValueError("x has %d rows, graph has %d" % (xr.shape[0], g.R))
    dev = xr.device
    a = _scalar(alpha, "alpha", dev) if rhs else None
    if rhs and a is None:
        raise ValueError("spmm_rhs: alpha required")
    b = _scalar(beta, "beta", dev) if add_source else None
    x0r = _rows(x0, "x0", dt) if add_source else None
    st = None
    if stage is not None:
        for t in stage.tensors():
            _require_gpu(t, "stage tensor", dt)
            if not t.is_contiguous() or t.numel() != xr.numel():
                raise ValueError("stage tensors must be contiguous and shaped like x")
        st = ctypes.byref(stage.struct(xr))
    elif out is None:
        out = torch.empty_like(xr)
    grouped = g.csc if transpose else g.csr
    plan = grouped.plan
    partials = _partials(plan, C, dev)
    plan.order_launch(dev)
    epi = (C, _ptr(xr), C, _ptr(x0r), C, _ptr(a), _ptr(b), _flags(rhs, alpha_sigmoid, add_source), _ptr(out), C,
           _ptr(partials), plan.n_slots, st, _stream(dev))
    items, col = plan.items, grouped.col
    if frozen is not None:
        fr, home, steps = frozen
        if (fr.plan is not plan or stage is None or dt != torch.float32 or not isinstance(w_csr, torch.Tensor)
                or add_source or not rhs):
            raise ValueError("spmm_rhs: frozen rows take the plain-weight fp32 stage launches of their own graph")
        if home is None:
            # GNPDE_LIVE_ITEMS: the launch code stripes these launches' columns on a large graph
            live = epi[:7] + (epi[7] | _lib.LIVE_ITEMS,) + epi[8:]
            _lib.call("gnpde_spmm_rhs_f32", _ptr(items), fr.n_live_items, _ptr(plan.heavy), plan.n_heavy,
                      _ptr(col), _ptr(w_csr), *live)
        else:
            hr = _rows(home, "frozen home", dt)
            if hr.shape != xr.shape:
                raise ValueError("spmm_rhs: the frozen rows' home must be shaped like x")
            _lib.call("gnpde_spmm_rhs_frozen_f32", _ptr(items), fr.n_live_items, _ptr(plan.heavy), plan.n_heavy,
                      _ptr(col), _ptr(w_csr), C, _ptr(xr), C, _ptr(a), _flags(rhs, alpha_sigmoid, add_source), C,
                      _ptr(partials), plan.n_slots, st, _ptr(hr), fr.n_live, fr.n_rows, int(steps), _stream(dev))
        return None
    if isinstance(w_csr, CompactWeights):  # the sampled graph: the plan's items over the retained edges
        if w_csr.grouped is not grouped or w_csr.transpose != bool(transpose):
            raise ValueError("spmm_rhs: compacted weights of another grouped CSR")
        items, col, w_csr = w_csr.items, w_csr.col, w_csr.w
    if dt == torch.bfloat16:
        if isinstance(w_csr, on_the_fly):
            raise ValueError("bf16 storage takes precomputed weights (attn_rhs(..., fuse=False))")
        _lib.call("gnpde_spmm_rhs_bf16", _ptr(items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
                  _ptr(col), _ptr(w_csr), *epi)
    elif isinstance(w_csr, RefDstWeights):
        if transpose:
            raise ValueError("on-the-fly attention weights aggregate over the CSR only")
        _lib.call("gnpde_attn_ref_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
                  _ptr(grouped.col), _ptr(w_csr.cs), _ptr(w_csr.m), _ptr(w_csr.rl), _ptr(w_csr.mr), w_csr.heads,
                  *epi)
    elif isinstance(w_csr, GatWeights):
        if transpose:
            raise ValueError("on-the-fly attention weights aggregate over the CSR only")
        _lib.call("gnpde_attn_gat_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
                  _ptr(grouped.col), _ptr(w_csr.sp), _ptr(w_csr.m), _ptr(w_csr.rl), w_csr.norm_idx, w_csr.heads,
                  w_csr.slope, *epi)
    elif isinstance(w_csr, RefDstSquareplusWeights):
        if transpose:
            raise ValueError("on-the-fly attention weights aggregate over the CSR only")
        _lib.call("gnpde_attn_sp_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
                  _ptr(grouped.col), _ptr(w_csr.pn), _ptr(w_csr.rl), w_csr.heads, *epi)
    else:
        _lib.call("gnpde_spmm_rhs_f32", _ptr(items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
                  _ptr(col), _ptr(w_csr), *epi)
    return None if stage is not None else out.view(shape)


class CompactWeights(object):
    """Grouped-order weights with zeros (the sampled graph of HardAttODEblock training,
    src/block_transformer_hard_attention.py:52-56) compacted inside the plan's items
    (gnpde_compact_items_f32): ``items`` / ``col`` / ``w`` replace the grouped CSR's
    for K1, which then gathers the retained edges only, in the full plan's order and
    hub chunks (the masked full graph's sums: dropped edges added exact zeros).
    ``full`` is the uncompacted grouped-order weights.  Refreshed in place
    (compact_weights(..., out=)), so captured step graphs keep replaying."""

    def __init__(self, grouped, transpose, full, col, w, items):
        self.grouped, self.transpose = grouped, transpose
        self.full, self.col, self.w, self.items = full, col, w, items


def compact_weights(grouped, w_full, transpose, out=None):
    """CompactWeights of grouped-order weights ``w_full`` [nnz] over ``grouped`` (a
    GroupedCSR: the CSR, or the CSC with transpose=True); ``out``: an earlier
    CompactWeights of the same grouped CSR refreshed in place."""
    plan = grouped.plan
    dev = w_full.device
    _require_gpu(w_full, "w_full", torch.float32)
    if out is None:
        out = CompactWeights(grouped, transpose, w_full, torch.empty_like(grouped.col),
                             torch.empty(max(grouped.nnz, 1), dtype=torch.float32, device=dev),
                             torch.empty_like(plan.items))
    elif out.grouped is not grouped or out.transpose != transpose:
        raise ValueError("compact_weights: out belongs to another grouped CSR")
    out.full = w_full
    _lib.call("gnpde_compact_items_f32", _ptr(plan.items), plan.n_items, _ptr(grouped.col), _ptr(w_full),
              _ptr(out.col), _ptr(out.w), _ptr(out.items), _stream(dev))
    return out


# byte offsets of the hub partial stores are 32-bit (buffer addressing, csrc/common.hpp kBufRecords)
_PARTIALS_MAX_BYTES = 0xffffff00


def _partials(plan, C, dev):
    """fp32 scratch of the hub chunk partial sums: n_slots * C floats."""
    if not plan.n_slots:
        return None
    if plan.n_slots * C * 4 >= _PARTIALS_MAX_BYTES:
        raise ValueError("gnpde: %d hub partial slots x %d columns exceed the 4 GiB of 32-bit buffer offsets the "
                         "in-launch hub combine addresses; use a larger chunk (opt['gnpde_chunk'])" % (plan.n_slots, C))
    return torch.empty(plan.n_slots * C, dtype=torch.float32, device=dev)


class RefDstWeights(object):
    """Weights K1 computes on the fly (gnpde_attn_ref_rhs_f32): the fork's
    scaled_dot under destination-grouped softmax, head-mean per edge from the
    node scores cs [R,h] and the CSC statistics m [R,h], rl [R,h] or their
    packed records mr [R, stats_record_floats(h)] fp32 (two heads)."""

    def __init__(self, cs, m, rl, heads, mr=None):
        self.cs, self.m, self.rl, self.heads, self.mr = cs, m, rl, int(heads), mr


class GatWeights(object):
    """Weights K1 computes on the fly (gnpde_attn_gat_rhs_f32): the GAT attention,
    head-mean per edge from the node-score pairs sp [R,2h] fp64 (gat_scores) and the
    statistics m [R,h] fp64, rl [R,h] of the softmax groups (rows for norm_idx 0,
    destinations for norm_idx 1)."""

    def __init__(self, sp, m, rl, heads, slope, norm_idx):
        self.sp, self.m, self.rl = sp, m, rl
        self.heads, self.slope, self.norm_idx = int(heads), float(slope), int(norm_idx)


# head counts gnpde_attn_gat_rhs_f32 is built for (csrc/gat.hip); beyond: weights pass + K1
GAT_FUSED_MAX_HEADS = 8
# The fused GAT K1 is the default only where it measured faster than the weights pass + the
# plain K1 on the G-arxiv benchmark graph (tools/gat_bench.py): up to two heads
# (the two-head instantiation) for either grouping, more heads (the generic one) under
# destination-grouped softmax; more heads under source-grouped softmax measured 1.1 % slower and
# take the weights pass.  GNPDE_GAT_FUSE=1 fuses wherever the library supports it, 0 never.
GAT_FUSE = os.environ.get("GNPDE_GAT_FUSE", "auto")


def gat_fuse_default(heads, norm_idx):
    """Whether ODEFuncAtt asks attn_rhs for the fused GAT K1 (fuse=...)."""
    if GAT_FUSE in ("0", "1"):
        return GAT_FUSE == "1"
    return heads <= 2 or norm_idx == 1


def spmm_rhs_rows(g, plan, w_csr, x_src, x_rows, row0, x0=None, alpha=None, beta=None, alpha_sigmoid=True,
                  add_source=False, stage=None, out=None, col=None, ns=None, mr=None):
    """K1 over a row block: ``plan`` covers rows [row0, row0 + n) by their
    positions in ``x_src`` (the gathered state); gathers read ``x_src`` through
    ``col`` (default: the CSR's global ids; dist.RowPartition passes ids
    relabelled into its padded layout); the block's own state ``x_rows`` [n, C],
    ``x0`` and the outputs are local buffers addressed through pointers shifted
    back by row0 rows (never dereferenced outside the block).  The epilogue's
    x_r comes from x_src[row], which holds the same values.

    Weights: ``w_csr`` in CSR order (plain), a RefDstWeights (the fork's scaled_dot
    under destination-grouped softmax, formed in the gather loop:
    gnpde_attn_ref_rhs_f32), or ``ns`` = per-edge scaled_dot NodeScores over the
    whole state (q, k rows at the positions of x_src; ``mr``: destination
    statistics records for norm_idx 1, None for source-grouped softmax: the fused
    gnpde_attn_dot_rhs_f32)."""
    if isinstance(w_csr, CompactWeights):
        raise ValueError("spmm_rhs_rows: compacted (sampled-graph) weights take the whole-graph K1 (spmm_rhs)")
    xs = _rows(x_src, "x_src")
    xl = _rows(x_rows, "x_rows")
    C = xs.shape[1]
    dev = xs.device
    shift = int(row0) * C * 4
    sp = lambda t: ctypes.c_void_p(t.data_ptr() - shift) if t is not None else ctypes.c_void_p(0)  # noqa: E731
    a = _scalar(alpha, "alpha", dev)
    b = _scalar(beta, "beta", dev) if add_source else None
    x0r = _rows(x0, "x0") if add_source else None
    st = None
    if stage is not None:
        for t in stage.tensors():
            _require_gpu(t, "stage tensor", torch.float32)
        if stage.wide:
            raise ValueError("spmm_rhs_rows: the adaptive solvers' wide stages run unsharded or in column stripes")
        st = ctypes.byref(stage.struct(xs, shift))
    elif out is None:
        out = torch.empty_like(xl)
    cp = _ptr(g.csr.col if col is None else col)
    epi = (C, _ptr(xs), C, sp(x0r), C, _ptr(a), _ptr(b), _flags(True, alpha_sigmoid, add_source),
           sp(out) if out is not None else ctypes.c_void_p(0), C)
    plan.order_launch(dev)
    if ns is not None:
        H, dk = ns.heads, ns.dk
        if not _lib.fn("gnpde_attn_dot_supported")(H, dk, C):
            raise ValueError("spmm_rhs_rows: per-edge scores of heads=%d dk=%d C=%d outside the fused kernel" %
                             (H, dk, C))
        nws = int(_lib.fn("gnpde_attn_dot_workspace_floats")(H, C, plan.n_slots))
        ws = torch.empty(max(nws, 4), dtype=torch.float32, device=dev)
        _lib.call("gnpde_attn_dot_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy, cp,
                  _ptr(ns.q), _ptr(ns.k), ns.ldqk, H, dk, _ptr(mr), *epi, _ptr(ws), plan.n_slots, st, _stream(dev))
    elif isinstance(w_csr, RefDstWeights):
        partials = _partials(plan, C, dev)
        _lib.call("gnpde_attn_ref_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy, cp,
                  _ptr(w_csr.cs), _ptr(w_csr.m), _ptr(w_csr.rl), _ptr(w_csr.mr), w_csr.heads, *epi, _ptr(partials),
                  plan.n_slots, st, _stream(dev))
    else:
        partials = _partials(plan, C, dev)
        _lib.call("gnpde_spmm_rhs_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy, cp,
                  _ptr(w_csr), *epi, _ptr(partials), plan.n_slots, st, _stream(dev))
    return None if stage is not None else out.view(x_rows.shape)


# --------------------------------------------------------------------------- attention
SCORE_MODES = {
    ('scaled_dot', 'reference'): _lib.SCORE_REFERENCE,
    ('scaled_dot', 'per_edge'): _lib.SCORE_DOT,
    ('exp_kernel', 'reference'): _lib.SCORE_EXP_KERNEL,
    ('exp_kernel', 'per_edge'): _lib.SCORE_EXP_KERNEL,
    ('cosine_sim', 'reference'): _lib.SCORE_COSINE,
    ('cosine_sim', 'per_edge'): _lib.SCORE_COSINE,
    ('pearson', 'reference'): _lib.SCORE_PEARSON,
    ('pearson', 'per_edge'): _lib.SCORE_PEARSON,
}


def linear(x, W, bias=None, split=None):
    """MFMA projection: x [R,K] @ W[Nout,K]^T + bias -> (out[:, :split], out[:, split:]).
    x fp32, or bf16 storage (gnpde_linear_bf16: widened exactly on load, so the same
    values and bits as the projection of x.float()); outputs fp32."""
    xdt = x.dtype if isinstance(x, torch.Tensor) and x.dtype in STATE_DTYPES else torch.float32
    xr = _rows(x, "x", xdt)
    _require_gpu(W, "W", torch.float32)
    W = W.contiguous()
    Nout, K = W.shape
    if xr.shape[1] != K:
        raise ValueError("linear: x has %d columns, W expects %d" % (xr.shape[1], K))
    if bias is not None:
        _require_gpu(bias, "bias", torch.float32)
        bias = bias.contiguous()
    split = Nout if split is None else int(split)
    R = xr.shape[0]
    out_a = torch.empty(R, split, dtype=torch.float32, device=xr.device)
    out_b = torch.empty(R, Nout - split, dtype=torch.float32, device=xr.device) if split < Nout else None
    name = "gnpde_linear_bf16" if xdt == torch.bfloat16 else "gnpde_linear_f32"
    _lib.call(name, _ptr(xr), R, K, K, _ptr(W), _ptr(bias), Nout, split, _ptr(out_a), max(split, 1),
              _ptr(out_b), max(Nout - split, 1), _stream(xr.device))
    return out_a, out_b


def linear_wgrad(gy, x):
    """gW = gy^T x [M, K] on the fp32 matrix cores (gnpde_linear_wgrad_f32): the
    weight gradient of the Q / K projections (the backward of nn.Linear,
    function_transformer_attention.py:224-225), rows reduced in a fixed order."""
    gyr = _rows(gy, "gy")
    xr = _rows(x, "x")
    if gyr.shape[0] != xr.shape[0]:
        raise ValueError("linear_wgrad: gy has %d rows, x has %d" % (gyr.shape[0], xr.shape[0]))
    R, M = gyr.shape
    K = xr.shape[1]
    out = torch.empty(M, K, dtype=torch.float32, device=xr.device)
    nb = _lib.fn("gnpde_linear_wgrad_workspace_bytes")(R, M, K)
    ws = torch.empty(nb, dtype=torch.uint8, device=xr.device)
    _lib.call("gnpde_linear_wgrad_f32", _ptr(gyr), R, M, M, _ptr(xr), K, K, _ptr(out), K, _ptr(ws), nb,
              _stream(xr.device))
    return out


def _linear_rhs_fuses(stage):
    """Whether gnpde_linear_rhs_f32 fuses ``stage``: the fixed-grid epilogue (f_out, outputs,
    at most STAGE_PRE_K operands); everything else takes f + stage_apply."""
    return not (stage.wide or stage.dot is not None or stage.dense is not None or stage.scale_rows is not None
                or stage.out_rows is not None or stage.scale is not None or stage.f_lin != 0.0)


def linear_rhs(z, Wt, x, x0=None, alpha=None, beta=None, rhs=True, alpha_sigmoid=True, add_source=False, out=None,
               stage=None, fuse=True, bias=None):
    """f = a*(z Wt^T - x) [+ b*x0] (or z Wt^T with rhs=False): the output product of the
    GAT value projection with the RHS epilogue and the fixed-grid stage combination fused
    (gnpde_linear_rhs_f32).  z [..., K] fp32, Wt [C, K] fp32 (= Wout^T), x / x0 [..., C]
    fp32 with the rows of z.  stage: a ``Stage`` -> its outputs are written instead of f
    (returns None); a stage the kernel does not fuse (Stage.wide, a coefficient scale,
    out_rows, f_lin), or any stage with fuse=False, takes f first and the stage in a second
    pass (stage_apply), as spmm_rhs does for on-the-fly weights — the same bits.
    bias [C] fp32: ax = z Wt^T + bias ahead of the epilogue (gnpde_linear_rhs_bias_f32, the
    transformer layer's Wout); None: gnpde_linear_rhs_f32."""
    if stage is not None and not (fuse and _linear_rhs_fuses(stage)):
        f = linear_rhs(z, Wt, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                       add_source=add_source, bias=bias)
        stage_apply(stage, f, x, x)
        return None
    zr = _rows(z, "z")
    _require_gpu(Wt, "Wt", torch.float32)
    Wt = Wt.contiguous()
    C, K = Wt.shape
    if zr.shape[1] != K:
        raise ValueError("linear_rhs: z has %d columns, Wt expects %d" % (zr.shape[1], K))
    R = zr.shape[0]
    dev = zr.device
    if x is None and (rhs or stage is not None):
        raise ValueError("linear_rhs: x required")
    xr = _rows(x, "x") if x is not None else None
    if xr is not None and tuple(xr.shape) != (R, C):
        raise ValueError("linear_rhs: x is %s, z Wt^T is (%d, %d)" % (tuple(xr.shape), R, C))
    a = _scalar(alpha, "alpha", dev) if rhs else None
    if rhs and a is None:
        raise ValueError("linear_rhs: alpha required")
    b = _scalar(beta, "beta", dev) if add_source else None
    x0r = _rows(x0, "x0") if add_source else None
    if x0r is not None and tuple(x0r.shape) != (R, C):
        raise ValueError("linear_rhs: x0 is %s, z Wt^T is (%d, %d)" % (tuple(x0r.shape), R, C))
    st = None
    if stage is not None:
        for t in stage.tensors():
            _require_gpu(t, "stage tensor", torch.float32)
            if not t.is_contiguous() or t.numel() != R * C:
                raise ValueError("stage tensors must be contiguous and shaped like x")
        st = ctypes.byref(stage.struct(xr))
    elif out is None:
        out = torch.empty(R, C, dtype=torch.float32, device=dev)
    else:
        _require_gpu(out, "out", torch.float32)
        if not out.is_contiguous() or out.numel() != R * C:
            raise ValueError("linear_rhs: out must be contiguous and hold %d x %d" % (R, C))
    if bias is not None:
        _require_gpu(bias, "bias", torch.float32)
        bias = bias.contiguous()
        if bias.numel() != C:
            raise ValueError("linear_rhs: bias has %d elements, z Wt^T has %d columns" % (bias.numel(), C))
        _lib.call("gnpde_linear_rhs_bias_f32", _ptr(zr), R, K, K, _ptr(Wt), C, _ptr(bias), _ptr(xr), C, _ptr(x0r), C,
                  _ptr(a), _ptr(b), _flags(rhs, alpha_sigmoid, add_source), _ptr(out), C, st, _stream(dev))
    else:
        _lib.call("gnpde_linear_rhs_f32", _ptr(zr), R, K, K, _ptr(Wt), C, _ptr(xr), C, _ptr(x0r), C, _ptr(a), _ptr(b),
                  _flags(rhs, alpha_sigmoid, add_source), _ptr(out), C, st, _stream(dev))
    if stage is not None:
        return None
    return out.view(x.shape if x is not None else tuple(z.shape[:-1]) + (C,))


def head_aggregate(g, wh, v, coo=False, out=None):
    """The per-head value aggregation of the transformer layer's mix_features branch
    (gnpde_head_aggregate_f32, csrc/head_aggregate.hip):
      z[r, d] = (1/H) sum_{p in row r} sum_h wh[p, h] * v[col[p], h*dk + d]      [B,N,dk]
    v [B,N,att] (or [R,att]) fp32, head h owning columns h*dk .. h*dk+dk-1; wh the per-head
    edge weights, [nnz, H] in aggregation-CSR order (head_weights), or with coo=True an
    attention [B,E,H] in COO order (the layer's own output, an explicitly given one), which
    the kernel reads through the CSR's perm.
    Work items are K1's plan; no float atomics: repeated launches give the same bits."""
    vr = _rows(v, "v")
    _require_gpu(wh, "per-head weights", torch.float32)
    wh = wh.contiguous()
    H = int(wh.shape[-1])
    att = vr.shape[1]
    if wh.numel() != g.nnz * H or (coo and tuple(wh.shape) != (g.B, g.E, H)):
        raise ValueError("head_aggregate: weights %s do not match %d edges x %d heads" % (tuple(wh.shape), g.nnz, H))
    if H < 1 or att % H:
        raise ValueError("head_aggregate: %d columns of v do not split into %d heads" % (att, H))
    if vr.shape[0] != g.R:
        raise ValueError("v has %d rows, graph has %d" % (vr.shape[0], g.R))
    dk = att // H
    dev = vr.device
    if out is None:
        out = torch.empty(g.R, dk, dtype=torch.float32, device=dev)
    else:
        _require_gpu(out, "out", torch.float32)
        if not out.is_contiguous() or out.numel() != g.R * dk:
            raise ValueError("head_aggregate: out must be contiguous and hold %d x %d" % (g.R, dk))
    plan = g.csr.plan
    nws = int(_lib.fn("gnpde_head_aggregate_workspace_floats")(dk, plan.n_slots))
    if nws * 4 >= _PARTIALS_MAX_BYTES:
        raise ValueError("gnpde: %d hub partial slots x %d columns exceed the 4 GiB of 32-bit buffer offsets the "
                         "in-launch hub combine addresses; use a larger chunk (opt['gnpde_chunk'])"
                         % (plan.n_slots, dk))
    ws = torch.empty(nws, dtype=torch.float32, device=dev) if nws else None
    plan.order_launch(dev)
    _lib.call("gnpde_head_aggregate_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
              _ptr(g.csr.rowptr), _ptr(g.csr.col), _ptr(g.csr.perm if coo else None), g.R, _ptr(wh), H, dk, _ptr(vr),
              att, _ptr(out), dk, _ptr(ws), plan.n_slots, _stream(dev))
    return out.view(tuple(v.shape[:-1]) + (dk,)) if v.dim() == 3 else out.view(g.R, dk)


def head_weights(g, ns, m, rl, norm_idx):
    """The per-head edge weights of head_aggregate for this RHS evaluation, [nnz, H] in
    aggregation-CSR order: the layer's attention pass with a CSR-order output — ScoreArgs::score
    with the group statistics (softmax: gnpde_edge_attention_csr_f32) or the squareplus operands
    (m an ops.SquareplusState: gnpde_squareplus_attention_csr_f32), one pass for every
    attention_type, score mode, grouping and normaliser; the values of edge_attention /
    squareplus_attention, bit for bit, at att[perm[p]].  No head mean is formed.  (Measured
    against head_aggregate reading the COO attention through perm: DESIGN.md §6.16.)"""
    dev = g.csr.col.device
    wh = torch.empty(max(g.nnz, 1), ns.heads, dtype=torch.float32, device=dev)
    if isinstance(m, SquareplusState):
        _sp_check_mode(ns)
        _lib.call("gnpde_squareplus_attention_csr_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz,
                  g.N, int(norm_idx), ns.mode, ns.heads, _ptr(m.pn), _ptr(m.sc), _ptr(m.M), _ptr(rl), _ptr(wh),
                  _stream(dev))
    else:
        _lib.call("gnpde_edge_attention_csr_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), g.nnz, int(norm_idx), ns.mode,
                  ns.heads, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(m), _ptr(rl),
                  _ptr(wh), _stream(dev))
    return wh[:g.nnz]


class NodeScores(object):
    """Per-RHS node-level operands of the attention scores.  GAT (SCORE_GAT): ``sp``
    = the node-score pairs [R, 2h] fp64 = [sl | sr] and ``slope`` the LeakyReLU slope;
    the C ABI takes them in the places of cs and score_p0."""

    def __init__(self, mode, heads, dk, cs=None, q=None, k=None, p0=1.0, p1=1.0, sp=None, slope=None):
        self.mode, self.heads, self.dk = mode, heads, dk
        self.sp, self.slope = sp, (None if slope is None else float(slope))
        if sp is not None:
            cs, p0 = sp, slope
        self.cs, self.q, self.k = cs, q, k
        self.p0, self.p1 = float(p0), float(p1)
        self.ldqk = q.shape[1] if q is not None else 1


def gat_workspace(x, B):
    """Scratch of gat_scores (the folded U): allocate once per parameter version so
    that captured step graphs keep reading the buffer they were captured with."""
    C = x.shape[-1]
    nb = _lib.fn("gnpde_gat_scores_workspace_bytes")(B, C)
    return torch.empty(int(nb), dtype=torch.uint8, device=x.device)


def gat_scores(g, x, W, a, heads, slope, ws=None):
    """GAT node scores (function_GAT_attention.py:123-134 without wx): NodeScores of
    mode SCORE_GAT with sp [R, 2h] fp64 = [sl | sr] = x U, U = W [C, att] folded with
    a [2dk] on the device (gnpde_gat_scores_f32; x read once)."""
    xr = _rows(x, "x")
    _require_gpu(W, "W", torch.float32)
    _require_gpu(a, "a", torch.float32)
    W = W.contiguous()
    a = a.contiguous().view(-1)
    C, att = W.shape
    heads = int(heads)
    if xr.shape[1] != C:
        raise ValueError("gat_scores: x has %d columns, W expects %d" % (xr.shape[1], C))
    if att % heads or a.numel() != 2 * (att // heads):
        raise ValueError("gat_scores: attention_dim %d, heads %d, a of %d elements" % (att, heads, a.numel()))
    if xr.shape[0] != g.R:
        raise ValueError("x has %d rows, graph has %d" % (xr.shape[0], g.R))
    if ws is None:
        ws = gat_workspace(xr, g.B)
    sp = torch.empty(g.R, 2 * heads, dtype=torch.float64, device=xr.device)
    _lib.call("gnpde_gat_scores_f32", _ptr(xr), g.B, g.N, C, C, _ptr(W), _ptr(a), att, heads, _ptr(sp), _ptr(ws),
              ws.numel(), _stream(xr.device))
    return NodeScores(_lib.SCORE_GAT, heads, att // heads, sp=sp, slope=slope)


def gat_score_backward(g, ns, gs):
    """ge [B,E,h] = gs * LeakyReLU'(sl[src] + sr[dst]) (COO order; gnpde_gat_score_backward_f32)."""
    _require_gpu(gs, "score grad", torch.float32)
    gs = gs.contiguous()
    ge = torch.empty_like(gs)
    _lib.call("gnpde_gat_score_backward_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz, ns.heads,
              _ptr(ns.sp), ns.slope, _ptr(gs), _ptr(ge), _stream(gs.device))
    return ge


def _keysum_workspace(g, dev, nbytes):
    """Scratch of gnpde_ref_scores_f32 (tile partials, U and v), held by the graph
    (freed with it) per stream and size, so that captured step graphs
    keep reading the buffer they were captured with and two streams never share one."""
    d = g.__dict__.setdefault('_keysum_ws', {})
    key = (torch.cuda.current_stream(dev).cuda_stream, int(nbytes))
    ws = d.get(key)
    if ws is None:
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
        d[key] = ws
    return ws


def node_scores(g, x, Wq, bq, Wk, bk, heads, attention_type='scaled_dot', score_mode='reference',
                output_var=1.0, lengthscale=1.0, wcat=None):
    """Q/K-side work of SpGraphTransAttentionLayer.forward (function_transformer_attention.py:224-259)."""
    mode = SCORE_MODES[(attention_type, score_mode)]
    # the per-edge modes project a bf16 state directly (gnpde_linear_bf16); the reference
    # mode's key sum and node scores read fp32
    bf = isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 and mode != _lib.SCORE_REFERENCE
    xr = _rows(x, "x", torch.bfloat16 if bf else torch.float32)
    # a given [Wq; Wk] operand decides the width (the beltrami layer folds its four
    # projections into one and has no Wq of its own)
    att = Wq.shape[0] if Wq is not None else wcat[0].shape[0] // 2
    if att % heads:
        raise ValueError("attention_dim %d not divisible by heads %d" % (att, heads))
    dk = att // heads
    if mode == _lib.SCORE_REFERENCE:
        B, N, C = g.B, g.N, xr.shape[1]
        cs = torch.empty(g.R, heads, dtype=torch.float64, device=xr.device)
        ws_bytes = _lib.fn("gnpde_keysum_workspace_bytes")(B, N, C, att)
        ws = _keysum_workspace(g, xr.device, ws_bytes)
        for name, t in (("Wq", Wq), ("bq", bq), ("Wk", Wk), ("bk", bk)):
            _require_gpu(t, name, torch.float32)
        _lib.call("gnpde_ref_scores_f32", _ptr(xr), B, N, C, C, _ptr(g.indeg), _ptr(Wq.contiguous()),
                  _ptr(bq.contiguous()), _ptr(Wk.contiguous()), _ptr(bk.contiguous()), att, heads, _ptr(cs), _ptr(ws),
                  ws_bytes, _stream(xr.device))
        return NodeScores(mode, heads, dk, cs=cs)
    if wcat is not None:
        W, b = wcat
    else:
        W = torch.cat([Wq, Wk], 0)
        b = torch.cat([bq, bk], 0) if bq is not None else None
    q, k = linear(xr, W, b, split=att)
    return NodeScores(mode, heads, dk, q=q, k=k, p0=output_var, p1=lengthscale)


def ref_keysum(g, x, Wk, bk):
    """The fork's global key sum S [B, att] fp64 of a (column stripe of the) state:
    S_b = Wk xbar_b + (sum indeg) bk with xbar_b = sum_n indeg(n) x_n
    (gnpde_ref_keysum_f32; function_transformer_attention.py:249's
    sum over e' of k_dst(e')).  Linear in x's columns: the shares of the stripes of
    a state sum to the key sum of the whole (bk on one stripe only)."""
    xr = _rows(x, "x")
    C = xr.shape[1]
    att = Wk.shape[0]
    for name, t in (("Wk", Wk), ("bk", bk)):
        _require_gpu(t, name, torch.float32)
    S = torch.empty(g.B, att, dtype=torch.float64, device=xr.device)
    nb = _lib.fn("gnpde_keysum_workspace_bytes")(g.B, g.N, C, att)
    ws = _keysum_workspace(g, xr.device, nb)
    _lib.call("gnpde_ref_keysum_f32", _ptr(xr), g.B, g.N, C, C, _ptr(g.indeg), _ptr(Wk.contiguous()),
              _ptr(bk.contiguous()), att, _ptr(S), _ptr(ws), nb, _stream(xr.device))
    return S


def ref_scores_from_keysum(g, x, S, Wq, bq, heads):
    """Node scores cs [R, heads] fp64 = q . S / sqrt(dk) of a (column stripe of the)
    state from a given key sum S (gnpde_ref_scores_from_keysum_f32): the stripe's
    share of cs (bq on one stripe only)."""
    xr = _rows(x, "x")
    C = xr.shape[1]
    att = Wq.shape[0]
    _require_gpu(S, "S", torch.float64)
    for name, t in (("Wq", Wq), ("bq", bq)):
        _require_gpu(t, name, torch.float32)
    cs = torch.empty(g.R, heads, dtype=torch.float64, device=xr.device)
    nb = _lib.fn("gnpde_keysum_workspace_bytes")(g.B, g.N, C, att)
    ws = _keysum_workspace(g, xr.device, nb)
    _lib.call("gnpde_ref_scores_from_keysum_f32", _ptr(xr), g.B, g.N, C, C, _ptr(S.contiguous()),
              _ptr(Wq.contiguous()), _ptr(bq.contiguous()), att, heads, _ptr(cs), _ptr(ws), nb, _stream(xr.device))
    return cs


def uniform_scores(heads):
    """Source-grouped softmax of the fork's scaled_dot: every score of a source
    row is q_i . S / sqrt(dk), identical within the group, so softmax gives
    exp(0)/(outdeg + 1e-16) whatever x, Q and K are.  The
    weights depend on the graph only and are computed once per graph."""
    return NodeScores(_lib.SCORE_UNIFORM, heads, 1)


def stats_record_floats(heads):
    """Floats per packed statistics record (include/gnpde.h GNPDE_STATS_RECORD_FLOATS)."""
    return (2 * heads + 3) & ~3


def _seg_call(g, ns, norm_idx, out_kind, packed=False, rows=None):
    """K2 (gnpde_seg_softmax_f32) over the grouped CSR of the softmax groups:
    out_kind 0 -> head-mean weights in aggregation-CSR order (norm_idx 0 only);
    1 -> (m, rl), or with packed=True (None, None, mr): the packed statistics
    records only.  NotImplemented when the shape is outside the kernel."""
    gat = ns.mode == _lib.SCORE_GAT  # statistics of either grouping; weights from them (attn_weights / K1)
    if ns.mode == _lib.SCORE_UNIFORM or ((ns.mode == _lib.SCORE_REFERENCE or gat) and out_kind == 0):
        return NotImplemented
    eb = _lib.fn("gnpde_seg_block_edges")(ns.mode, ns.heads, ns.dk)
    if eb <= 0:
        return NotImplemented
    if ns.q is not None and (ns.ldqk % 4 or ns.q.data_ptr() % 16 or ns.k.data_ptr() % 16):
        return NotImplemented
    grouped = g.csr if norm_idx == 0 else g.csc
    long_items = (ns.mode == _lib.SCORE_REFERENCE and out_kind == 1 and norm_idx == 1) or gat
    # a small graph's statistics launch is one round of items: every long item one pass
    # (its hub groups in one-pass chunks), so no wavefront walks a group alone
    long_max = int(_lib.fn("gnpde_seg_long_pass_edges")(ns.heads)) if (long_items and g.R < SMALL_GRAPH_ROWS and
                                                                        SEG_LONG_SPLIT) else None
    if rows is not None:  # the groups of rows [r0, r1) only (outputs: full-size, those rows written)
        if out_kind != 1:
            return NotImplemented
        if rows[1] <= rows[0]:  # an empty block (a rank with no groups): nothing to form
            dev, H = grouped.col.device, ns.heads
            if packed:
                return None, None, torch.zeros(g.R, stats_record_floats(H), dtype=torch.float32, device=dev)
            return (torch.zeros(g.R, H, dtype=torch.float64, device=dev),
                    torch.zeros(g.R, H, dtype=torch.float32, device=dev))
        plan = grouped.seg_plan_rows(rows[0], rows[1], eb, long_items=long_items, long_max=long_max)
    else:
        plan = grouped.seg_plan(eb, long_items=long_items, long_max=long_max)
    dev = grouped.col.device
    H = ns.heads
    packed = packed and out_kind == 1
    need_stats = not packed and (out_kind == 1 or plan.n_chunk > 0)
    m = torch.empty(g.R, H, dtype=torch.float64, device=dev) if need_stats else None
    rl = torch.empty(g.R, H, dtype=torch.float32, device=dev) if need_stats else None
    mr = torch.empty(g.R, stats_record_floats(H), dtype=torch.float32, device=dev) if packed else None
    partials = torch.empty(plan.n_slots * 2 * H, dtype=torch.float64, device=dev) if plan.n_slots else None
    w = torch.empty(max(g.nnz, 1), dtype=torch.float32, device=dev) if out_kind == 0 else None
    plan.order_launch(dev)  # chunked plans' statistics fixups read partials written by this launch
    rc = _lib.call_rc("gnpde_seg_softmax_f32", _ptr(plan.items), plan.n_items, plan.n_hub, plan.n_long,
                      _ptr(plan.chunk_items), plan.n_chunk,
                      _ptr(plan.heavy), plan.n_heavy, _ptr(grouped.rowptr), _ptr(grouped.rowidx), _ptr(grouped.col),
                      int(norm_idx == 1), out_kind, ns.mode, H, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk,
                      ns.p0, ns.p1, _ptr(w), _ptr(m), _ptr(rl), _ptr(mr), _ptr(partials), _stream(dev))
    if rc == _lib.EUNSUPPORTED:
        return NotImplemented
    _lib.check(rc, "gnpde_seg_softmax_f32")
    if out_kind == 0:
        return w
    return (None, None, mr) if packed else (m, rl)


def softmax_stats(g, ns, norm_idx, seg=True, packed=False, rows=None):
    """m [R,h] fp64, rl [R,h]: per-group max and 1/(sum-exp + 1e-16)
    (utils.softmax, src/utils.py:116-127).  seg=True: the edge-block kernel K2;
    shapes outside it (and seg=False) use the per-group kernels
    (gnpde_softmax_stats_f32).  packed=True returns (None, None, mr): the same
    statistics as packed records [R, stats_record_floats(h)] fp32 only (the form
    the fused-weight K1 reads in one cache line per edge).  rows=(r0, r1): only
    the groups [r0, r1) are formed (K2; full-size outputs with those rows written,
    the same values as the full launch) — NotImplemented outside K2's shapes."""
    if rows is not None:
        return _seg_call(g, ns, norm_idx, 1, packed=packed, rows=rows) if seg else NotImplemented
    if seg:
        r = _seg_call(g, ns, norm_idx, 1, packed=packed)
        if r is not NotImplemented:
            return r
    grouped = g.csr if norm_idx == 0 else g.csc
    plan = grouped.stats_plan
    dev = grouped.col.device
    H = ns.heads
    m = None if packed else torch.empty(g.R, H, dtype=torch.float64, device=dev)
    rl = None if packed else torch.empty(g.R, H, dtype=torch.float32, device=dev)
    mr = torch.empty(g.R, stats_record_floats(H), dtype=torch.float32, device=dev) if packed else None
    partials = torch.empty(plan.n_slots * 2 * H, dtype=torch.float64, device=dev) if plan.n_slots else None
    _lib.call("gnpde_softmax_stats_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
              _ptr(grouped.col), int(norm_idx == 1), ns.mode, H, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk,
              ns.p0, ns.p1, _ptr(m), _ptr(rl), _ptr(mr), _ptr(partials), _stream(dev))
    return (None, None, mr) if packed else (m, rl)


def attn_weights(g, ns, m, rl, norm_idx, seg=True, edges=None):
    """Head-mean softmax weights in aggregation-CSR order [nnz].  norm_idx 0:
    K2 computes them straight from the scores (m, rl unused, may be None);
    norm_idx 1 (and shapes outside K2): edge-parallel from the group
    statistics (gnpde_attn_weights_f32).  edges=(e0, e1): only the CSR
    positions [e0, e1), edge-parallel from the given m, rl ([e1 - e0] weights,
    the same values as the full pass: gnpde.dist's edge-sharded weights)."""
    dev = g.csr.col.device
    if edges is not None:
        e0, e1 = (int(v) for v in edges)
        if m is None or rl is None or not 0 <= e0 <= e1 <= g.nnz:
            raise ValueError("attn_weights: edges needs the statistics m, rl and 0 <= e0 <= e1 <= nnz")
        w = torch.empty(max(e1 - e0, 1), dtype=torch.float32, device=dev)
        if e1 > e0:
            _lib.call("gnpde_attn_weights_f32", _ptr(g.csr.rowidx[e0:e1]), _ptr(g.csr.col[e0:e1]), e1 - e0,
                      int(norm_idx), ns.mode, ns.heads, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0,
                      ns.p1, _ptr(m), _ptr(rl), _ptr(w), _stream(dev))
        return w[:e1 - e0]
    if seg and norm_idx == 0:
        w = _seg_call(g, ns, 0, 0)
        if w is not NotImplemented:
            return w
    if m is None:
        m, rl = softmax_stats(g, ns, norm_idx, seg=seg)
    w = torch.empty(max(g.nnz, 1), dtype=torch.float32, device=dev)
    _lib.call("gnpde_attn_weights_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), g.nnz, int(norm_idx), ns.mode, ns.heads,
              ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(m), _ptr(rl), _ptr(w),
              _stream(dev))
    return w


# Small graphs (SMALL_GRAPH_ROWS): the fork's scaled_dot weights under destination-grouped
# softmax as a separate edge-parallel pass (gnpde_attn_weights_f32, every edge at once)
# instead of in K1's gather loop, whose chain per edge (the destination's statistics, one
# exp per head) is the launch's critical path there.  "wide": for the adaptive solvers'
# wide stages only (then K1 fuses the stage: no stage pass); "all"; "none".
SMALL_PRECOMPUTE = os.environ.get("GNPDE_SMALL_PRECOMPUTE", "wide")


# Any graph: the adaptive solvers' wide stages take the weights pass too, so the plain-weight
# K1 fuses the stage (STG 4) instead of forming f and applying the stage in a second pass
# over f and its operands (gnpde_stage_apply_f32) — GNPDE_WIDE_PRECOMPUTE=0: the pass.
WIDE_PRECOMPUTE = os.environ.get("GNPDE_WIDE_PRECOMPUTE", "1") != "0"


def _small_precompute(g, stage):
    if WIDE_PRECOMPUTE and stage is not None and stage.wide:
        return True
    if g.R >= SMALL_GRAPH_ROWS or SMALL_PRECOMPUTE == "none":
        return False
    return SMALL_PRECOMPUTE == "all" or (stage is not None and stage.wide)


def attn_rhs(g, ns, m, rl, norm_idx, x, x0=None, alpha=None, beta=None, rhs=True, alpha_sigmoid=True,
             add_source=False, out=None, stage=None, seg=True, fuse=True, mr=None):
    """K2 + K1: f = a*(A_att x - x) [+ b x0], A_att = head-mean softmax weights
    (m, rl: destination statistics for norm_idx 1, or None to compute them;
    mr: the same statistics as packed records, softmax_stats(packed=True)).
    Reference scores under norm_idx 1 (fuse=True): the weights are computed
    inside K1 from (cs, m, rl) or (cs, mr) — same bits as the separate weights
    pass.  Two heads with no statistics given: the packed records.  Per-edge
    scaled_dot (fuse=True, shapes of gnpde_attn_dot_supported): one fused pass
    (attn_dot_rhs) for either grouping.  GAT scores (fuse=True, an fp32 state): the
    weights inside K1 from (sp, m, rl) of either grouping (gnpde_attn_gat_rhs_f32) —
    same bits as the weights pass + K1 (ODEFuncAtt passes fuse=gat_fuse_default(...): where
    the fused pass measured faster)."""
    if fuse and norm_idx == 1 and ns.mode == _lib.SCORE_REFERENCE and x.dtype == torch.float32 and \
            not _small_precompute(g, stage):
        if m is None and mr is None:
            if ns.heads == 2:
                _, _, mr = softmax_stats(g, ns, 1, seg=seg, packed=True)
            else:
                m, rl = softmax_stats(g, ns, 1, seg=seg)
        w = RefDstWeights(ns.cs, m, rl, ns.heads, mr=mr)
        return spmm_rhs(g, w, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                        add_source=add_source, out=out, stage=stage)
    if fuse and ns.mode == _lib.SCORE_GAT and x.dtype == torch.float32 and ns.heads <= GAT_FUSED_MAX_HEADS and \
            not _small_precompute(g, stage):
        if m is None:
            m, rl = softmax_stats(g, ns, norm_idx, seg=seg)
        w = GatWeights(ns.sp, m, rl, ns.heads, ns.slope, norm_idx)
        return spmm_rhs(g, w, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                        add_source=add_source, out=out, stage=stage)
    if fuse and ns.mode == _lib.SCORE_DOT and (x.dtype == torch.float32 or (x.dtype == torch.bfloat16 and
                                                                              norm_idx == 0)) and \
            _lib.fn("gnpde_attn_dot_supported")(ns.heads, ns.dk, x.shape[-1]):
        if norm_idx == 1 and mr is None:
            _, _, mr = softmax_stats(g, ns, 1, seg=seg, packed=True)
        r = attn_dot_rhs(g, ns, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                         add_source=add_source, out=out, stage=stage, mr=mr if norm_idx == 1 else None)
        if r is not NotImplemented:
            return r
    w = attn_weights(g, ns, m, rl, norm_idx, seg=seg)
    return spmm_rhs(g, w, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                    add_source=add_source, out=out, stage=stage)


def attn_dot_rhs(g, ns, x, x0=None, alpha=None, beta=None, rhs=True, alpha_sigmoid=True, add_source=False,
                 out=None, stage=None, mr=None):
    """The per-edge scaled_dot RHS in one aggregation pass (gnpde_attn_dot_rhs_f32,
    csrc/flash.hip): under source-grouped softmax (norm_idx 0; mr None) the pass
    forms each row's softmax statistics itself; under destination-grouped softmax
    (norm_idx 1) ``mr`` holds the destinations' packed statistics records
    (softmax_stats(..., packed=True)) and the pass weights every scored edge with
    them.  No [nnz] weights.  NotImplemented for shapes outside the fused kernel
    (gnpde_attn_dot_supported)."""
    dt = x.dtype if isinstance(x, torch.Tensor) and x.dtype in STATE_DTYPES else torch.float32
    bf = dt == torch.bfloat16
    xr = _rows(x, "x", dt)
    C = xr.shape[1]
    H, dk = ns.heads, ns.dk
    if not _lib.fn("gnpde_attn_dot_supported")(H, dk, C):
        return NotImplemented
    if stage is not None and (stage.wide or len(stage.outs) > 1 or stage.dot is not None):
        return NotImplemented  # fused here: single-output fixed-grid stages (the caller takes K2 + K1)
    if bf and mr is not None:
        return NotImplemented  # a bf16 state: source-grouped softmax only (K2 + the bf16 K1 otherwise)
    row_align = 8 if bf else 16
    if ns.ldqk % 4 or ns.q.data_ptr() % 16 or ns.k.data_ptr() % 16 or xr.data_ptr() % row_align:
        return NotImplemented
    if xr.shape[0] != g.R:
        raise ValueError("x has %d rows, graph has %d" % (xr.shape[0], g.R))
    dev = xr.device
    a = _scalar(alpha, "alpha", dev) if rhs else None
    if rhs and a is None:
        raise ValueError("attn_dot_rhs: alpha required")
    b = _scalar(beta, "beta", dev) if add_source else None
    x0r = _rows(x0, "x0", dt) if add_source else None
    if x0r is not None and x0r.data_ptr() % row_align:
        return NotImplemented
    st = None
    if stage is not None:
        for t in stage.tensors():
            _require_gpu(t, "stage tensor", dt)
            if not t.is_contiguous() or t.numel() != xr.numel():
                raise ValueError("stage tensors must be contiguous and shaped like x")
        st = ctypes.byref(stage.struct(xr))
    elif out is None:
        out = torch.empty_like(xr)
    plan = g.csr.plan
    nws = int(_lib.fn("gnpde_attn_dot_workspace_floats")(H, C, plan.n_slots))
    ws = None
    if nws:
        if nws * 4 >= _PARTIALS_MAX_BYTES:
            return NotImplemented
        ws = torch.empty(nws, dtype=torch.float32, device=dev)
    plan.order_launch(dev)
    rc = _lib.call_rc("gnpde_attn_dot_rhs_bf16" if bf else "gnpde_attn_dot_rhs_f32", _ptr(plan.items), plan.n_items,
                      _ptr(plan.heavy), plan.n_heavy,
                      _ptr(g.csr.col), _ptr(ns.q), _ptr(ns.k), ns.ldqk, H, dk, _ptr(mr), C, _ptr(xr), C,
                      _ptr(x0r), C, _ptr(a), _ptr(b), _flags(rhs, alpha_sigmoid, add_source), _ptr(out), C, _ptr(ws),
                      plan.n_slots, st, _stream(dev))
    if rc == _lib.EUNSUPPORTED:
        return NotImplemented
    _lib.check(rc, "gnpde_attn_dot_rhs_f32")
    return None if stage is not None else out.view(x.shape)


def edge_attention(g, ns, m, rl, norm_idx):
    """attention [B,E,h] in COO order (SpGraphTransAttentionLayer.forward's first output)."""
    dev = g.csr.col.device
    att = torch.empty(g.B, g.E, ns.heads, dtype=torch.float32, device=dev)
    _lib.call("gnpde_edge_attention_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz, int(norm_idx),
              ns.mode, ns.heads, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(m), _ptr(rl),
              _ptr(att), _stream(dev))
    return att


# --------------------------------------------------------------------------- squareplus normalisation
# opt['square_plus'] (src/utils.py:129-140): p = squareplus(s - M_b), M_b the maximum over ALL edges
# and heads of batch element b, normalised per group.  csrc/squareplus.hip; DESIGN.md §6.12.
class SquareplusState(object):
    """Per-RHS device operands of the squareplus normaliser: ``M`` [B] fp64 (the global
    score maximum per batch element), ``amax`` [B] int64 (its first COO position, for the
    backward), and the values the later passes read: ``pn`` [R,h] fp32 = p per node
    (reference scores; written by squareplus_stats) or ``sc`` [nnz,h] fp32 = the stored
    per-edge scores in COO order.  ``ws``: the reduction's scratch.  Built by
    squareplus_buffers; a layer keeps one per state shape so that captured step graphs keep
    reading the buffers they were captured with and nothing is read on the host."""

    def __init__(self, M, amax, pn, sc, ws):
        self.M, self.amax, self.pn, self.sc, self.ws = M, amax, pn, sc, ws

    def tensors(self):
        return [t for t in (self.M, self.amax, self.pn, self.sc, self.ws) if t is not None]


class RefDstSquareplusWeights(object):
    """Weights K1 computes on the fly (gnpde_attn_sp_rhs_f32): the fork's scaled_dot under
    destination-grouped squareplus, head-mean per edge from pn [R,h] and rl [R,h]."""

    def __init__(self, pn, rl, heads):
        self.pn, self.rl, self.heads = pn, rl, int(heads)


# The fused squareplus K1 (reference scores, norm_idx 1, fp32 state) against the weights pass +
# the plain K1: the default is the variant that measured faster on the G-arxiv benchmark graph
# (tools/squareplus_bench.py, profiles/squareplus_rhs_bench.json, DESIGN.md §6.12: 0.1647 ms fused
# against 0.1693 per RHS, two heads, C = 128).  GNPDE_SQUAREPLUS_FUSE=1 / 0 forces either.
SQUAREPLUS_FUSE = os.environ.get("GNPDE_SQUAREPLUS_FUSE", "auto")


def squareplus_fuse_default():
    if SQUAREPLUS_FUSE in ("0", "1"):
        return SQUAREPLUS_FUSE == "1"
    return True


def _sp_check_mode(ns):
    if ns.mode in (_lib.SCORE_UNIFORM, _lib.SCORE_GAT):
        raise ValueError("squareplus: score mode %d is not supported (uniform scores keep the cached 1/outdeg "
                         "weights; the GAT layer is softmax only)" % ns.mode)


def squareplus_buffers(g, mode, heads, dev):
    """A SquareplusState with buffers for graph ``g`` and score mode ``mode``."""
    B = g.B
    M = torch.empty(B, dtype=torch.float64, device=dev)
    amax = torch.empty(B, dtype=torch.int64, device=dev)
    ws = torch.empty(int(_lib.fn("gnpde_score_max_workspace_bytes")(B)), dtype=torch.uint8, device=dev)
    pn = sc = None
    if mode == _lib.SCORE_REFERENCE:
        pn = torch.empty(g.R, heads, dtype=torch.float32, device=dev)
    else:
        sc = torch.empty(max(g.nnz, 1), heads, dtype=torch.float32, device=dev)
    return SquareplusState(M, amax, pn, sc, ws)


def score_max(g, ns, bufs=None):
    """The squareplus shift: M [B] fp64 = the maximum score over all edges and heads of each
    batch element, with its first position (gnpde_score_max_f32; workgroup partials + a
    final pass, no atomics).  Reference scores: the maximum of the node scores over the rows
    with an out-edge.  Per-edge modes: one edge pass that also stores the scores.  Returns the
    SquareplusState (``bufs`` filled in place, or a new one)."""
    _sp_check_mode(ns)
    dev = g.csr.col.device
    sq = bufs if bufs is not None else squareplus_buffers(g, ns.mode, ns.heads, dev)
    csr = g.csr
    _lib.call("gnpde_score_max_f32", _ptr(csr.rowptr), _ptr(csr.rowidx), _ptr(csr.col), _ptr(csr.perm), g.B, g.N, g.E,
              ns.mode, ns.heads, ns.dk, _ptr(ns.cs), _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(sq.M),
              _ptr(sq.amax), _ptr(sq.sc), _ptr(sq.ws), sq.ws.numel(), _stream(dev))
    return sq


def squareplus_stats(g, ns, sq, norm_idx):
    """rl [R,h] = 1 / (sum of p over the group + 1e-16), groups = the CSR's rows (norm_idx 0)
    or the CSC's (norm_idx 1), over the grouped CSR's statistics plan (hub groups in chunks
    merged in a fixed order).  Reference scores: also writes sq.pn."""
    _sp_check_mode(ns)
    grouped = g.csr if norm_idx == 0 else g.csc
    plan = grouped.stats_plan
    dev = grouped.col.device
    H = ns.heads
    rl = torch.empty(g.R, H, dtype=torch.float32, device=dev)
    partials = torch.empty(plan.n_slots * H, dtype=torch.float64, device=dev) if plan.n_slots else None
    _lib.call("gnpde_squareplus_stats_f32", _ptr(plan.items), plan.n_items, _ptr(plan.heavy), plan.n_heavy,
              _ptr(grouped.col), _ptr(grouped.perm), int(norm_idx == 1), g.R, g.N, ns.mode, H, _ptr(ns.cs),
              _ptr(sq.sc), _ptr(sq.M), _ptr(sq.pn), _ptr(rl), _ptr(partials), _stream(dev))
    return rl


def squareplus_weights(g, ns, sq, rl, norm_idx):
    """Head-mean squareplus weights in aggregation-CSR order [nnz] (gnpde_squareplus_weights_f32)."""
    _sp_check_mode(ns)
    dev = g.csr.col.device
    w = torch.empty(max(g.nnz, 1), dtype=torch.float32, device=dev)
    _lib.call("gnpde_squareplus_weights_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz, g.N,
              int(norm_idx), ns.mode, ns.heads, _ptr(sq.pn), _ptr(sq.sc), _ptr(sq.M), _ptr(rl), _ptr(w), _stream(dev))
    return w


def squareplus_attention(g, ns, sq, rl, norm_idx):
    """attention [B,E,h] in COO order under squareplus (gnpde_squareplus_attention_f32)."""
    _sp_check_mode(ns)
    dev = g.csr.col.device
    att = torch.empty(g.B, g.E, ns.heads, dtype=torch.float32, device=dev)
    _lib.call("gnpde_squareplus_attention_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz, g.N,
              int(norm_idx), ns.mode, ns.heads, _ptr(sq.pn), _ptr(sq.sc), _ptr(sq.M), _ptr(rl), _ptr(att),
              _stream(dev))
    return att


def squareplus_backward(grouped, att, g_att, rl, amax):
    """dL/ds [B,E,H] (COO, the layout of softmax_backward) of the squareplus normalisation
    over the groups of ``grouped`` from the saved attention, rl and the arg-max positions
    amax [B] of the forward: the group term and the max term (gnpde_squareplus_backward_f32)."""
    _require_gpu(att, "attention", torch.float32)
    _require_gpu(g_att, "attention grad", torch.float32)
    _require_gpu(rl, "rl", torch.float32)
    _require_gpu(amax, "amax", torch.int64)
    att, g_att = att.contiguous(), g_att.contiguous()
    B, H = att.shape[0], att.shape[-1]
    gs = torch.empty_like(att)
    nb = int(_lib.fn("gnpde_squareplus_backward_workspace_bytes")(B))
    ws = torch.empty(nb, dtype=torch.uint8, device=att.device)
    _lib.call("gnpde_squareplus_backward_f32", _ptr(grouped.rowptr), _ptr(grouped.perm), grouped.R, grouped.nnz, B, H,
              _ptr(att), _ptr(g_att), _ptr(rl), _ptr(amax), _ptr(gs), _ptr(ws), nb, _stream(att.device))
    return gs


def squareplus_rhs(g, ns, norm_idx, x, x0=None, alpha=None, beta=None, rhs=True, alpha_sigmoid=True,
                   add_source=False, out=None, stage=None, fuse=None, bufs=None):
    """f = a*(A_att x - x) [+ b x0] with A_att the head-mean squareplus weights: the score
    maximum, the group statistics, then — reference scores under norm_idx 1 with an fp32
    state (fuse, default squareplus_fuse_default()) — K1 forming the weights in its gather
    loop (gnpde_attn_sp_rhs_f32; the same bits as the separate pass), or the weights pass +
    the plain K1 (per-edge modes, a bf16 state, the adaptive solvers' wide stages and small
    graphs under the rules of _small_precompute).  No host read."""
    sq = score_max(g, ns, bufs)
    rl = squareplus_stats(g, ns, sq, norm_idx)
    if fuse is None:
        fuse = squareplus_fuse_default()
    if fuse and norm_idx == 1 and ns.mode == _lib.SCORE_REFERENCE and x.dtype == torch.float32 and \
            not _small_precompute(g, stage):
        w = RefDstSquareplusWeights(sq.pn, rl, ns.heads)
    else:
        w = squareplus_weights(g, ns, sq, rl, norm_idx)
    return spmm_rhs(g, w, x, x0=x0, alpha=alpha, beta=beta, rhs=rhs, alpha_sigmoid=alpha_sigmoid,
                    add_source=add_source, out=out, stage=stage)


# --------------------------------------------------------------------------- backward passes
def sddmm(g, gf, x, heads=1, alpha=None, alpha_sigmoid=False):
    """d <gf, a (A(w) x)> / d w in COO order: [B,E] (heads=1) or [B,E,heads]
    (w = the head mean of an [B,E,heads] attention): a <gf[src], x[dst]> / heads."""
    gfr = _rows(gf, "gf")
    xr = _rows(x, "x")
    C = xr.shape[1]
    dev = xr.device
    a = _scalar(alpha, "alpha", dev)
    shape = (g.B, g.E) if heads == 1 else (g.B, g.E, heads)
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    _lib.call("gnpde_sddmm_f32", _ptr(g.csr.rowidx), _ptr(g.csr.col), _ptr(g.csr.perm), g.nnz, C, _ptr(gfr), C,
              _ptr(xr), C, _ptr(a), int(alpha_sigmoid), int(heads), _ptr(out), _stream(dev))
    return out


def softmax_backward(grouped, att, g_att):
    """Edge-softmax backward over the groups of ``grouped`` (COO [B,E,H] in and out)."""
    _require_gpu(att, "attention", torch.float32)
    _require_gpu(g_att, "attention grad", torch.float32)
    att, g_att = att.contiguous(), g_att.contiguous()
    H = att.shape[-1]
    gs = torch.empty_like(att)
    _lib.call("gnpde_softmax_backward_f32", _ptr(grouped.rowptr), _ptr(grouped.perm), grouped.R, grouped.nnz, H,
              _ptr(att), _ptr(g_att), _ptr(gs), _stream(att.device))
    return gs


def segment_sum(grouped, vals):
    """[R,H] fp64 sums of COO per-edge values [B,E,H] over the rows of ``grouped``."""
    _require_gpu(vals, "values", torch.float32)
    vals = vals.contiguous()
    H = vals.shape[-1]
    out = torch.empty(grouped.R, H, dtype=torch.float64, device=vals.device)
    _lib.call("gnpde_segment_sum_f64", _ptr(grouped.rowptr), _ptr(grouped.perm), grouped.R, grouped.nnz, H,
              _ptr(vals), _ptr(out), _stream(vals.device))
    return out


def dot(a, b, out=None):
    """<a, b> of two fp32 device tensors of the same size, accumulated in fp64
    (gnpde_dot_f64, fixed order): 0-d float64 tensor on the device (``out``: a
    one-element fp64 device tensor, e.g. a slot of a record, written in place)."""
    _require_gpu(a, "a", torch.float32)
    _require_gpu(b, "b", torch.float32)
    if a.numel() != b.numel():
        raise ValueError("dot: sizes differ (%d, %d)" % (a.numel(), b.numel()))
    a, b = a.contiguous(), b.contiguous()
    if out is None:
        out = torch.empty((), dtype=torch.float64, device=a.device)
    else:
        _require_gpu(out, "dot out", torch.float64)
        if out.numel() != 1:
            raise ValueError("dot: out must hold one fp64")
    nbytes = _lib.fn("gnpde_dot_workspace_bytes")()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    _lib.call("gnpde_dot_f64", a.numel(), _ptr(a), _ptr(b), _ptr(out), _ptr(ws), nbytes, _stream(a.device))
    return out


def sum_f64(v, out=None, accumulate=False):
    """sum of an fp64 device vector (gnpde_sum_f64, fixed order) into a 0-d fp64
    tensor (added to ``out`` with accumulate=True)."""
    _require_gpu(v, "v", torch.float64)
    v = v.contiguous()
    if out is None:
        out = torch.zeros((), dtype=torch.float64, device=v.device)
    nbytes = _lib.fn("gnpde_dot_workspace_bytes")()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=v.device)
    _lib.call("gnpde_sum_f64", v.numel(), _ptr(v), _ptr(out), int(bool(accumulate)), _ptr(ws), nbytes,
              _stream(v.device))
    return out


def scaled_sq_sums(y0, f0, f1, atol, rtol, out):
    """The squared sums of the initial-step selection for one component of a mixed
    norm (gnpde_scaled_sq_sums_f32): f1 None -> out[0] = sum (y0/sc)^2, out[1] =
    sum (f0/sc)^2; else out[0] = sum ((f1 - f0)/sc)^2; sc = atol + |y0| rtol.
    out: fp64 device [2] (a view is fine)."""
    for t in (y0, f0) + ((f1,) if f1 is not None else ()):
        _require_gpu(t, "scaled_sq_sums operand", torch.float32)
        if not t.is_contiguous() or t.numel() != y0.numel():
            raise ValueError("scaled_sq_sums: operands must be contiguous and shaped alike")
    _require_gpu(out, "scaled_sq_sums out", torch.float64)
    if out.numel() < 2 or not out.is_contiguous():
        raise ValueError("scaled_sq_sums: out needs 2 contiguous doubles")
    nbytes = _lib.fn("gnpde_initial_step_workspace_bytes")()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=y0.device)
    _lib.call("gnpde_scaled_sq_sums_f32", y0.numel(), _ptr(y0), _ptr(f0), _ptr(f1), float(atol), float(rtol),
              _ptr(out), _ptr(ws), nbytes, _stream(y0.device))


def segment_sums(v, out):
    """out[s] = sum of row s of the fp64 device matrix v [nseg, len] (gnpde_segment_sums_f64,
    fixed order per segment): several epilogue row channels reduced in one pass."""
    _require_gpu(v, "segment_sums v", torch.float64)
    _require_gpu(out, "segment_sums out", torch.float64)
    if v.dim() != 2 or not v.is_contiguous():
        raise ValueError("segment_sums: v must be a contiguous [nseg, len] matrix")
    if out.numel() < v.shape[0] or not out.is_contiguous():
        raise ValueError("segment_sums: out needs nseg contiguous doubles")
    nbytes = _lib.fn("gnpde_segment_sums_workspace_bytes")(v.shape[0])
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=v.device)
    _lib.call("gnpde_segment_sums_f64", v.shape[0], v.shape[1], _ptr(v), _ptr(out), _ptr(ws), nbytes,
              _stream(v.device))


def initial_step(y0, f0, f1, atol, rtol, order, h, hf=None, ws=None):
    """torchdiffeq's _select_initial_step on the device (gnpde_initial_step_*):
    phase 0 (f1 None) writes h[0] = h0, h[1] = d1 and hf = float(h0); phase 1
    (f1 = f(y0 + h0 f0)) writes h[2] = the first step.  h: fp64 [3], hf: fp32 0-d."""
    dt = y0.dtype
    if dt not in STATE_DTYPES:
        raise TypeError("initial_step: state dtype %s" % dt)
    for t in (y0, f0) + ((f1,) if f1 is not None else ()):
        _require_gpu(t, "initial_step state", dt)
        if not t.is_contiguous() or t.numel() != y0.numel():
            raise ValueError("initial_step: y0, f0, f1 must be contiguous and shaped alike")
    _require_gpu(h, "h", torch.float64)
    if h.numel() < 3 or (f1 is None and hf is None):
        raise ValueError("initial_step: h needs 3 doubles; phase 0 needs hf")
    if hf is not None:
        _require_gpu(hf, "hf", torch.float32)
    nbytes = _lib.fn("gnpde_initial_step_workspace_bytes")()
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=y0.device)
    name = "gnpde_initial_step_bf16" if dt == torch.bfloat16 else "gnpde_initial_step_f32"
    _lib.call(name, y0.numel(), _ptr(y0), _ptr(f0), _ptr(f1), float(atol), float(rtol), float(order), _ptr(h),
              _ptr(hf), _ptr(ws), nbytes, _stream(y0.device))


def initial_step_lin(y0, v, atol, rtol, order, h, hf=None, ws=None):
    """Phase 1 of the device initial step from v = L f0 (gnpde_initial_step_lin_*):
    d2 = rms(v / scale); writes h[2] (and hf).  h: fp64 [3] after phase 0."""
    dt = y0.dtype
    if dt not in STATE_DTYPES:
        raise TypeError("initial_step_lin: state dtype %s" % dt)
    for t in (y0, v):
        _require_gpu(t, "initial_step state", dt)
        if not t.is_contiguous() or t.numel() != y0.numel():
            raise ValueError("initial_step_lin: y0 and v must be contiguous and shaped alike")
    _require_gpu(h, "h", torch.float64)
    if hf is not None:
        _require_gpu(hf, "hf", torch.float32)
    nbytes = _lib.fn("gnpde_initial_step_workspace_bytes")()
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=y0.device)
    name = "gnpde_initial_step_lin_f32" if dt == torch.float32 else "gnpde_initial_step_lin_bf16"
    _lib.call(name, y0.numel(), _ptr(y0), _ptr(v), float(atol), float(rtol), float(order), _ptr(h), _ptr(hf),
              _ptr(ws), ws.numel(), _stream(y0.device))


def initial_step_rows(rows_a, rows_b, n, order, h, hf, ws=None):
    """gnpde_initial_step_rows: the initial-step rules from the squared-sum rows of the f0
    launch (phase 0: rows_a its err_rows, rows_b its scale_rows) or of the launch over L f0
    (phase 1: rows_b None).  h: fp64 [3], hf: fp32 0-d (device)."""
    _require_gpu(rows_a, "rows", torch.float64)
    if rows_b is not None:
        _require_gpu(rows_b, "rows", torch.float64)
    _require_gpu(h, "h", torch.float64)
    if hf is not None:
        _require_gpu(hf, "hf", torch.float32)
    nbytes = _lib.fn("gnpde_initial_step_workspace_bytes")()
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=rows_a.device)
    _lib.call("gnpde_initial_step_rows", rows_a.numel(), _ptr(rows_a), _ptr(rows_b), float(n), float(order), _ptr(h),
              _ptr(hf), _ptr(ws), ws.numel(), _stream(rows_a.device))


def adaptive_control(err_rows, n, order, safety, ifactor, dfactor, dt, scale, rec, ws=None, t=None):
    """The step's error-row sum and torchdiffeq's step-size controller on the device
    (gnpde_adaptive_control): rec = {error ratio, dt, next dt, squared error sum};
    dt (fp64 0-d) and scale (fp32 0-d) advance to the next step's size; ``t`` (fp64,
    optional: its first element) advances by the step when it is accepted (the step
    start a folded dense output reads, Stage.dense).  ``ws``: a reusable workspace
    (gnpde_dot_workspace_bytes() bytes)."""
    _require_gpu(err_rows, "err_rows", torch.float64)
    _require_gpu(dt, "dt", torch.float64)
    _require_gpu(scale, "scale", torch.float32)
    _require_gpu(rec, "rec", torch.float64)
    if rec.numel() < 4:
        raise ValueError("adaptive_control: rec needs 4 doubles")
    if t is not None:
        _require_gpu(t, "t", torch.float64)
    nbytes = _lib.fn("gnpde_dot_workspace_bytes")()
    if ws is None:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=err_rows.device)
    _lib.call("gnpde_adaptive_control", err_rows.numel(), _ptr(err_rows), float(n), float(order), float(safety),
              float(ifactor), float(dfactor), _ptr(dt), _ptr(scale), _ptr(rec), _ptr(t), _ptr(ws), ws.numel(),
              _stream(err_rows.device))


def wcolsum(x, B, N, w):
    """y [B,H,C+1] fp64: y[b,h,:C] = sum_n w[b*N+n,h] x[b,n,:], y[b,h,C] = sum_n w[b*N+n,h]."""
    xr = _rows(x, "x")
    _require_gpu(w, "weights", torch.float64)
    w = w.contiguous()
    H = w.shape[-1]
    C = xr.shape[1]
    ws_bytes = _lib.fn("gnpde_wcolsum_workspace_bytes")(B, N, C, H)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=xr.device)
    y = torch.empty(B, H, C + 1, dtype=torch.float64, device=xr.device)
    _lib.call("gnpde_wcolsum_f64", _ptr(xr), B, N, C, C, _ptr(w), H, _ptr(y), _ptr(ws), ws_bytes,
              _stream(xr.device))
    return y


def score_input_grad(gcs, U, deg, gxbar, B, N, C, out=None):
    """gx [R,C] fp32 = gcs U_b^T + deg * gxbar_b  (reference-mode node-score backward)."""
    H = gcs.shape[-1]
    dev = gcs.device
    gx = torch.empty(B * N, C, dtype=torch.float32, device=dev) if out is None else out
    _lib.call("gnpde_score_input_grad_f32", _ptr(gcs.contiguous()), _ptr(U.contiguous()), _ptr(deg),
              _ptr(gxbar.contiguous()), B, N, C, H, _ptr(gx), C, int(out is not None), _stream(dev))
    return gx


def score_grad(grouped, side, ns, gs, with_params=False):
    """gnpde_score_grad_f32: dL/d(q) (side 0, over the aggregation CSR) or dL/d(k)
    (side 1, over the CSC) [R, att] from gs = dL/ds [B,E,H] (COO) for the per-edge
    score modes; with_params (exp_kernel): also the per-edge terms of
    dL/d(output_var), dL/d(lengthscale) summed in fp64 -> (out, g_p0, g_p1)."""
    _require_gpu(gs, "score grad", torch.float32)
    gs = gs.contiguous()
    att = ns.heads * ns.dk
    dev = gs.device
    out = torch.empty(grouped.R, att, dtype=torch.float32, device=dev)
    gp = torch.empty(max(grouped.nnz, 1), 2 * ns.heads, dtype=torch.float32, device=dev) if with_params else None
    _lib.call("gnpde_score_grad_f32", _ptr(grouped.rowptr), _ptr(grouped.col), _ptr(grouped.perm), grouped.R,
              grouped.nnz, int(side), ns.mode, ns.heads, ns.dk, _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(gs),
              _ptr(out), att, _ptr(gp), _stream(dev))
    if not with_params:
        return out
    if grouped.nnz == 0:
        z = torch.zeros((), dtype=torch.float64, device=dev)
        return out, z, z
    gpd = gp[:grouped.nnz].double()
    return out, gpd[:, :ns.heads].sum(), gpd[:, ns.heads:].sum()


def score_grad_split(grouped, side, ns, gs, dk_split, with_params=False):
    """gnpde_score_grad_split_f32: score_grad's exp_kernel path for heads of two parts
    (elements [0, dk_split) and [dk_split, dk) of each head; the beltrami product kernel
    folded into one exp_kernel): dL/d(q) (side 0) or dL/d(k) (side 1) [R, att]; with_params
    also the fp64 sums of the three per-edge columns -> (out, S0, S1, S2):
    S0 = sum g_s 2 s / p0, S1 / S2 = sum g_s s |q - k|^2 / p1^2 over the first / second part."""
    _require_gpu(gs, "score grad", torch.float32)
    if ns.mode != _lib.SCORE_EXP_KERNEL:
        raise ValueError("score_grad_split: exp_kernel scores only (mode %d)" % ns.mode)
    dk_split = int(dk_split)
    if not 0 <= dk_split <= ns.dk:
        raise ValueError("score_grad_split: dk_split %d outside [0, dk = %d]" % (dk_split, ns.dk))
    gs = gs.contiguous()
    H = ns.heads
    att = H * ns.dk
    if gs.numel() != max(grouped.nnz, 0) * H:
        raise ValueError("score_grad_split: gs holds %d values, expected nnz * heads = %d"
                         % (gs.numel(), grouped.nnz * H))
    dev = gs.device
    out = torch.empty(grouped.R, att, dtype=torch.float32, device=dev)
    gp = torch.empty(max(grouped.nnz, 1), 3 * H, dtype=torch.float32, device=dev) if with_params else None
    _lib.call("gnpde_score_grad_split_f32", _ptr(grouped.rowptr), _ptr(grouped.col), _ptr(grouped.perm), grouped.R,
              grouped.nnz, int(side), H, ns.dk, dk_split, _ptr(ns.q), _ptr(ns.k), ns.ldqk, ns.p0, ns.p1, _ptr(gs),
              _ptr(out), att, _ptr(gp), _stream(dev))
    if not with_params:
        return out
    if grouped.nnz == 0:
        z = torch.zeros((), dtype=torch.float64, device=dev)
        return out, z, z, z
    sums = gp[:grouped.nnz].double().view(grouped.nnz, 3, H).sum(dim=(0, 2))
    return out, sums[0], sums[1], sums[2]


def gather_head(grouped, w, h, scale=1.0):
    """scale * w[:, :, h] (COO [B,E,H]) in ``grouped`` order [nnz]."""
    _require_gpu(w, "values", torch.float32)
    w = w.contiguous()
    H = w.shape[-1]
    out = torch.empty(max(grouped.nnz, 1), dtype=torch.float32, device=w.device)
    _lib.call("gnpde_gather_head_f32", _ptr(w), grouped.nnz, H, int(h), _ptr(grouped.perm), float(scale), _ptr(out),
              _stream(w.device))
    return out


# --------------------------------------------------------------------------- solver glue
def rows_copy(src, dst, order=None, dst_copy=None):
    """gnpde_rows_copy: dst[k] = src[order[k]] (rows = the leading dims flattened,
    order int64 or None = identity) and, when given, dst_copy[order[k]] = the same
    row (a plain copy of src) from the same read."""
    _require_gpu(src, "src")
    src = src.contiguous()
    C = src.shape[-1]
    rows = src.numel() // max(C, 1)
    for t, nm in ((dst, "dst"), (dst_copy, "dst_copy")):
        if t is not None:
            _require_gpu(t, nm, src.dtype)
            if not t.is_contiguous() or t.numel() != src.numel():
                raise ValueError("rows_copy: %s must be contiguous and sized like src" % nm)
    if order is not None:
        _require_gpu(order, "order", torch.int64)
        if order.numel() != rows:
            raise ValueError("rows_copy: %d order entries for %d rows" % (order.numel(), rows))
    _lib.call("gnpde_rows_copy", _ptr(src), rows, C * src.element_size(), _ptr(order), _ptr(dst), _ptr(dst_copy),
              _stream(src.device))
    return dst


def rk_combine(y0, ks, coefs, scale, out=None):
    """out = y0 + scale * sum_j coefs[j] * ks[j]  (one fused pass; y0=None means 0)."""
    ref = y0 if y0 is not None else ks[0]
    _require_gpu(ref, "y0", torch.float32)
    if y0 is not None:
        y0 = y0.contiguous()
    if out is None:
        out = torch.empty_like(ref, memory_format=torch.contiguous_format)
    nk = len(ks)
    kp = (ctypes.c_void_p * max(nk, 1))()
    cf = (ctypes.c_double * max(nk, 1))()
    keep = []
    for j, (k, c) in enumerate(zip(ks, coefs)):
        _require_gpu(k, "k%d" % j, torch.float32)
        k = k.contiguous()
        keep.append(k)
        kp[j] = k.data_ptr()
        cf[j] = float(c)
    _lib.call("gnpde_rk_combine_f32", ref.numel(), _ptr(y0), nk, kp, cf, float(scale), _ptr(out),
              _stream(ref.device))
    return out


# --------------------------------------------------------------------------- regulariser row passes
ROW_MAX_ARRAYS = 4  # arrays of one gnpde_row_energy_f32 pass
ROW_MAX_COLS = 256  # row length the regulariser passes take


def _row_arrays(ks, name):
    """Contiguous fp32 device arrays of one shape [..., C] -> (list, R, C)."""
    ks = [k.contiguous() for k in ks]
    for j, k in enumerate(ks):
        _require_gpu(k, "%s[%d]" % (name, j), torch.float32)
        if k.shape != ks[0].shape or k.dim() < 1:
            raise ValueError("%s: arrays must share one shape [..., C]" % name)
    C = ks[0].shape[-1]
    return ks, ks[0].numel() // max(C, 1), C


def row_energy_torch(ks, coefs, acc=None, accumulate=False):
    """The row pass of ``row_energy`` restated in torch (any device): fp64
    s[r] = sum_i coefs[i] * sum_c ks[i][r,c]^2 over the leading dims' rows.  Returns the fp32
    rounding of s shaped like the leading dims, or, with ``acc`` (fp64, one entry per row), stores
    (or, with accumulate, adds) s there and returns ``acc``."""
    s = None
    for k, c in zip(ks, coefs):
        e = float(c) * k.double().pow(2).sum(-1)
        s = e if s is None else s + e
    if acc is None:
        return s.float()
    if accumulate:
        acc.add_(s.view(acc.shape))
    else:
        acc.copy_(s.view(acc.shape))
    return acc


def row_energy(ks, coefs, acc=None, accumulate=False):
    """s[r] = sum_i coefs[i] * sum_c ks[i][r,c]^2 in one read of up to 4 fp32 arrays [..., C]
    (gnpde_row_energy_f32: the per-row sum in fp64, a fixed order, no atomics).  Without ``acc``
    returns the fp32 rounding shaped like the leading dims; with ``acc`` (fp64 device tensor, one
    entry per row) stores s there, or adds it with accumulate=True, and returns ``acc``."""
    if not 1 <= len(ks) <= ROW_MAX_ARRAYS or len(coefs) != len(ks):
        raise ValueError("row_energy: 1 to %d arrays and one coefficient each" % ROW_MAX_ARRAYS)
    ks, R, C = _row_arrays(ks, "row_energy")
    if not 1 <= C <= ROW_MAX_COLS:
        raise ValueError("row_energy: rows of 1 to %d columns (got %d)" % (ROW_MAX_COLS, C))
    dev = ks[0].device
    n = len(ks)
    kp = (ctypes.c_void_p * n)(*[k.data_ptr() for k in ks])
    cf = (ctypes.c_double * n)(*[float(c) for c in coefs])
    out = None
    if acc is None:
        out = torch.empty(ks[0].shape[:-1], dtype=torch.float32, device=dev)
    else:
        _require_gpu(acc, "row_energy acc", torch.float64)
        if not acc.is_contiguous() or acc.numel() != R:
            raise ValueError("row_energy: acc must be contiguous with one fp64 per row")
    _lib.call("gnpde_row_energy_f32", R, C, n, kp, cf, _ptr(acc), int(bool(accumulate)), _ptr(out), _stream(dev))
    return out if acc is None else acc


def row_axpy_torch(base, terms, out=None):
    """``row_axpy`` restated in torch (any device): base + sum_j coef_j * g_j[..., None] * src_j,
    formed in fp64 and rounded to fp32 once; terms = [(coef, g, src), ...]."""
    src0 = terms[0][2] if terms else base
    s = torch.zeros(src0.shape, dtype=torch.float64, device=src0.device) if base is None else base.double()
    for c, g, src in terms:
        s = s + (float(c) * g.double()).reshape(src.shape[:-1]).unsqueeze(-1) * src.double()
    s = s.float()
    if out is not None:
        out.copy_(s)
        return out
    return s


def row_axpy(base, terms, out=None):
    """out[r,:] = base[r,:] + sum_j coef_j * g_j[r] * src_j[r,:] in one pass (gnpde_row_axpy_f32):
    terms = [(coef, g, src), ...], at most two; g_j one value per row, all fp32 or all fp64;
    ``base`` None = 0; ``out`` may be ``base`` (default: a new tensor).  Every element is an fp64
    sum rounded to fp32 once."""
    if len(terms) > 2 or (base is None and not terms):
        raise ValueError("row_axpy: a base and/or one or two terms")
    srcs, R, C = _row_arrays([s for _, _, s in terms] + ([base] if base is not None else []), "row_axpy")
    if not 1 <= C <= ROW_MAX_COLS:
        raise ValueError("row_axpy: rows of 1 to %d columns (got %d)" % (ROW_MAX_COLS, C))
    base_c = srcs.pop() if base is not None else None
    if out is base and base is not None and base_c is not base:
        raise ValueError("row_axpy: an in-place base must be contiguous")
    dev = srcs[0].device if srcs else base_c.device
    gs = [g.contiguous() for _, g, _ in terms]
    g_f64 = bool(gs) and gs[0].dtype == torch.float64
    for g in gs:
        _require_gpu(g, "row_axpy g", torch.float64 if g_f64 else torch.float32)
        if g.numel() != R:
            raise ValueError("row_axpy: g must hold one value per row")
    if out is None:
        out = torch.empty_like(srcs[0] if srcs else base_c)
    else:
        _require_gpu(out, "row_axpy out", torch.float32)
        if not out.is_contiguous() or out.numel() != R * C:
            raise ValueError("row_axpy: out must be contiguous and sized like the arrays")
    n = len(terms)
    sp = (ctypes.c_void_p * max(n, 1))(*[s.data_ptr() for s in srcs])
    gp = (ctypes.c_void_p * max(n, 1))(*[g.data_ptr() for g in gs])
    cf = (ctypes.c_double * max(n, 1))(*[float(c) for c, _, _ in terms])
    _lib.call("gnpde_row_axpy_f32", R, C, _ptr(base_c), n, sp, gp, int(g_f64), cf, _ptr(out), _stream(dev))
    return out


# --------------------------------------------------------------------------- multistep (Adams) passes
def _adams_operand(t, name, like):
    _require_gpu(t, name, torch.float32)
    if not t.is_contiguous() or t.numel() != like.numel():
        raise ValueError("adams: %s must be contiguous and sized like y0" % name)


def adams_predict(y0, hist, cdy, dy, x, cdelta=None, delta=None):
    """gnpde_adams_predict_f32: dy = sum_j cdy[j] hist[j], x = y0 + dy and (with ``cdelta`` /
    ``delta``) delta = sum_j cdelta[j] hist[j], from one read of y0 and of every history array
    (newest first, at most _lib.ADAMS_MAX_HISTORY); fp64 sums, one rounding per stored value.
    The coefficients carry the step size."""
    _require_gpu(y0, "y0", torch.float32)
    if not y0.is_contiguous():
        raise ValueError("adams: y0 must be contiguous")
    nh = len(hist)
    if not 1 <= nh <= _lib.ADAMS_MAX_HISTORY or len(cdy) != nh or (cdelta is not None and len(cdelta) != nh):
        raise ValueError("adams_predict: 1 to %d history arrays, one coefficient each" % _lib.ADAMS_MAX_HISTORY)
    if (cdelta is None) != (delta is None):
        raise ValueError("adams_predict: cdelta and delta go together")
    for t, nm in ((dy, "dy"), (x, "x")) + (((delta, "delta"),) if delta is not None else ()):
        _adams_operand(t, nm, y0)
    hp = (ctypes.c_void_p * nh)()
    c1 = (ctypes.c_double * nh)()
    c2 = (ctypes.c_double * nh)() if cdelta is not None else None
    for j, h in enumerate(hist):
        _adams_operand(h, "hist[%d]" % j, y0)
        hp[j] = h.data_ptr()
        c1[j] = float(cdy[j])
        if c2 is not None:
            c2[j] = float(cdelta[j])
    _lib.call("gnpde_adams_predict_f32", y0.numel(), _ptr(y0), nh, hp, c1, c2, _ptr(dy), _ptr(x), _ptr(delta),
              _stream(y0.device))
    return dy, x, delta


def adams_workspace(device):
    """The corrector's workspace, zeroed: int32 words, the first four the status record
    {converged, iterations, ratio (fp32 bits), reserved} (gnpde_adams_status_t)."""
    return torch.zeros(_lib.call_rc("gnpde_adams_workspace_bytes") // 4, dtype=torch.int32, device=device)


def adams_status_reset(ws):
    """Zero the status record and the arrival counter, in stream order (once per step)."""
    _require_gpu(ws, "ws", torch.int32)
    _lib.call("gnpde_adams_status_reset", _ptr(ws), _stream(ws.device))


def adams_correct(f, delta, y0, dy, x, cf, rtol, atol, ws):
    """gnpde_adams_correct_f32: one gated corrector iteration — unless ws's status says converged,
    dy <- cf f + delta, x <- y0 + dy, status <- {ratio < 1, iterations + 1, ratio} with ratio =
    max |dy_old - dy| / (atol + rtol max(|dy_old|, |dy|)) (a NaN propagates)."""
    _require_gpu(y0, "y0", torch.float32)
    _require_gpu(ws, "ws", torch.int32)
    if not y0.is_contiguous():
        raise ValueError("adams: y0 must be contiguous")
    for t, nm in ((f, "f"), (delta, "delta"), (dy, "dy"), (x, "x")):
        _adams_operand(t, nm, y0)
    _lib.call("gnpde_adams_correct_f32", y0.numel(), _ptr(f), _ptr(delta), _ptr(y0), float(cf), float(rtol),
              float(atol), _ptr(dy), _ptr(x), _ptr(ws), ws.numel() * 4, _stream(y0.device))


def adams_status(ws):
    """(converged, iterations, ratio) of the status record: one host read (it waits for the
    stream)."""
    rec = ws[:4].cpu()
    return bool(rec[0].item()), int(rec[1].item()), float(rec[2:3].view(torch.float32).item())


# --------------------------------------------------------------------------- early-stop scoring
def decode_score_torch(y, W, b, split, label, counts_out, ld=None, rows=None, pred_out=None):
    """gnpde_decode_score_f32 restated in torch ops (any device, no host read): the path
    for a decoder outside the kernel's range (K > 128 or Cd > 512) and the scorer the
    host tests inject.  Same contract: relu of the first Cd columns, the linear layer,
    argmax with the lowest class winning a tie, the hits of each split ADDED to
    counts_out[3]."""
    ld = y.shape[-1] if ld is None else int(ld)
    K, Cd = W.shape
    z = torch.relu(y.reshape(-1, ld)[:, :Cd].float())
    logits = z @ W.float().t()
    if b is not None:
        logits = logits + b.float()
    # the first maximal class (torch.max's index among ties is unspecified on a device)
    top = logits.max(dim=1, keepdim=True).values
    ids = torch.arange(K, device=y.device).expand_as(logits)
    pred = torch.where(logits == top, ids, torch.full_like(ids, K)).min(dim=1).values
    if rows is not None:
        r = rows.long()
        split, label = split[r], label[r]
    scored = split != 0
    hit = (pred == label.long()) & scored
    s = split.to(torch.int32)
    bits = torch.stack([(s >> k) & 1 for k in range(3)], 1)
    counts_out += (bits * hit.to(torch.int32).unsqueeze(1)).sum(0).to(counts_out.dtype)
    if pred_out is not None:
        pred_out.copy_(torch.where(scored, pred, torch.full_like(pred, -1)).to(pred_out.dtype))
    return counts_out


def decode_score(y, W, b, split, label, counts_out, ld=None, rows=None, pred_out=None):
    """gnpde_decode_score_f32: score one state against the packed splits (pack_splits) in
    one launch.  y [..., ld] fp32 (R rows), W [K, Cd] with Cd <= ld, b [K] or None; split
    uint8 [R] (bit 0 train, 1 validation, 2 test), label int32 [R]; rows int32 [R] or None
    (state row i takes split / label from position rows[i]: NodeLayout.order32); the
    three hit counts are ADDED to counts_out (int32 [3], e.g. one slot of a per-solve
    record); pred_out int32 [R] or None (-1: unscored row).  A decoder outside the
    kernel's range (GNPDE_EUNSUPPORTED) takes decode_score_torch."""
    _require_gpu(y, "y", torch.float32)
    if not y.is_contiguous():
        raise ValueError("decode_score: y must be contiguous")
    ld = y.shape[-1] if ld is None else int(ld)
    R = y.numel() // max(ld, 1)
    _require_gpu(W, "W", torch.float32)
    _require_gpu(split, "split", torch.uint8)
    _require_gpu(label, "label", torch.int32)
    _require_gpu(counts_out, "counts_out", torch.int32)
    if W.dim() != 2 or not W.is_contiguous():
        raise ValueError("decode_score: W must be a contiguous [K, Cd] matrix")
    K, Cd = W.shape
    if b is not None:
        _require_gpu(b, "b", torch.float32)
        if b.numel() != K or not b.is_contiguous():
            raise ValueError("decode_score: b must hold K contiguous entries")
    if split.numel() != R or label.numel() != R or not (split.is_contiguous() and label.is_contiguous()):
        raise ValueError("decode_score: split and label must hold one contiguous entry per state row (%d)" % R)
    if counts_out.numel() != 3 or not counts_out.is_contiguous():
        raise ValueError("decode_score: counts_out must be 3 contiguous int32")
    for t, nm in ((rows, "rows"), (pred_out, "pred_out")):
        if t is not None:
            _require_gpu(t, nm, torch.int32)
            if t.numel() != R or not t.is_contiguous():
                raise ValueError("decode_score: %s must hold one contiguous int32 per state row (%d)" % (nm, R))
    rc = _lib.call_rc("gnpde_decode_score_f32", _ptr(y), R, ld, Cd, _ptr(W), _ptr(b), K, _ptr(split), _ptr(label),
                      _ptr(rows), _ptr(counts_out), _ptr(pred_out), _stream(y.device))
    if rc == _lib.EUNSUPPORTED:
        return decode_score_torch(y, W, b, split, label, counts_out, ld=ld, rows=rows, pred_out=pred_out)
    _lib.check(rc, "gnpde_decode_score_f32")
    return counts_out


_SPLITS = {}  # (tensor keys of y and the masks, R, device) -> (split, label, sizes)


def pack_splits(data, R, device):
    """The packed split masks and labels of a data object, once per object: split uint8 [R]
    (bit 0 ``train_mask``, bit 1 ``val_mask``, bit 2 ``test_mask``), label int32 [R]
    (``data.y``) and the three mask sizes as host ints (read here, once).  The tensors are
    [N] or [B, N], flattened to rows; a per-node set repeats over the batch elements of
    a [B, N] state.  Cached by tensor identity and version."""
    srcs = (data.y, data.train_mask, data.val_mask, data.test_mask)
    key = tuple(_tensor_key(t) for t in srcs) + (int(R), str(device))
    hit = _SPLITS.get(key)
    if hit is not None:
        return hit

    def rows(t):
        t = t.reshape(-1)
        if t.numel() != R:
            if t.numel() == 0 or R % t.numel() != 0:
                raise ValueError("pack_splits: %d entries do not tile %d state rows" % (t.numel(), R))
            t = t.repeat(R // t.numel())
        return t

    masks = [rows(m).to(torch.bool) for m in srcs[1:]]
    split = torch.zeros(R, dtype=torch.uint8, device=masks[0].device)
    for k, m in enumerate(masks):
        split |= m.to(torch.uint8) << k
    sizes = tuple(int(v) for v in torch.stack([m.sum() for m in masks]).tolist())
    out = (split.to(device).contiguous(), rows(data.y).to(device=device, dtype=torch.int32).contiguous(), sizes)
    if len(_SPLITS) >= 8:
        _SPLITS.clear()
    _SPLITS[key] = out
    return out


# --------------------------------------------------------------------------- kNN rewiring
KNN_MAX_K = 64  # the kernel's range (csrc/knn.hip kKnnMaxK); a larger k takes knn_torch
KNN_TORCH_BYTES = 1 << 28  # knn_torch: bytes of one chunk's [rows, N, C] differences


def _knn_input(x, name):
    if not isinstance(x, torch.Tensor):
        raise TypeError("%s: x must be a torch.Tensor" % name)
    if x.dtype != torch.float32:
        raise TypeError("gnpde: %s: x must be torch.float32, got %s" % (name, x.dtype))
    if x.dim() == 2:
        x = x.unsqueeze(0)
    if x.dim() != 3 or x.shape[-1] < 1:
        raise ValueError("%s: x must be [B, N, C] or [N, C] with C >= 1, got %s" % (name, tuple(x.shape)))
    return x


def knn_mask(x):
    """The masked rows of x [B, N, C] (bool [B, N]): all zero, or any non-finite value."""
    return (x == 0).all(dim=-1) | ~torch.isfinite(x).all(dim=-1)


def knn_torch(x, k, return_dist=False, chunk_bytes=None):
    """gnpde_knn_f32 restated in torch ops (any device; chunked over query rows): the path
    for k > 64, the function the host tests inject and the baseline of tools/knn_bench.py.
    Same contract as knn: difference-form fp32 distances, the k smallest (d, j) keys in
    ascending order (one integer key (float bits of d) << 32 | j per pair, so the order
    does not depend on topk's tie behaviour), masked rows as in knn.  A graph with fewer
    than k unmasked rows pads with index -1 / distance +inf (k > N raises).  chunk_bytes:
    the size of one chunk's [rows, N, C] differences (KNN_TORCH_BYTES)."""
    x = _knn_input(x, "knn_torch")
    k = int(k)
    B, N, C = x.shape
    if k < 1:
        raise ValueError("knn_torch: k=%d must be >= 1" % k)
    if k > N:
        raise ValueError("knn_torch: k=%d exceeds the %d rows of a graph" % (k, N))
    dev = x.device
    masked = knn_mask(x)
    n_valid = (~masked).sum(dim=1).to(torch.int32)
    xs = torch.where(masked.unsqueeze(-1), torch.zeros_like(x), x)  # keep non-finite values out of the arithmetic
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=dev) if return_dist else None
    j = torch.arange(N, dtype=torch.int64, device=dev)
    none = torch.iinfo(torch.int64).max
    rows = max(1, min(N, int(chunk_bytes or KNN_TORCH_BYTES) // max(1, 4 * N * C)))
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            d = ((xs[b, r0:r1, None, :] - xs[b, None, :, :]) ** 2).sum(-1)          # [rows, N], d >= 0
            key = (d.view(torch.int32).to(torch.int64) << 32) | j                    # order of (d, j)
            key = torch.where(masked[b].unsqueeze(0), torch.full_like(key, none), key)
            top = torch.topk(key, k, dim=1, largest=False, sorted=True).values
            pad = top == none
            idx[b, r0:r1] = torch.where(pad, torch.full_like(top, -1), top & 0xFFFFFFFF).to(torch.int32)
            if return_dist:
                dd = (top >> 32).to(torch.int32).view(torch.float32)
                dist[b, r0:r1] = torch.where(pad, torch.full_like(dd, float("inf")), dd)
        own = torch.arange(N, dtype=torch.int32, device=dev).unsqueeze(1).expand(N, k)
        idx[b] = torch.where(masked[b].unsqueeze(1), own, idx[b])
        if return_dist:
            dist[b] = torch.where(masked[b].unsqueeze(1), torch.zeros_like(dist[b]), dist[b])
    return (idx, dist, n_valid) if return_dist else (idx, n_valid)


def knn(x, k, return_dist=False):
    """gnpde_knn_f32: the k nearest rows of every row of x [B, N, C] (or [N, C]: B = 1)
    within its graph, by d_ij = sum_c (x_ic - x_jc)^2 in fp32, in ascending (d_ij, j).
    Returns (idx int32 [B, N, k], n_valid int32 [B]) or (idx, dist fp32 [B, N, k],
    n_valid); nothing is read back here (n_valid stays on the device).  A masked row
    (all zero, or any non-finite value) is never a neighbour and returns its own index;
    a graph with n_valid < k pads with -1 / +inf (k > N raises).  A column prefix of a
    wider buffer: knn_strided.  k > 64 (outside the kernel's range) takes knn_torch."""
    return _knn(x, k, return_dist, None)


def knn_strided(buf, cols, k, return_dist=False):
    """knn on the first ``cols`` columns of a contiguous [B, N, ld] (or [N, ld]) buffer,
    without a copy (gnpde_knn_f32's ld > C)."""
    return _knn(buf, k, return_dist, int(cols))


def _knn(x, k, return_dist, cols):
    x = _knn_input(x, "knn")
    _require_gpu(x, "x", torch.float32)
    x = x.contiguous()
    k = int(k)
    B, N, ld = x.shape
    C = ld if cols is None else cols
    if not 1 <= C <= ld:
        raise ValueError("knn: cols=%d must be in [1, %d]" % (C, ld))
    if k < 1:
        raise ValueError("knn: k=%d must be >= 1" % k)
    if k > N:
        raise ValueError("knn: k=%d exceeds the %d rows of a graph" % (k, N))
    if k > KNN_MAX_K:
        return knn_torch(x[..., :C], k, return_dist)
    dev = x.device
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=dev) if return_dist else None
    n_valid = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.fn("gnpde_knn_workspace_bytes")(B, N)), dtype=torch.uint8, device=dev)
    _lib.call("gnpde_knn_f32", _ptr(x), B, N, C, ld, k, _ptr(idx), _ptr(dist), _ptr(n_valid), _ptr(ws),
              _stream(dev))
    return (idx, dist, n_valid) if return_dist else (idx, n_valid)


# --------------------------------------------------------------------------- multi_modal cross-attention
CROSS_ATTENTION_MAX_C = 256  # the kernel's range (csrc/cross_attention.hip kXaMaxC)


def _cross_attention_input(q, k, v, name):
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s: %s must be a torch.Tensor" % (name, nm))
        if t.dtype != torch.float32:
            raise TypeError("gnpde: %s: %s must be torch.float32, got %s" % (name, nm, t.dtype))
    if q.dim() == 2:
        q, k, v = q.unsqueeze(0), k.unsqueeze(0), v.unsqueeze(0)
    if q.dim() != 3 or k.dim() != 3 or q.shape[-1] < 1:
        raise ValueError("%s: q must be [B, N, C] and k / v [B, M, C] with C >= 1, got %s / %s / %s"
                         % (name, tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    if k.shape != v.shape or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
        raise ValueError("%s: k %s and v %s must both be [B=%d, M, C=%d]"
                         % (name, tuple(k.shape), tuple(v.shape), q.shape[0], q.shape[2]))
    if k.shape[1] < 1:
        raise ValueError("%s: M = 0 (a softmax over no keys)" % name)
    return q, k, v


def cross_attention_torch(q, k, v, scale, lse=False):
    """gnpde_cross_attention_f32 restated in torch ops (any device): the function the host
    tests check against the oracle and the baseline of tools/multimodal_bench.py.  Same
    contract as cross_attention; it materialises the [B, N, M] scores."""
    shape = q.shape
    q, k, v = _cross_attention_input(q, k, v, "cross_attention_torch")
    s = torch.matmul(q, k.transpose(1, 2)) * float(scale)
    out = torch.matmul(torch.softmax(s, dim=-1), v).view(shape)
    if lse:
        return out, torch.logsumexp(s, dim=-1).view(shape[:-1])
    return out


def cross_attention(q, k, v, scale, lse=False, out=None):
    """gnpde_cross_attention_f32: out[b,n,:] = softmax_m(scale * <q[b,n], k[b,m]>) v[b,m,:]
    for q [B, N, C] (or [N, C]: B = 1) and k / v [B, M, C] fp32, flash style on the fp32
    matrix cores: no [B, N, M] buffer.  lse=True also returns max + ln(sum exp) of the
    scaled scores per row [B, N] (what the backward recomputes the softmax from).
    1 <= C <= 256 (a wider C raises: there is no other device path), any N and M >= 1.
    The same bits on every run."""
    shape = q.shape
    q, k, v = _cross_attention_input(q, k, v, "cross_attention")
    for t, nm in ((q, "q"), (k, "k"), (v, "v")):
        _require_gpu(t, nm, torch.float32)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    B, N, C = q.shape
    M = k.shape[1]
    dev = q.device
    if out is None:
        out = torch.empty(B, N, C, dtype=torch.float32, device=dev)
    else:
        _require_gpu(out, "out", torch.float32)
        if not out.is_contiguous() or out.numel() != B * N * C:
            raise ValueError("cross_attention: out must be contiguous and hold %d x %d x %d" % (B, N, C))
    ls = torch.empty(B, N, dtype=torch.float32, device=dev) if lse else None
    _lib.call("gnpde_cross_attention_f32", _ptr(q), C, _ptr(k), _ptr(v), B, N, M, C, float(scale), _ptr(out), C,
              _ptr(ls), _stream(dev))
    out = out.view(shape)
    return (out, ls.view(shape[:-1])) if lse else out


# --------------------------------------------------------------------------- two-hop product (rewire_attention)
TWO_HOP_LDS_MAX = 512          # rows whose width bound fits the LDS hash table (csrc/two_hop.hip kThList)
TWO_HOP_SCRATCH_BYTES = 1 << 28  # global scratch of the wide rows: one accumulator + bitmap per resident wavefront
TWO_HOP_MAX_WAVES = 1024       # resident wavefronts of the wide-row regime
TWO_HOP_DENSE_N = 2048         # two_hop_torch: the dense route up to this many nodes


def _two_hop_coo(g_or_csr, w, num_nodes, name):
    """(N, row int64 [E], col int64 [E], w [E]) of any accepted input: a GraphCSR
    or an edge_index ([1,2,E] / [2,E], with num_nodes) with COO-order weights, or a coalesced
    CSR (rowptr, col) with CSR-order values."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("%s: w must be a torch.Tensor" % name)
    if isinstance(g_or_csr, GraphCSR):
        ei, N = g_or_csr.edge_index, g_or_csr.N
    elif isinstance(g_or_csr, torch.Tensor):
        if num_nodes is None:
            raise ValueError("%s: an edge_index needs num_nodes" % name)
        ei, N = g_or_csr, int(num_nodes)
    elif isinstance(g_or_csr, (tuple, list)) and len(g_or_csr) == 2:
        rowptr, col = g_or_csr
        N = rowptr.numel() - 1
        nnz = w.numel()
        if col.numel() < nnz:
            raise ValueError("%s: %d values for %d columns" % (name, nnz, col.numel()))
        row = torch.repeat_interleave(torch.arange(N, dtype=torch.int64, device=rowptr.device),
                                      (rowptr[1:] - rowptr[:-1]).long())
        if row.numel() != nnz:
            raise ValueError("%s: rowptr covers %d positions, w has %d" % (name, row.numel(), nnz))
        return N, row, col[:nnz].long(), w.reshape(-1)
    else:
        raise TypeError("%s: expected a GraphCSR, an edge_index or a (rowptr, col) pair" % name)
    if ei.dim() == 2:
        ei = ei.unsqueeze(0)
    if ei.dim() != 3 or ei.shape[1] != 2:
        raise ValueError("%s: edge_index must be [1,2,E] or [2,E], got %s" % (name, tuple(ei.shape)))
    if ei.shape[0] != 1:
        raise NotImplementedError("gnpde: %s: the product's edge count differs per graph; only B = 1 is supported"
                                  % name)
    if w.numel() != ei.shape[2]:
        raise ValueError("%s: %d weights for %d edges" % (name, w.numel(), ei.shape[2]))
    return N, ei[0, 0], ei[0, 1], w.reshape(-1)


def two_hop_torch(g_or_csr, w, num_nodes=None, dense_n=None):
    """two_hop restated in torch ops (any device): the function the host tests check against
    the oracle and the baseline of tools/rewire_bench.py.  Same contract: the structural
    positions of W·W in ascending (row, col) order, S = 0.5 W + 0.5 W·W on them with a zero
    diagonal, (edge_index int64 [1,2,nnz], values [nnz], rowptr int32 [N+1]).  Up to dense_n
    (TWO_HOP_DENSE_N) nodes it densifies as the reference does; beyond, torch.sparse.mm and
    coalesce.  The summation order is torch's, not the kernel's."""
    N, row, col, wv = _two_hop_coo(g_or_csr, w, num_nodes, "two_hop_torch")
    dev = wv.device
    row, col = row.to(dev), col.to(dev)
    if N <= int(TWO_HOP_DENSE_N if dense_n is None else dense_n):
        W = torch.zeros(N, N, dtype=wv.dtype, device=dev).index_put_((row, col), wv, accumulate=True)
        A = torch.zeros(N, N, dtype=torch.float64, device=dev).index_put_((row, col), torch.ones((), dtype=torch.float64,
                                                                                                device=dev))
        pos = torch.nonzero(torch.matmul(A, A) > 0)          # row-major: ascending (row, col)
        S = 0.5 * W + 0.5 * torch.matmul(W, W)
        S.fill_diagonal_(0)
        r, c = pos[:, 0], pos[:, 1]
        vals = S[r, c]
    else:
        Wc = torch.sparse_coo_tensor(torch.stack([row, col]), wv, (N, N)).coalesce()
        WW = torch.sparse.mm(Wc, Wc).coalesce()
        r, c = WW.indices()[0], WW.indices()[1]
        vals = 0.5 * WW.values()
        kww = r * N + c
        kw = Wc.indices()[0] * N + Wc.indices()[1]
        at = torch.searchsorted(kww, kw).clamp(max=max(kww.numel() - 1, 0))
        hit = (kww[at] == kw) if kww.numel() else torch.zeros_like(kw, dtype=torch.bool)
        vals[at[hit]] += 0.5 * Wc.values()[hit]              # W is coalesced: every position at most once
        vals = torch.where(r == c, torch.zeros_like(vals), vals)
    rowptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(r, minlength=N), 0)
    return torch.stack([r, c]).unsqueeze(0), vals, rowptr.to(torch.int32)


def coalesced_csr(g, w):
    """The coalesced CSR of a GraphCSR g (B = 1) with COO-order weights w: (rowptr int32
    [N+1], col int32, val fp32), rows sorted by column, duplicates summed one after another in
    COO order (gnpde_coalesce_sum_f32).  col / val keep the capacity of g's edge count (the
    coalesced length is rowptr[N], on the device): nothing is read back."""
    _require_gpu(w, "weights", torch.float32)
    if g.B != 1:
        raise NotImplementedError("gnpde: coalesced_csr: only B = 1 is supported")
    csr, N, E = g.csr, g.N, g.nnz
    dev = w.device
    if w.numel() != E:
        raise ValueError("coalesced_csr: %d weights for %d edges" % (w.numel(), E))
    if E == 0:
        return (torch.zeros(N + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                torch.zeros(1, dtype=torch.float32, device=dev))
    key = csr.rowidx[:E].long() * N + csr.col[:E].long()
    skey, order = torch.sort(key, stable=True)     # equal (row, col) keep their CSR (= COO) order
    ws = w.reshape(-1)[csr.perm[:E].long()][order].contiguous()
    first = torch.ones(E, dtype=torch.bool, device=dev)
    first[1:] = skey[1:] != skey[:-1]
    csum = torch.cumsum(first, 0)
    uid = (csum - 1).contiguous()
    col = torch.zeros(E, dtype=torch.int32, device=dev)
    col[uid] = (skey % N).to(torch.int32)          # the entries of a run write the same value
    val = torch.zeros(E, dtype=torch.float32, device=dev)
    first8 = first.to(torch.uint8)
    _lib.call("gnpde_coalesce_sum_f32", _ptr(ws), _ptr(first8), _ptr(uid), E, _ptr(val), _stream(dev))
    before = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), csum])   # runs that start before position p
    rowptr = before[csr.rowptr.long()].to(torch.int32).contiguous()             # a row's positions stay its own
    return rowptr, col, val


def two_hop_check_length(nnz):
    """The product's length, checked before anything of that length is allocated."""
    if nnz >= 2 ** 31:
        raise ValueError("two_hop: the product has %d positions, the int32 CSR holds fewer than 2^31" % nnz)
    return nnz


def two_hop(g_or_csr, w, num_nodes=None, lds_max=None, scratch_bytes=None, return_col=False):
    """The two-hop product of the rewire_attention block (csrc/two_hop.hip): for W given as a
    GraphCSR or an edge_index ([1,2,E] / [2,E] int64 with num_nodes) with COO-order fp32 weights
    (duplicates are summed: coalesced_csr), or as an already coalesced CSR (rowptr, col) with
    CSR-order values, the structural positions of W·W in ascending (row, col) order and
      S[i, j] = 0.5 * ((sum_m W[i, m] W[m, j]) + W[i, j]),  S[i, i] = 0
    on them.  Returns (edge_index int64 [1,2,nnz], values fp32 [nnz], rowptr int32 [N+1])
    (and the int32 columns with return_col).  Deterministic: the sum runs over the m of row i
    in CSR order, no floating-point atomic.  Regimes: rows whose width bound ub_i = sum of the
    neighbour rows' lengths is at most lds_max (default TWO_HOP_LDS_MAX, the largest value)
    accumulate in an LDS hash table; wider rows in a dense accumulator in global scratch, one
    per resident wavefront, as many as fit scratch_bytes (TWO_HOP_SCRATCH_BYTES).  One device
    read: the product's length, to allocate it; 2^31 positions or more raise ValueError.  (An
    edge_index or a (rowptr, col) pair is range-checked first, which reads the device too; a
    GraphCSR was checked when it was built.)"""
    if isinstance(w, torch.Tensor) and w.dtype != torch.float32:
        raise TypeError("gnpde: two_hop: the weights must be torch.float32, got %s" % w.dtype)
    if isinstance(g_or_csr, (tuple, list)) and len(g_or_csr) == 2:
        rowptr, col = g_or_csr
        _require_gpu(rowptr, "rowptr", torch.int32)
        _require_gpu(col, "col", torch.int32)
        _require_gpu(w, "values", torch.float32)
        rowptr, col, val = rowptr.contiguous(), col.contiguous(), w.contiguous().reshape(-1)
        N = rowptr.numel() - 1
        if val.numel():
            lo, hi = int(col[:val.numel()].min()), int(col[:val.numel()].max())
            if lo < 0 or hi >= N or int(rowptr[-1]) != val.numel():
                raise IndexError("two_hop: CSR columns must be in [0, %d) and rowptr[N] the value count" % N)
    else:
        if not isinstance(w, torch.Tensor):
            raise TypeError("two_hop: w must be a torch.Tensor")
        _require_gpu(w, "weights", torch.float32)
        if isinstance(g_or_csr, torch.Tensor):
            N0, r, c, _ = _two_hop_coo(g_or_csr, w, num_nodes, "two_hop")
            g = GraphCSR(torch.stack([r, c]).unsqueeze(0), N0)
        elif isinstance(g_or_csr, GraphCSR):
            g = g_or_csr
            _two_hop_coo(g, w, None, "two_hop")
        else:
            raise TypeError("two_hop: expected a GraphCSR, an edge_index or a (rowptr, col) pair")
        rowptr, col, val = coalesced_csr(g, w.contiguous())
        N = g.N
    dev = val.device
    cap = int(_lib.fn("gnpde_two_hop_lds_max")())
    lds_max = TWO_HOP_LDS_MAX if lds_max is None else int(lds_max)
    if not 0 <= lds_max <= cap:
        raise ValueError("two_hop: lds_max=%d must be in [0, %d]" % (lds_max, cap))
    if N == 0:
        out = (torch.zeros(1, 2, 0, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.float32, device=dev),
               torch.zeros(1, dtype=torch.int32, device=dev))
        return out + (torch.zeros(0, dtype=torch.int32, device=dev),) if return_col else out
    words = (N + 31) // 32
    budget = TWO_HOP_SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
    n_waves = max(1, min(TWO_HOP_MAX_WAVES, budget // (4 * (N + words))))
    acc = torch.empty(n_waves * N, dtype=torch.float32, device=dev)
    bits = torch.zeros(n_waves * words, dtype=torch.int32, device=dev)
    ub = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.empty(N, dtype=torch.int32, device=dev)
    st = _stream(dev)
    _lib.call("gnpde_two_hop_bound_i32", _ptr(rowptr), _ptr(col), N, _ptr(ub), st)
    _lib.call("gnpde_two_hop_count_i32", _ptr(rowptr), _ptr(col), N, _ptr(ub), lds_max, n_waves, _ptr(acc), _ptr(bits),
              _ptr(count), st)
    ptr64 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    ptr64[1:] = torch.cumsum(count, 0, dtype=torch.int64)
    nnz = two_hop_check_length(int(ptr64[-1]))  # the one device read: the product's length
    out_ptr = ptr64.to(torch.int32)
    out_col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    out_val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
    out_ei = torch.empty(1, 2, nnz, dtype=torch.int64, device=dev)
    _lib.call("gnpde_two_hop_fill_f32", _ptr(rowptr), _ptr(col), _ptr(val), N, _ptr(ub), lds_max, n_waves, _ptr(acc),
              _ptr(bits), _ptr(out_ptr), nnz, _ptr(out_col), _ptr(out_val), _ptr(out_ei), st)
    out = (out_ei, out_val[:nnz], out_ptr)
    return out + (out_col[:nnz],) if return_col else out


# --------------------------------------------------------------------------- GDC diffusion rewiring
TOPK_COLS_MAX_K = 128          # the kernel's range (csrc/topk_cols.hip kTkMaxK)
GDC_BLOCK = 128                # seeds of one column block: K1's headline width
GDC_MAX_BYTES = 8 << 30        # the dense positional encoding's size guard
# The seed term of a diffusion launch (diffusion_block): from this many rows on it is added to
# the block's diagonal after the launch instead of streaming E_J as a stage operand.  Measured
# at two sizes only (profiles/gdc_bench.json): 169,343 rows 99.8 against 111.9 us per product;
# 2,708 rows, where the extra launch is what costs, 26.2 against 21.9.  The crossover between
# them is not measured: the limit is LAYOUT_MIN_ROWS, below which the state sits in cache.
GDC_DIAGONAL_MIN_ROWS = 32768


def _topk_cols_input(y, k, ncols, name):
    if not isinstance(y, torch.Tensor):
        raise TypeError("%s: y must be a torch.Tensor" % name)
    if y.dtype != torch.float32:
        raise TypeError("gnpde: %s: y must be torch.float32, got %s" % (name, y.dtype))
    if y.dim() != 2:
        raise ValueError("%s: y must be [N, ld], got %s" % (name, tuple(y.shape)))
    N, ld = y.shape
    ncols = ld if ncols is None else int(ncols)
    k = int(k)
    if not 0 <= ncols <= ld:
        raise ValueError("%s: ncols=%d must be in [0, ld=%d]" % (name, ncols, ld))
    if k < 1:
        raise ValueError("%s: k=%d must be >= 1" % (name, k))
    if k > N:
        raise ValueError("%s: k=%d exceeds the %d rows of the block" % (name, k, N))
    return N, ld, ncols, k


def _value_order_code(v):
    """int64 code of fp32 values whose ascending order is the values' DESCENDING order
    (-0 as +0): csrc/topk_cols.hip tk_encode, shifted into the signed range."""
    u = v.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    u = torch.where((u & 0x7FFFFFFF) == 0, torch.zeros_like(u), u)
    m = torch.where(u >= 0x80000000, 0xFFFFFFFF - u, u + 0x80000000)
    return (0xFFFFFFFF - m) - 0x80000000


def rank_order_sum(val):
    """val [n, k] fp32 -> the sum of every row taken sequentially in fp32, column 0 first."""
    s = torch.zeros(val.shape[0], dtype=torch.float32, device=val.device)
    for i in range(val.shape[1]):
        s = s + val[:, i]
    return s


def topk_cols_torch(y, k, ncols=None):
    """gnpde_topk_cols_f32 restated in torch ops (any device): for every column c < ncols of
    the row-major block y [N, ld] the k entries largest in the total order (value descending,
    row ascending; -0 as +0) -> (idx int32 [ncols, k], val fp32 [ncols, k], wnorm fp32
    [ncols, k]), wnorm = val / the sequential fp32 sum of val in rank order (0 for a zero sum).
    One integer key per entry, so the result does not depend on topk's tie behaviour."""
    N, ld, ncols, k = _topk_cols_input(y, k, ncols, "topk_cols_torch")
    dev = y.device
    yt = y[:, :ncols].t().contiguous()                                        # [ncols, N]
    key = (_value_order_code(yt) << 32) + torch.arange(N, dtype=torch.int64, device=dev)
    top = torch.topk(key, k, dim=1, largest=False, sorted=True).values
    idx = top & 0xFFFFFFFF
    val = torch.gather(yt, 1, idx)
    val = torch.where(val == 0, torch.zeros_like(val), val)
    s = rank_order_sum(val).unsqueeze(1)
    wnorm = torch.where(s == 0, torch.zeros_like(val), val / s)
    return idx.to(torch.int32), val, wnorm


def topk_cols(y, k, ncols=None, rows_per_wg=None):
    """gnpde_topk_cols_f32 (csrc/topk_cols.hip): the k largest entries of every column
    c < ncols (default: all) of the contiguous row-major block y [N, ld] fp32, in the total
    order (value descending, row ascending) -> (idx int32 [ncols, k], val, wnorm) as
    topk_cols_torch.  Finite inputs; 1 <= k <= 128 and k <= N.  rows_per_wg (tests only): the
    rows one workgroup scans; the outputs do not depend on it."""
    N, ld, ncols, k = _topk_cols_input(y, k, ncols, "topk_cols")
    _require_gpu(y, "y", torch.float32)
    if not y.is_contiguous():
        raise ValueError("topk_cols: y must be contiguous")
    dev = y.device
    rp = 0 if rows_per_wg is None else int(rows_per_wg)
    idx = torch.empty(ncols, k, dtype=torch.int32, device=dev)
    val = torch.empty(ncols, k, dtype=torch.float32, device=dev)
    wnorm = torch.empty(ncols, k, dtype=torch.float32, device=dev)
    nbytes = int(_lib.fn("gnpde_topk_cols_workspace_bytes")(N, ncols, k, rp))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("gnpde_topk_cols_f32", _ptr(y), N, ncols, ld, k, _ptr(idx), _ptr(val), _ptr(wnorm), rp, _ptr(ws),
              nbytes, _stream(dev))
    return idx, val, wnorm


class DiffusionSchedule(object):
    """The coefficient schedule of one diffusion column block (diffusion_schedule): the
    iterate starts at ``init`` * E_J and every step forms, with one product T·x,
        x_next = cb * x_prev + cf * (T x) + ce * E_J      (steps: [(cb, cf, ce), ...]),
    x_prev the iterate before x (``two_term``; absent, i.e. 0, at the first step) — or no
    such term at all.  ``bound``: the 2-norm distance of the last iterate from the exact
    column in exact arithmetic."""

    def __init__(self, method, param, init, steps, two_term, bound):
        self.method, self.param, self.init, self.steps = method, param, init, steps
        self.two_term, self.bound = two_term, bound

    @property
    def products(self):
        return len(self.steps)


def diffusion_schedule(method, alpha=None, t=None, tol=1e-6):
    """Host code only.  'ppr': the Chebyshev iteration on (I - (1 - alpha) T) s = alpha e for
    a spectrum in [alpha, 2 - alpha] (T symmetric with its spectrum in [-1, 1]):
    x_0 = 0, x_1 = alpha E, x_{m+1} = w_{m+1} (1 - alpha) T x_m + (1 - w_{m+1}) x_{m-1} +
    w_{m+1} alpha E with w_2 = 1 / (1 - q/2), w_{m+1} = 1 / (1 - w_m q / 4), q = (1 - alpha)^2,
    stopped at the first m with 2 rho^m <= tol alpha, rho = (sqrt(kappa) - 1) / (sqrt(kappa) +
    1), kappa = (2 - alpha) / alpha (|x_m - s|_2 <= 2 rho^m |s|_2 and |S e_j|_2 <= 1).
    'heat': Horner on the Taylor series theta_p = e^-t t^p / p!: Y = theta_K E, then
    Y <- T Y + theta_p E for p = K - 1 .. 0, K the first index whose tail sum_{p > K} theta_p
    is at most tol e^-t."""
    tol = float(tol)
    if not tol > 0:
        raise ValueError("diffusion_schedule: tol=%r must be positive" % tol)
    if method == 'ppr':
        a = float(alpha)
        if not 0.0 < a < 1.0:
            raise ValueError("diffusion_schedule: ppr alpha=%r must be in (0, 1)" % a)
        kappa = (2.0 - a) / a
        rho = (math.sqrt(kappa) - 1.0) / (math.sqrt(kappa) + 1.0)
        m = 1
        while 2.0 * rho ** m > tol * a:
            m += 1
        q = (1.0 - a) ** 2
        steps, w = [], None
        for _ in range(m - 1):  # x_2 .. x_m
            w = 1.0 / (1.0 - q / 2.0) if w is None else 1.0 / (1.0 - w * q / 4.0)
            steps.append((1.0 - w, w * (1.0 - a), w * a))
        return DiffusionSchedule('ppr', a, a, steps, True, 2.0 * rho ** m)
    if method == 'heat':
        tt = float(t)
        if not tt >= 0.0:
            raise ValueError("diffusion_schedule: heat t=%r must be >= 0" % tt)
        e = math.exp(-tt)
        theta, total = [e], e
        while 1.0 - total > tol * e and len(theta) < 1000:
            theta.append(theta[-1] * tt / len(theta))
            total += theta[-1]
        K = len(theta) - 1
        steps = [(0.0, 1.0, theta[p]) for p in range(K - 1, -1, -1)]
        return DiffusionSchedule('heat', tt, theta[K], steps, False, max(1.0 - total, 0.0))
    raise ValueError("diffusion_schedule: method %r (ppr | heat)" % (method,))


def _seed_block(N, j0, ncols, device, dtype=torch.float32):
    """E_J [N, ncols]: column c is the unit vector of node j0 + c."""
    E = torch.zeros(N, ncols, dtype=dtype, device=device)
    E[j0:j0 + ncols].fill_diagonal_(1.0)
    return E


def diffusion_block(g, w, j0, ncols, schedule, seed=None):
    """The columns [j0, j0 + ncols) of the diffusion matrix of T (GraphCSR ``g`` with
    CSR-order weights ``w``, symmetric) by ``schedule``: one K1 launch per product, the
    step's combination fused into its stage epilogue, two [N, ncols] buffers in turn (the
    ppr output overwrites x_{m-1}, its own base).  seed: 'operand' — E_J materialised once and
    passed as the stage's operand; 'diagonal' — no operand, ce added to the block's diagonal
    after the launch; None — by size (GDC_DIAGONAL_MIN_ROWS).  -> fp32 [N, ncols]."""
    if g.B != 1:
        raise NotImplementedError("gnpde: diffusion_block: only B = 1 is supported")
    if seed is None:
        seed = 'diagonal' if g.N >= GDC_DIAGONAL_MIN_ROWS else 'operand'
    if seed not in ('operand', 'diagonal'):
        raise ValueError("diffusion_block: seed %r (operand | diagonal)" % (seed,))
    N, j0, ncols = g.N, int(j0), int(ncols)
    if not (0 <= j0 and 1 <= ncols and j0 + ncols <= N):
        raise ValueError("diffusion_block: columns [%d, %d) outside [0, %d)" % (j0, j0 + ncols, N))
    dev = w.device
    if seed == 'operand':
        E = _seed_block(N, j0, ncols, dev)
        cur = E * schedule.init
    else:  # no E_J at all: the start is init on the block's diagonal
        E = None
        cur = torch.zeros(N, ncols, dtype=torch.float32, device=dev)
        cur[j0:j0 + ncols].fill_diagonal_(schedule.init)
    other = torch.empty_like(cur)
    prev = None
    for cb, cf, ce in schedule.steps:
        if schedule.two_term:
            out, base = (prev, prev) if prev is not None else (other, None)
        else:
            out, base = other, None
        terms = [(E, ce)] if seed == 'operand' else []
        spmm_rhs(g, w, cur, rhs=False, stage=Stage(outs=[(out, base, cb if base is not None else 0.0, cf, terms)]))
        if seed == 'diagonal':
            out[j0:j0 + ncols].diagonal().add_(ce)
        if schedule.two_term:
            prev, cur = cur, out
        else:
            cur, other = out, cur
    return cur


def diffusion_block_torch(T, j0, ncols, schedule, dtype=torch.float32):
    """diffusion_block in torch ops: T a torch sparse (or dense) [N, N] matrix."""
    N = T.shape[0]
    E = _seed_block(N, j0, ncols, T.device, dtype)
    cur, prev = E * schedule.init, None
    mm = torch.sparse.mm if T.layout != torch.strided else torch.matmul
    for cb, cf, ce in schedule.steps:
        nxt = cf * mm(T, cur) + ce * E
        if schedule.two_term and prev is not None:
            nxt = nxt + cb * prev
        prev, cur = cur, nxt
    return cur


def _gdc_edges(edge_index, w, N, name):
    if not isinstance(edge_index, torch.Tensor) or edge_index.dtype != torch.int64:
        raise TypeError("%s: edge_index must be an int64 tensor" % name)
    ei = edge_index
    if ei.dim() == 3:
        if ei.shape[0] != 1:
            raise NotImplementedError("gnpde: %s: the rewired edge count differs per graph; only B = 1 is supported"
                                      % name)
        ei = ei[0]
    if ei.dim() != 2 or ei.shape[0] != 2:
        raise ValueError("%s: edge_index must be [2,E] or [1,2,E], got %s" % (name, tuple(edge_index.shape)))
    E = ei.shape[1]
    if w is None:
        w = torch.ones(E, dtype=torch.float32, device=ei.device)
    else:
        if w.dtype != torch.float32:
            raise TypeError("gnpde: %s: weights must be torch.float32, got %s" % (name, w.dtype))
        w = w.reshape(-1)
        if w.numel() != E:
            raise ValueError("%s: %d weights for %d edges" % (name, w.numel(), E))
    if E and (int(ei.min()) < 0 or int(ei.max()) >= N):
        raise IndexError("%s: edge_index values must be in [0, %d)" % (name, N))
    return ei[0], ei[1], w


def _coalesce_sum(row, col, w, N):
    """(row, col, w) -> sorted by (row, col), duplicates summed one after another in COO
    order (no atomics: every pass adds to distinct positions)."""
    if row.numel() == 0:
        return row, col, w
    key = row * N + col
    skey, order = torch.sort(key, stable=True)
    ws = w[order]
    first = torch.ones_like(skey, dtype=torch.bool)
    first[1:] = skey[1:] != skey[:-1]
    uid = torch.cumsum(first, 0) - 1
    pos = torch.arange(skey.numel(), device=skey.device)
    start = torch.zeros(int(uid[-1]) + 1, dtype=torch.int64, device=skey.device)
    start[uid[first]] = pos[first]
    rank = pos - start[uid]
    val = torch.zeros(start.numel(), dtype=w.dtype, device=w.device)
    for r in range(int(rank.max()) + 1):
        sel = rank == r
        val[uid[sel]] += ws[sel]
    ukey = skey[first]
    return torch.div(ukey, N, rounding_mode='floor'), ukey % N, val


def _last_self_loops(row, col, w, N, fill):
    """add_remaining_self_loops as ops.add_self_loops reads it: the non-loop edges, then one
    loop per node with its last existing loop's weight, or ``fill``."""
    loop = row == col
    pos = torch.arange(row.numel(), device=row.device)
    last = torch.full((N,), -1, dtype=torch.int64, device=row.device)
    if bool(loop.any()):
        last = last.scatter_reduce(0, row[loop], pos[loop], 'amax', include_self=True)
    lw = torch.full((N,), float(fill), dtype=w.dtype, device=w.device)
    has = last >= 0
    lw[has] = w[last[has]]
    nodes = torch.arange(N, device=row.device)
    return torch.cat([row[~loop], nodes]), torch.cat([col[~loop], nodes]), torch.cat([w[~loop], lw])


def gdc_matrix(edge_index, w, N, self_loop_weight=1.0, remaining=False):
    """Steps 1 and 2's input of the GDC contract, in torch ops on any device: M = coalesce(A) +
    w_self I (remaining=False, PyG GDC.__call__) or A with the missing self loops filled
    (remaining=True, GDCWrapper.position_encoding), coalesced and sorted by (row, col), and
    checked symmetric on the device -> (row, col, val)."""
    row, col, w = _gdc_edges(edge_index, w, N, "gdc")
    ws = 0.0 if self_loop_weight is None else float(self_loop_weight)
    if ws != 0.0:
        if remaining:
            row, col, w = _last_self_loops(row, col, w, N, ws)
        else:
            nodes = torch.arange(N, device=row.device)
            row, col = torch.cat([row, nodes]), torch.cat([col, nodes])
            w = torch.cat([w, torch.full((N,), ws, dtype=w.dtype, device=w.device)])
    row, col, val = _coalesce_sum(row, col, w, N)
    tkey, order = torch.sort(col * N + row)
    if not (torch.equal(tkey, row * N + col) and torch.equal(val[order], val)):
        raise ValueError("gdc: normalization_in='sym' needs a symmetric weighted graph (the iteration bounds rest "
                         "on T's spectrum lying in [-1, 1]); symmetrise it first, e.g. with "
                         "graph_rewiring.to_undirected")
    return row, col, val


def _gdc_schedule(method, alpha, t, tol):
    return diffusion_schedule('ppr', alpha=alpha, tol=tol) if method == 'ppr' else \
        diffusion_schedule('heat', t=t, tol=tol)


def _gdc_check(N, sparsification, k, dense, max_bytes):
    if dense:
        if 4 * N * N > int(max_bytes):
            raise ValueError("gdc: the dense [%d, %d] positional encoding takes %d bytes, above max_bytes=%d"
                             % (N, N, 4 * N * N, int(max_bytes)))
    elif sparsification == 'topk':
        if int(k) < 1:
            raise ValueError("gdc: gdc_k=%d must be >= 1" % int(k))
        if int(k) > N:
            raise ValueError("gdc: gdc_k=%d exceeds the %d nodes of the graph" % (int(k), N))
    elif sparsification != 'threshold':
        raise ValueError("gdc: sparsification %r (topk | threshold)" % (sparsification,))


def _gdc_run(N, block_fn, topk_fn, sparsification, k, threshold, dense, block, dev):
    """The per-block part shared by gdc and gdc_torch: block_fn(j0, ncols) -> Y [N, ncols]."""
    if dense:
        S = torch.empty(N, N, dtype=torch.float32, device=dev)
    rows, cols, vals = [], [], []
    for j0 in range(0, N, block):
        ncols = min(block, N - j0)
        Y = block_fn(j0, ncols)
        if dense:
            s = Y.sum(0, keepdim=True)
            S[:, j0:j0 + ncols] = torch.where(s == 0, torch.zeros_like(Y), Y / s)
        elif sparsification == 'topk':
            idx, _val, wn = topk_fn(Y, k)
            rows.append(idx.reshape(-1).to(torch.int64))
            cols.append(torch.arange(j0, j0 + ncols, device=dev).repeat_interleave(k))
            vals.append(wn.reshape(-1))
        else:
            keep = Y >= threshold
            kept = torch.where(keep, Y, torch.zeros_like(Y))
            s = kept.sum(0, keepdim=True)
            wn = torch.where(s == 0, torch.zeros_like(Y), kept / s)
            at = torch.nonzero(keep)
            rows.append(at[:, 0])
            cols.append(at[:, 1] + j0)
            vals.append(wn[at[:, 0], at[:, 1]])
    if dense:
        return S
    row, col, val = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    order = torch.argsort(row * N + col)
    return torch.stack([row[order], col[order]]), val[order]


def gdc(edge_index, w, N, method='ppr', alpha=0.05, t=3.0, self_loop_weight=1.0, sparsification='topk', k=64,
        threshold=0.01, tol=1e-6, dense=False, max_bytes=GDC_MAX_BYTES, seed=None, block=GDC_BLOCK):
    """Graph diffusion convolution of one symmetric graph on the device (the contract of
    gnpde.graph_rewiring's docstring): M with self loops, T = D^-1/2 M D^-1/2 (ops.norm_weights,
    GCN), then per block of ``block`` seed columns the diffusion recurrence on K1
    (diffusion_block) and the column top-k (topk_cols) or the threshold, column-normalised.
    -> (edge_index int64 [2, E] sorted by (row, col), weights fp32 [E]); dense=True (the
    positional encoding; self loops by add_remaining_self_loops = ops.add_self_loops): the
    column-normalised S, fp32 [N, N], at most max_bytes."""
    N = int(N)
    _require_gpu(edge_index, "edge_index", torch.int64)
    if w is not None:
        _require_gpu(w, "edge weights", torch.float32)
    _gdc_check(N, sparsification, k, dense, max_bytes)
    if sparsification == 'topk' and not dense and int(k) > TOPK_COLS_MAX_K:
        raise ValueError("gdc: gdc_k=%d outside the kernel's range (1 <= k <= %d)" % (int(k), TOPK_COLS_MAX_K))
    dev = edge_index.device
    ws = 0.0 if self_loop_weight is None else float(self_loop_weight)
    if dense and ws != 0.0:
        row, col, wv = _gdc_edges(edge_index, w, N, "gdc")
        ei, wl = add_self_loops(torch.stack([row, col]).unsqueeze(0), wv.unsqueeze(0), ws, N)
        row, col, val = gdc_matrix(ei, wl.reshape(-1), N, 0.0)
    else:
        row, col, val = gdc_matrix(edge_index, w, N, ws)
    ei = torch.stack([row, col]).unsqueeze(0).contiguous()
    tw = norm_weights(ei, val.unsqueeze(0).contiguous(), N, _lib.NORM_GCN)
    g = GraphCSR(ei, N, validate=False)
    w_csr = g.gather_weights(tw)
    sched = _gdc_schedule(method, alpha, t, tol)
    return _gdc_run(N, lambda j0, nc: diffusion_block(g, w_csr, j0, nc, sched, seed=seed), topk_cols, sparsification,
                    int(k), float(threshold), dense, int(block), dev)


def gdc_torch(edge_index, w, N, method='ppr', alpha=0.05, t=3.0, self_loop_weight=1.0, sparsification='topk', k=64,
              threshold=0.01, tol=1e-6, dense=False, max_bytes=GDC_MAX_BYTES, block=GDC_BLOCK):
    """gdc restated in torch ops on any device (the host tests' path and the baseline of
    tools/gdc_bench.py): the same schedules with torch.sparse.mm products in fp32, the
    selection by topk_cols_torch.  The summation orders are torch's, not the kernels'."""
    N = int(N)
    _gdc_check(N, sparsification, k, dense, max_bytes)
    row, col, val = gdc_matrix(edge_index, w, N, self_loop_weight, remaining=dense)
    dev = val.device
    deg = torch.zeros(N, dtype=torch.float32, device=dev).index_add_(0, col, val)
    fac = deg.pow(-0.5)
    fac = torch.where(torch.isinf(fac), torch.zeros_like(fac), fac)
    T = torch.sparse_coo_tensor(torch.stack([row, col]), fac[row] * val * fac[col], (N, N)).coalesce()
    sched = _gdc_schedule(method, alpha, t, tol)
    return _gdc_run(N, lambda j0, nc: diffusion_block_torch(T, j0, nc, sched), topk_cols_torch, sparsification,
                    int(k), float(threshold), dense, int(block), dev)


# --------------------------------------------------------------------------- positional-encoding distances
# (pos_enc_knn rewiring: csrc/posdist.hip; the contract is in gnpde.graph_rewiring's docstring)
POSDIST_MAX_BYTES = GDC_MAX_BYTES  # the dense fp32 [N, N] matrix of the torch restatements
POSDIST_MAX_EDGES = (1 << 31) * 16  # pair_threshold_edges: edges of one edge list
POINCARE_EPS = 2.0 ** -52  # float64 eps, the reference's clamp of 1 - |x|^2
_METRICS = {'euclid': _lib.METRIC_EUCLID, 'euclidean': _lib.METRIC_EUCLID, 'poincare': _lib.METRIC_POINCARE,
            'hyperbolic': _lib.METRIC_POINCARE, _lib.METRIC_EUCLID: _lib.METRIC_EUCLID,
            _lib.METRIC_POINCARE: _lib.METRIC_POINCARE}


def _metric(metric, name):
    try:
        return _METRICS[metric.lower() if isinstance(metric, str) else metric]
    except KeyError:
        raise ValueError("%s: metric %r ('euclid' | 'poincare')" % (name, metric))


def pair_rank(N, quant):
    """(lo, hi, frac): numpy.quantile's position among M = N^2 sorted values for the linear
    method — its virtual index (M - 1) q, one float64 product (M - 1 is exact in float64 for
    N <= 2^26), lo = floor, hi = min(lo + 1, M - 1), frac = index - lo (0 when hi == lo).  Pure host arithmetic in Python ints and floats."""
    N, q = int(N), float(quant)
    if N < 1:
        raise ValueError("pair_rank: N=%d must be >= 1" % N)
    if not 0.0 <= q <= 1.0:     # (a NaN fails both comparisons)
        raise ValueError("pair_rank: quantile %r outside [0, 1]" % (quant,))
    M = N * N
    pos = float(M - 1) * q
    lo = min(max(int(math.floor(pos)), 0), M - 1)
    hi = min(lo + 1, M - 1)
    frac = pos - math.floor(pos) if hi > lo else 0.0
    return lo, hi, frac


def pair_dist_from_u(u, metric):
    """The distance of a rank value, in float64: sqrt(u) (euclid) or arccosh(1 + 2u) =
    log1p(2u + 2 sqrt(u (u + 1))) (poincare)."""
    u = u.double()
    if _metric(metric, "pair_dist_from_u") == _lib.METRIC_EUCLID:
        return torch.sqrt(u)
    return torch.log1p(2.0 * u + 2.0 * torch.sqrt(u * (u + 1.0)))


def _quantile_lerp(a, b, frac):
    """numpy's _lerp of two float64 scalars (frac a host float)."""
    if frac == 0.0:
        return a
    d = b - a
    return b - d * (1.0 - frac) if frac >= 0.5 else a + d * frac


def _pos_r(x, metric):
    """r of the rank value u_ij = d_ij r_i r_j for the rows of x [..., N, C]: fp32 [..., N]; |x|^2,
    1 - |x|^2 and the reciprocal in float64, one rounding to fp32 (as the pre-pass of
    csrc/posdist.hip)."""
    if metric == _lib.METRIC_EUCLID:
        return torch.ones(x.shape[:-1], dtype=torch.float32, device=x.device)
    q = (x.double() ** 2).sum(-1)
    return (1.0 / torch.clamp_min(1.0 - q, POINCARE_EPS)).float()


def _pair_u_rows(x, r, r0, r1):
    """fp32 rank values u [r1 - r0, N] of the rows r0 .. r1 of one graph x [N, C]; NaN -> +inf."""
    d = ((x[r0:r1, None, :] - x[None, :, :]) ** 2).sum(-1)
    u = d * (r[r0:r1, None] * r[None, :])
    return torch.where(torch.isnan(u), torch.full_like(u, float("inf")), u)


def pos_knn_torch(x, k, metric, return_dist=False, chunk_bytes=None):
    """gnpde_pos_knn_f32 restated in torch ops (any device; chunked over query rows): the k
    smallest (u, j) keys of every row in ascending order, only rows with a non-finite value
    masked (they return themselves; an all-zero row is the origin).  -> (idx int32 [B, N, k],
    n_valid int32 [B]) or (idx, dist fp32 [B, N, k], n_valid), dist the distance itself."""
    x = _knn_input(x, "pos_knn_torch")
    m = _metric(metric, "pos_knn_torch")
    k = int(k)
    B, N, C = x.shape
    if k < 1:
        raise ValueError("pos_knn_torch: k=%d must be >= 1" % k)
    if k > N:
        raise ValueError("pos_knn_torch: k=%d exceeds the %d rows of a graph" % (k, N))
    dev = x.device
    masked = ~torch.isfinite(x).all(dim=-1)
    n_valid = (~masked).sum(dim=1).to(torch.int32)
    xs = torch.where(masked.unsqueeze(-1), torch.zeros_like(x), x)
    r = _pos_r(xs, m)
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=dev) if return_dist else None
    j = torch.arange(N, dtype=torch.int64, device=dev)
    none = torch.iinfo(torch.int64).max
    rows = max(1, min(N, int(chunk_bytes or KNN_TORCH_BYTES) // max(1, 4 * N * C)))
    for b in range(B):
        for r0 in range(0, N, rows):
            r1 = min(N, r0 + rows)
            u = _pair_u_rows(xs[b], r[b], r0, r1)
            key = (u.view(torch.int32).to(torch.int64) << 32) | j
            key = torch.where(masked[b].unsqueeze(0), torch.full_like(key, none), key)
            top = torch.topk(key, k, dim=1, largest=False, sorted=True).values
            pad = top == none
            idx[b, r0:r1] = torch.where(pad, torch.full_like(top, -1), top & 0xFFFFFFFF).to(torch.int32)
            if return_dist:
                uu = (top >> 32).to(torch.int32).view(torch.float32)
                dd = pair_dist_from_u(uu, m).float()
                dist[b, r0:r1] = torch.where(pad, torch.full_like(dd, float("inf")), dd)
        own = torch.arange(N, dtype=torch.int32, device=dev).unsqueeze(1).expand(N, k)
        idx[b] = torch.where(masked[b].unsqueeze(1), own, idx[b])
        if return_dist:
            dist[b] = torch.where(masked[b].unsqueeze(1), torch.zeros_like(dist[b]), dist[b])
    return (idx, dist, n_valid) if return_dist else (idx, n_valid)


def pos_knn(x, k, metric, return_dist=False):
    """gnpde_pos_knn_f32: the k nearest rows of every row of x [B, N, C] (or [N, C]: B = 1, device
    fp32) within its graph under ``metric`` ('euclid' | 'poincare'), in ascending (u, j), the self
    index included.  Returns (idx int32 [B, N, k], n_valid int32 [B]) or (idx, dist fp32 [B, N, k],
    n_valid), dist the distance itself (sqrt(u) | arccosh(1 + 2u)); nothing is read back here.
    Only a row with a non-finite value is masked (never a neighbour, returns its own index).
    1 <= k <= 64 (the kernel's range), k <= N."""
    x = _knn_input(x, "pos_knn")
    _require_gpu(x, "x", torch.float32)
    m = _metric(metric, "pos_knn")
    x = x.contiguous()
    k = int(k)
    B, N, C = x.shape
    if k < 1:
        raise ValueError("pos_knn: k=%d must be >= 1" % k)
    if k > N:
        raise ValueError("pos_knn: k=%d exceeds the %d rows of a graph" % (k, N))
    if k > KNN_MAX_K:
        raise ValueError("pos_knn: k=%d outside the kernel's range (1 <= k <= %d)" % (k, KNN_MAX_K))
    dev = x.device
    idx = torch.empty(B, N, k, dtype=torch.int32, device=dev)
    dist = torch.empty(B, N, k, dtype=torch.float32, device=dev) if return_dist else None
    n_valid = torch.empty(B, dtype=torch.int32, device=dev)
    ws = torch.empty(int(_lib.fn("gnpde_pos_knn_workspace_bytes")(B, N)), dtype=torch.uint8, device=dev)
    _lib.call("gnpde_pos_knn_f32", _ptr(x), B, N, C, C, k, m, _ptr(idx), _ptr(dist), _ptr(n_valid), _ptr(ws),
              _stream(dev))
    return (idx, dist, n_valid) if return_dist else (idx, n_valid)


def _pair_input(x, name):
    x = _knn_input(x, name)
    if x.shape[0] != 1:
        raise NotImplementedError("%s: one graph (B = 1), got B = %d: the edge counts differ per graph"
                                  % (name, x.shape[0]))
    return x[0]


def _pair_dense_u(x, m, max_bytes, name):
    N, C = x.shape
    if 4 * N * N > int(max_bytes):
        raise ValueError("%s: the dense [%d, %d] matrix takes %d bytes, above max_bytes=%d"
                         % (name, N, N, 4 * N * N, int(max_bytes)))
    r = _pos_r(x, m)
    u = torch.empty(N, N, dtype=torch.float32, device=x.device)
    rows = max(1, min(N, KNN_TORCH_BYTES // max(1, 4 * N * C)))
    for r0 in range(0, N, rows):
        u[r0:r0 + rows] = _pair_u_rows(x, r, r0, min(N, r0 + rows))
    return u


def pair_quantile_torch(x, quant, metric, max_bytes=POSDIST_MAX_BYTES):
    """pair_quantile restated in torch ops on any device, on the dense fp32 [N, N] rank values
    (at most max_bytes, else ValueError): -> (thr float64 scalar, u_lo fp32 scalar, count_le
    int64 scalar)."""
    x = _pair_input(x, "pair_quantile_torch")
    m = _metric(metric, "pair_quantile_torch")
    lo, hi, frac = pair_rank(x.shape[0], quant)
    flat = _pair_dense_u(x, m, max_bytes, "pair_quantile_torch").reshape(-1)
    u_lo = torch.kthvalue(flat, lo + 1).values
    u_hi = torch.kthvalue(flat, hi + 1).values if (hi > lo and frac != 0.0) else u_lo
    thr = _quantile_lerp(pair_dist_from_u(u_lo, m), pair_dist_from_u(u_hi, m), frac)
    return thr, u_lo, (flat <= u_lo).sum()


def pair_threshold_edges_torch(x, quant, metric, max_bytes=POSDIST_MAX_BYTES):
    """pair_threshold_edges restated in torch ops on any device (dense, at most max_bytes)."""
    x = _pair_input(x, "pair_threshold_edges_torch")
    m = _metric(metric, "pair_threshold_edges_torch")
    lo = pair_rank(x.shape[0], quant)[0]
    if not bool(torch.isfinite(x).all()):
        raise ValueError("pair_threshold_edges_torch: x holds a non-finite value")
    u = _pair_dense_u(x, m, max_bytes, "pair_threshold_edges_torch")
    u_lo = torch.kthvalue(u.reshape(-1), lo + 1).values
    return torch.nonzero(u <= u_lo).t().contiguous()


def _pair_ws(x):
    N = x.shape[0]
    nbytes = int(_lib.fn("gnpde_pair_workspace_bytes")(N))
    return torch.empty(nbytes, dtype=torch.uint8, device=x.device), nbytes


def _pair_gpu_input(x, metric, name):
    x = _pair_input(x, name)
    _require_gpu(x, "x", torch.float32)
    return x.contiguous(), _metric(metric, name)


def pair_select(x, rank, metric, ws=None):
    """gnpde_pair_select_f32: (u fp32 [1], count_le int64 [1]) on the device — the rank value of
    0-based rank ``rank`` among the N^2 entries of one graph x [N, C], and the number of entries
    <= it.  Nothing is read back."""
    x, m = _pair_gpu_input(x, metric, "pair_select")
    N, C = x.shape
    rank = int(rank)
    if not 0 <= rank < N * N:
        raise ValueError("pair_select: rank=%d must be in [0, N^2=%d)" % (rank, N * N))
    buf, nbytes = ws if ws is not None else _pair_ws(x)
    u = torch.empty(1, dtype=torch.float32, device=x.device)
    cnt = torch.empty(1, dtype=torch.int64, device=x.device)
    _lib.call("gnpde_pair_select_f32", _ptr(x), N, C, C, m, rank, _ptr(u), _ptr(cnt), _ptr(buf), nbytes,
              _stream(x.device))
    return u, cnt


def pair_quantile(x, quant, metric):
    """numpy.quantile(D, quant) over all N^2 pairwise distances of x [N, C] (device fp32; linear
    interpolation) without the matrix: -> (thr float64 device scalar, u_lo fp32 [1], count_le
    int64 [1]), u_lo the rank value of position lo = floor(quant (N^2 - 1)) and count_le the
    number of entries <= it ({D <= thr} = {u <= u_lo}).  One select for lo and, when the position
    is fractional, one for lo + 1; nothing is read back."""
    x, m = _pair_gpu_input(x, metric, "pair_quantile")
    lo, hi, frac = pair_rank(x.shape[0], quant)
    ws = _pair_ws(x)
    u_lo, cnt = pair_select(x, lo, m, ws)
    u_hi = pair_select(x, hi, m, ws)[0] if (hi > lo and frac != 0.0) else u_lo
    thr = _quantile_lerp(pair_dist_from_u(u_lo[0], m), pair_dist_from_u(u_hi[0], m), frac)
    return thr, u_lo, cnt


def pair_threshold_edges(x, quant, metric):
    """Every pair (i, j) of x [N, C] (device fp32, one graph) whose distance is at most
    numpy.quantile of all N^2 distances at ``quant``: edge_index int64 [2, E] in numpy.where
    order (i ascending, j ascending within i).  One select, a count pass, torch's cumsum and a
    fill pass; one host read (E, with the non-finite check) to allocate.  A non-finite value in
    x, or E >= 2^35, raises ValueError."""
    x, m = _pair_gpu_input(x, metric, "pair_threshold_edges")
    N, C = x.shape
    dev = x.device
    lo = pair_rank(N, quant)[0]
    ws = _pair_ws(x)
    u_lo, _cnt = pair_select(x, lo, m, ws)
    row_ptr = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    row_count = row_ptr[1:]
    _lib.call("gnpde_pair_threshold_count_f32", _ptr(x), N, C, C, m, _ptr(u_lo), _ptr(row_count), _ptr(ws[0]), ws[1],
              _stream(dev))
    row_count.cumsum_(0)     # row_ptr: the exclusive scan, row_ptr[N] the total
    bad = (~torch.isfinite(x)).sum()
    E, nbad = torch.stack([row_ptr[N], bad]).tolist()   # the host read
    if nbad:
        raise ValueError("pair_threshold_edges: x holds %d non-finite values" % nbad)
    if E >= POSDIST_MAX_EDGES:
        raise ValueError("pair_threshold_edges: %d edges, above the limit of %d" % (E, POSDIST_MAX_EDGES))
    ei = torch.empty(2, E, dtype=torch.int64, device=dev)
    _lib.call("gnpde_pair_threshold_fill_f32", _ptr(x), N, C, C, m, _ptr(u_lo), _ptr(row_ptr), E, _ptr(ei),
              _ptr(ws[0]), ws[1], _stream(dev))
    return ei


class PosDistBackend(object):
    """The two searches gnpde.graph_rewiring's positional-distance rewiring runs on."""

    def __init__(self, pos_knn, threshold_edges):
        self.pos_knn = pos_knn
        self.threshold_edges = threshold_edges


POSDIST_HIP = PosDistBackend(pos_knn, pair_threshold_edges)
POSDIST_TORCH = PosDistBackend(pos_knn_torch, pair_threshold_edges_torch)
