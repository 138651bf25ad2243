"""Float64 references of the backward kernels, one per kernel, and the inputs the
GPU tests feed them (tests/test_gpu_backward_kernels.py; checked on the host by
tests/test_backward_oracle_host.py).

Every reference restates the formula of its kernel's header comment
(csrc/backward.hip, csrc/score_backward.hip, csrc/gat.hip) in numpy float64, or in
torch CPU float64 where autograd is the simplest honest statement; none reads device
code.  Graphs are [B,2,E] edge lists of B graphs on N nodes each; a "group" is the
set of edges of one (graph, node) pair under one endpoint (0 = source, 1 =
destination), numbered b*N + node as the grouped CSR numbers its rows; per-edge
arrays are in COO order, flattened [B*E, ...] where noted.
"""
import numpy as np
import torch

EPS32 = 2.0 ** -23   # spacing of fp32 at 1: one rounding is within EPS32/2 relative
EPS64 = 2.0 ** -52

RTOL = 1e-5          # the project's forward bar (tests/test_gpu_parity.py)
GTOL = 1e-4          # the project's gradient bar (tests/test_gpu_backward.py)

MODES = {"scaled_dot": 1, "exp_kernel": 2, "cosine_sim": 3, "pearson": 4}   # gnpde._lib.SCORE_*


# ============================================================================ graphs
UNIT_B, UNIT_N, UNIT_E = 2, 97, 1009
GROUP_SIZES = (0, 1, 63, 64, 65, 200)     # around the 64-lane stride of one wavefront, and a long one
SRC_NODES = (0, 1, 2, 3, 4, 5)            # source nodes holding exactly GROUP_SIZES edges
DST_NODES = (10, 11, 12, 13, 14, 15)      # destination nodes holding exactly GROUP_SIZES edges


def unit_graph(seed=0):
    """[B,2,E] int64, B = 2, N = 97, E = 1009 (prime): on the source and on the
    destination side of both graphs, groups of exactly 0, 1, 63, 64, 65 and 200
    edges (constructed: SRC_NODES / DST_NODES), the other edges spread over the
    other nodes, COO order shuffled."""
    rng = np.random.default_rng(seed)
    B, N, E = UNIT_B, UNIT_N, UNIT_E
    n_special = sum(GROUP_SIZES)
    ei = np.empty((B, 2, E), np.int64)
    for b in range(B):
        for side, nodes in ((0, SRC_NODES), (1, DST_NODES)):
            other = np.setdiff1d(np.arange(N), np.asarray(nodes))
            ends = np.concatenate([np.repeat(np.asarray(nodes), GROUP_SIZES), rng.choice(other, E - n_special)])
            ei[b, side] = rng.permutation(ends)
    for b in range(B):
        for side, nodes in ((0, SRC_NODES), (1, DST_NODES)):
            cnt = np.bincount(ei[b, side], minlength=N)
            assert tuple(cnt[list(nodes)]) == GROUP_SIZES
    return ei


def groups_of(ei, N, side):
    """[B*E] int64: the group b*N + ei[b, side, e] of every edge, COO order."""
    B = ei.shape[0]
    return (ei[:, side, :] + N * np.arange(B)[:, None]).reshape(-1)


def longest_group_last_edge(gidx):
    """(group, COO id of its last edge in COO order) of the longest group."""
    cnt = np.bincount(gidx)
    r = int(np.argmax(cnt))
    return r, int(np.nonzero(gidx == r)[0][-1])


# ============================================================================ references
def sddmm(ei, gf, x, a, H):
    """g_w[b,e] = a/H <gf[b,src(e)], x[b,dst(e)]>: [B,E] (H = 1) or the same value on every
    head [B,E,H] (the weights were a head mean)."""
    gf, x = np.asarray(gf, np.float64), np.asarray(x, np.float64)
    B = ei.shape[0]
    out = np.stack([np.einsum('ec,ec->e', gf[b][ei[b, 0]], x[b][ei[b, 1]]) for b in range(B)]) * (float(a) / H)
    return out if H == 1 else np.repeat(out[:, :, None], H, axis=2)


def softmax_backward(group_idx, att, g):
    """g_s[e,h] = att[e,h] (g[e,h] - sum_{e' in group(e)} att[e',h] g[e',h]);  att, g [M,H]."""
    att, g = np.asarray(att, np.float64), np.asarray(g, np.float64)
    d = segment_sum(group_idx, att * g, int(group_idx.max()) + 1)
    return att * (g - d[group_idx])


def segment_sum(group_idx, vals, R):
    """out[r,h] = sum of vals[e,h] over the edges of group r;  vals [M,H] -> [R,H] (empty groups 0)."""
    vals = np.asarray(vals, np.float64)
    out = np.zeros((R, vals.shape[1]), np.float64)
    np.add.at(out, group_idx, vals)
    return out


def wcolsum(x, w):
    """y[b,h,c] = sum_n w[b,n,h] x[b,n,c] for c < C and y[b,h,C] = sum_n w[b,n,h];  -> [B,H,C+1]."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    return np.concatenate([np.einsum('bnh,bnc->bhc', w, x), w.sum(1)[:, :, None]], axis=2)


def score_input_grad(gcs, U, deg, gxbar, gx0=None, dtype=np.float32):
    """gx[b,n,c] = sum_h gcs[b,n,h] U[b,c,h] + deg[b,n] gxbar[b,c], rounded to fp32; with gx0
    (the kernel accumulating into an existing fp32 output) float32(float64(gx0) + that sum).
    dtype=np.float64 keeps the unrounded sum."""
    s = np.einsum('bnh,bch->bnc', np.asarray(gcs, np.float64), np.asarray(U, np.float64))
    s = s + np.asarray(deg, np.float64)[:, :, None] * np.asarray(gxbar, np.float64)[:, None, :]
    if gx0 is not None:
        s = np.asarray(gx0, np.float64) + s
    return s.astype(dtype)


def edge_scores(src, dst_k, mode, dk, p0=1.0, p1=1.0):
    """prods [..., E, h] from src, dst_k [..., E, d_k, h] as src/function_transformer_attention.py:
    246-259 writes them (torch, any float type and device).  scaled_dot is the per-edge form
    q.k / sqrt(d_k) that the kernel's header states (SCORE_DOT; the fork's :249 sums the keys of
    every edge first, which is the project's separate 'reference' mode and no per-edge score)."""
    if mode == "exp_kernel":
        return p0 ** 2 * torch.exp(-(torch.sum((src - dst_k) ** 2, dim=-2) / (2 * p1 ** 2)))
    if mode == "scaled_dot":
        return torch.sum(src * dst_k, dim=-2) / dk ** 0.5
    if mode == "pearson":
        src = src - torch.mean(src, dim=-2, keepdim=True)
        dst_k = dst_k - torch.mean(dst_k, dim=-2, keepdim=True)
    elif mode != "cosine_sim":
        raise ValueError(mode)
    return torch.nn.CosineSimilarity(dim=-2, eps=1e-5)(src, dst_k)


def _gather_qk(ei, N, q, k, H, dk):
    """src, dst_k [B*E, d_k, h] of q, k [B*N, h*d_k] (:230-244: view (h, d_k), transpose, gather)."""
    B = ei.shape[0]
    gs_, gd_ = (torch.from_numpy(groups_of(ei, N, s)) for s in (0, 1))
    qv = q.view(B * N, H, dk).transpose(1, 2)
    kv = k.view(B * N, H, dk).transpose(1, 2)
    return qv[gs_], kv[gd_]


def score_values(ei, N, q, k, mode, H, dk, p0=1.0, p1=1.0):
    """The scores s [B*E, H] themselves in float64 (numpy)."""
    q64, k64 = (torch.from_numpy(np.asarray(a, np.float64)) for a in (q, k))
    src, dst_k = _gather_qk(ei, N, q64, k64, H, dk)
    return edge_scores(src, dst_k, mode, dk, p0, p1).numpy()


def score_grad(ei, q, k, gs, mode, H, dk, p0=1.0, p1=1.0, N=None):
    """(gq, gk, g_ov, g_ls) = d L / d (q, k, output_var, lengthscale) of L = sum gs * s by torch
    float64 autograd;  q, k [B*N, H*dk], gs [B*E, H] (COO)."""
    B = ei.shape[0]
    N = q.shape[0] // B if N is None else N
    q64 = torch.from_numpy(np.array(q, np.float64)).requires_grad_(True)
    k64 = torch.from_numpy(np.array(k, np.float64)).requires_grad_(True)
    ov = torch.tensor(float(p0), dtype=torch.float64, requires_grad=True)
    ls = torch.tensor(float(p1), dtype=torch.float64, requires_grad=True)
    src, dst_k = _gather_qk(ei, N, q64, k64, H, dk)
    s = edge_scores(src, dst_k, mode, dk, ov, ls)
    L = (torch.from_numpy(np.asarray(gs, np.float64)) * s).sum()
    if mode == "exp_kernel":
        gq, gk, gov, gls = torch.autograd.grad(L, (q64, k64, ov, ls))
        return gq.numpy(), gk.numpy(), float(gov), float(gls)
    gq, gk = torch.autograd.grad(L, (q64, k64))
    return gq.numpy(), gk.numpy(), 0.0, 0.0


def score_grad_closed(ei, q, k, gs, mode, H, dk, side, p0=1.0, p1=1.0, drop_own=False):
    """The same gradient for one side (0: d/dq, 1: d/dk) in closed form, as the kernel's header
    states it:  g[r, h, :] = own' sum_e gs a_own(e) + sum_e gs a_oth(e) oth'(e)  over the edges of
    r's group; ``drop_own`` leaves the a_own term out (what a kernel that forgot it would give)."""
    B = ei.shape[0]
    R = q.shape[0]
    N = R // B
    q, k, gs = (np.asarray(a, np.float64) for a in (q, k, gs))
    qe = q.reshape(R, H, dk)[groups_of(ei, N, 0)]          # [M,H,dk]
    ke = k.reshape(R, H, dk)[groups_of(ei, N, 1)]
    own, oth = (qe, ke) if side == 0 else (ke, qe)
    if mode == "pearson":
        own = own - own.mean(-1, keepdims=True)
        oth = oth - oth.mean(-1, keepdims=True)
    if mode == "scaled_dot":
        a_own = np.zeros(gs.shape)
        a_oth = np.full(gs.shape, dk ** -0.5)
    elif mode == "exp_kernel":
        s = p0 ** 2 * np.exp(-((own - oth) ** 2).sum(-1) / (2 * p1 ** 2))
        a_own, a_oth = -s / p1 ** 2, s / p1 ** 2
    else:
        no = np.maximum(np.sqrt((own ** 2).sum(-1)), 1e-5)
        nt = np.maximum(np.sqrt((oth ** 2).sum(-1)), 1e-5)
        s = (own * oth).sum(-1) / (no * nt)
        a_own, a_oth = -s / no ** 2, 1.0 / (no * nt)
    per_edge = (gs * a_oth)[:, :, None] * oth
    if not drop_own:
        per_edge = per_edge + (gs * a_own)[:, :, None] * own
    out = np.zeros((R, H * dk))
    np.add.at(out, groups_of(ei, N, side), per_edge.reshape(-1, H * dk))
    return out


def gat_score_backward(ei, sp, slope, gs):
    """ge[e,h] = gs[e,h] * (sl[src(e),h] + sr[dst(e),h] > 0 ? 1 : slope), one fp32 product;
    sp [B*N, 2H] float64 = [sl | sr], gs [B*E, H] fp32 -> fp32 [B*E, H]."""
    H = gs.shape[1]
    N = sp.shape[0] // ei.shape[0]
    t = sp[groups_of(ei, N, 0), :H] + sp[groups_of(ei, N, 1), H:]
    return np.asarray(gs, np.float32) * np.where(t > 0.0, np.float32(1.0), np.float32(slope)).astype(np.float32)


def gather_head(order, w, h, scale):
    """scale * w[order, h] in fp32 (one product); ``order``: the COO ids in grouped order."""
    return np.float32(scale) * np.asarray(w, np.float32)[order, h]


# ============================================================================ bars
def rel(got, want):
    """max|got - want| / max|want|: the project's max-over-max error."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def softmax_backward_bar(want, g):
    """fp64 math and one rounding to fp32: 2^-23 |want| elementwise, and 1e-12 max|g| for the
    fp64 group sum (<= 200 terms of at most max|g| in absolute value, each within 2^-53)."""
    return EPS32 * np.abs(want) + 1e-12 * np.abs(np.asarray(g, np.float64)).max()


def segment_sum_bar(group_idx, vals, R):
    """len * 2^-52 * sum|v| per row and head: any order of a len-term fp64 sum."""
    cnt = np.bincount(group_idx, minlength=R).astype(np.float64)
    return cnt[:, None] * EPS64 * segment_sum(group_idx, np.abs(np.asarray(vals, np.float64)), R)


def wcolsum_bar(x, w):
    """N * 2^-52 * sum_n |w x| per output: any order of an N-term fp64 sum of fp64 products."""
    return x.shape[1] * EPS64 * wcolsum(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)))


def score_input_grad_bar(want):
    """One rounding of an fp64 sum to fp32: 2^-23 |want| elementwise plus 2^-23 max|want| 1e-6 of
    absolute slack (the fp64 sum's own error where its terms cancel)."""
    want = np.abs(np.asarray(want, np.float64))
    return EPS32 * want + EPS32 * want.max() * 1e-6


def sum_bar(v):
    """n * 2^-52 * sum|v|: any order of an n-term fp64 sum."""
    v = np.asarray(v, np.float64)
    return v.size * EPS64 * float(np.abs(v).sum())


def exceed(got, want, bar):
    """max over the elements of |got - want| / bar (0/0 counts as 0): <= 1 passes."""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    bar = np.broadcast_to(np.asarray(bar, np.float64), d.shape)
    r = np.where(d == 0.0, 0.0, d / np.where(bar > 0.0, bar, 1e-300))
    return float(r.max()) if r.size else 0.0


# ============================================================================ inputs of the GPU tests
SDDMM_CASES = [(1, C) for C in (5, 12, 13, 20, 27, 64, 80, 128, 162, 256, 260)] + \
              [(8, 12), (8, 128), (16, 12), (64, 20)]
# (heads, C) -> sddmm_kernel<VEC, GL>: (1,5) <1,8>, (1,13) <1,16>, (1,27) <1,32>, (1,162) <1,64> in three
# trips with a partial last one; (1,12) (1,20) <4,8>, (1,64) <4,16>, (1,80) (1,128) <4,32>, (1,256) <4,64>,
# (1,260) <4,64> with a second column trip; (16,12) <4,16> by the heads, (64,20) <4,64> by the heads.
SDDMM_ALPHA = [None, "raw", "sigmoid"]
ALPHA_VALUE = 0.7

SOFTMAX_HEADS = [1, 3, 8]
SEGSUM_HEADS = [1, 8, 16]
WCOLSUM_CASES = [(1, 1000, 80, 8), (3, 257, 162, 1), (2, 300, 5, 2), (300, 3, 12, 1), (1, 1, 128, 2),
                 (1, 500, 300, 2)]
WCOLSUM_REFUSED_C = 8192          # one row of C + 1 doubles is past 64 KiB of LDS
SIG_CASES = [(2, 50, 12, 1), (2, 50, 162, 8), (1, 70, 80, 16)]
GATHER_HEADS = [1, 8]
GATHER_DK = 16
GAT_HEADS = [1, 2, 8]
GAT_SLOPE = 0.2

_ALL = ("scaled_dot", "exp_kernel", "cosine_sim", "pearson")
SCORE_CASES = [(m, H, dk) for m in _ALL for (H, dk) in ((8, 16), (3, 5), (1, 64), (4, 80))] + \
              [(m, 2, 4) for m in ("scaled_dot", "exp_kernel")] + [("scaled_dot", 16, 64)]

SUM_NS = [0, 1, 7, 4096, 1000003]
SEGSUMS_CASES = [(1, 1), (3, 1000003), (9, 4096)]
SQ_NS = [1, 7, 4096, 1000003]
SQ_ATOL, SQ_RTOL = 2.0 ** -12, 2.0 ** -10    # exact in fp32: the kernel takes them as floats


def _rng(*key):
    return np.random.default_rng([int(k) for k in key])


def _mode_id(mode):
    return _ALL.index(mode) if mode in _ALL else 9


def sddmm_inputs(H, C):
    rng = _rng(1, H, C)
    B, N = UNIT_B, UNIT_N
    return (rng.standard_normal((B, N, C)).astype(np.float32), rng.standard_normal((B, N, C)).astype(np.float32))


def alpha_scale(kind):
    """The scalar the kernel multiplies by, in float64."""
    if kind is None:
        return 1.0
    return ALPHA_VALUE if kind == "raw" else 1.0 / (1.0 + np.exp(-ALPHA_VALUE))


def softmax_inputs(ei, side, H):
    """att [B*E,H]: a float64 softmax of random scores over the groups of ``side``, rounded to
    fp32;  g [B*E,H] fp32 random."""
    rng = _rng(2, side, H)
    gidx = groups_of(ei, UNIT_N, side)
    s = rng.standard_normal((gidx.size, H)) * 2.0
    m = np.full((UNIT_B * UNIT_N, H), -np.inf)
    np.maximum.at(m, gidx, s)
    e = np.exp(s - m[gidx])
    att = (e / segment_sum(gidx, e, UNIT_B * UNIT_N)[gidx]).astype(np.float32)
    return att, rng.standard_normal((gidx.size, H)).astype(np.float32)


def segsum_inputs(side, H):
    return _rng(3, side, H).standard_normal((UNIT_B * UNIT_E, H)).astype(np.float32)


def wcolsum_inputs(B, N, C, H):
    rng = _rng(4, B, N, C, H)
    return rng.standard_normal((B, N, C)).astype(np.float32), rng.standard_normal((B, N, H))


def sig_inputs(B, N, C, H):
    """gcs [B,N,H], U [B,C,H], gxbar [B,C] float64, deg [B,N] int32, gx0 [B,N,C] fp32."""
    rng = _rng(5, B, N, C, H)
    return (rng.standard_normal((B, N, H)), rng.standard_normal((B, C, H)),
            rng.integers(0, 40, size=(B, N)).astype(np.int32), rng.standard_normal((B, C)) * 0.1,
            rng.standard_normal((B, N, C)).astype(np.float32))


def gather_inputs(H):
    return _rng(6, H).standard_normal((UNIT_B * UNIT_E, H)).astype(np.float32)


def gat_inputs(ei, H):
    """sp [B*N, 2H] float64 with |sl[src] + sr[dst]| > 1e-6 on every edge and head, gs [B*E,H] fp32."""
    rng = _rng(7, H)
    sp = rng.standard_normal((UNIT_B * UNIT_N, 2 * H))
    t = sp[groups_of(ei, UNIT_N, 0), :H] + sp[groups_of(ei, UNIT_N, 1), H:]
    assert np.abs(t).min() > 1e-6 and (t > 0).any() and (t < 0).any()
    return sp, rng.standard_normal((UNIT_B * UNIT_E, H)).astype(np.float32)


def score_params(mode, dk):
    """(output_var, lengthscale): |q - k|^2 is about dk / 2 for the operands below, so the
    exponent of exp_kernel sits near -1/2 (not near -1, where s |q - k|^2, the lengthscale's
    gradient, is stationary in |q - k|^2 and would not see an error in it)."""
    return (1.3, (0.5 * dk) ** 0.5) if mode == "exp_kernel" else (1.0, 1.0)


def score_inputs(mode, H, dk):
    """q, k [B*N, H*dk] fp32, gs [B*E, H] fp32 (mean 0.3: the parameter gradients, plain sums
    over every edge and head, do not cancel to nothing), p0, p1.  Unit normal operands (halved
    for exp_kernel): dot scores of unit variance, cosines inside (-1, 1)."""
    rng = _rng(8, _mode_id(mode), H, dk)
    sc = 0.5 if mode == "exp_kernel" else 1.0
    R = UNIT_B * UNIT_N
    q = (rng.standard_normal((R, H * dk)) * sc).astype(np.float32)
    k = (rng.standard_normal((R, H * dk)) * sc).astype(np.float32)
    gs = (rng.standard_normal((UNIT_B * UNIT_E, H)) + 0.3).astype(np.float32)
    p0, p1 = score_params(mode, dk)
    return q, k, gs, np.float32(p0).item(), np.float32(p1).item()


def min_head_norm(q, k, mode, H, dk):
    """Smallest per-head norm of the (pearson: centred) operands: the eps clamp of the cosine
    is inactive above 1e-5."""
    out = np.inf
    for a in (q, k):
        v = np.asarray(a, np.float64).reshape(-1, H, dk)
        if mode == "pearson":
            v = v - v.mean(-1, keepdims=True)
        out = min(out, float(np.sqrt((v ** 2).sum(-1)).min()))
    return out


def sum_inputs(n):
    return _rng(9, n).standard_normal(n)


def segsums_inputs(nseg, ln):
    return _rng(10, nseg, ln).standard_normal((nseg, ln))


def sq_inputs(n):
    rng = _rng(11, n)
    return tuple(rng.standard_normal(n).astype(np.float32) for _ in range(3))


def scaled_sq_sums(y0, f0, f1, atol, rtol):
    """f1 None: (sum (y0/sc)^2, sum (f0/sc)^2); else sum ((f1 - f0)/sc)^2;  sc = atol + |y0| rtol."""
    y0, f0 = np.asarray(y0, np.float64), np.asarray(f0, np.float64)
    sc = atol + np.abs(y0) * rtol
    if f1 is None:
        return float(((y0 / sc) ** 2).sum()), float(((f0 / sc) ** 2).sum())
    return float((((np.asarray(f1, np.float64) - f0) / sc) ** 2).sum())
