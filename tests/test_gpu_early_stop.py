"""GPU: the early-stop test integrator (gnpde.early_stop_solver) and its score kernel
(gnpde_decode_score_f32, csrc/early_stop.hip).

Kernel: ops.decode_score against numpy on integer-valued data (y in {-3..3}, W in
{-2..2}, b in {-1, 0, 1}): every logit is exact in fp32 and ties are frequent, so
predictions and counts must equal np.argmax's exactly.

Solve: a synthetic graph (N = 300, mean degree 8, width 16, 5 classes, B = 1 and 2)
under the Laplacian and the transformer attention function against the float64
restatement of tests/early_stop_oracle.py.  The problems (T, earlystopxT, tol_scale,
seed) were chosen on the CPU with that oracle, and the test asserts what they were chosen
for: at least 8 accepted and 1 rejected step, validation labels (the oracle's predictions
at a middle accepted step) giving a unique strict maximum of the validation accuracy at a
step that is neither first nor last, and at most 2 % undecided rows per step.  A row is
undecided when its oracle top-2 logit margin is within
    delta = 2 (1e-5 max_c ||W_c||_1 + Cd 2^-24 max_c sum_j |W_cj z_j|):
the project's 1e-5 state parity bar carried through the decoder, the fp32 dot's rounding,
twice because both top logits move.  Step times are held to 1e-5 relative, the end-to-end
tests' bar for integrated values: a step size is the previous one times ratio^(-1/5), so it
is no less accurate than the error norm of states that meet that bar."""
import ctypes
import types

import numpy as np
import pytest
import torch

import early_stop_oracle as EO
import gnpde
import gnpde_oracle as O
from gnpde import _lib, integrator as gi, ops
from gnpde.early_stop_solver import EarlyStopInt
from test_gpu_parity import DEV, OPT, T, make_laplacian, make_transformer, rel

pytestmark = pytest.mark.gpu

SPLITS = np.array([0, 1, 2, 4, 3, 7], np.uint8)


# --------------------------------------------------------------------------- the kernel
def _score_case(rng, R, ld, Cd, K, split):
    y = rng.integers(-3, 4, (R, ld)).astype(np.float32)
    W = rng.integers(-2, 3, (K, Cd)).astype(np.float32)
    b = rng.integers(-1, 2, K).astype(np.float32)
    label = rng.integers(0, K, R).astype(np.int32)
    logits = np.maximum(y[:, :Cd], 0).astype(np.float64) @ W.T.astype(np.float64) + b
    assert np.abs(logits).max() < 2 ** 20  # exact in fp32 whatever the order
    return y, W, b, label, logits.argmax(1)


def _check_score(y, W, b, split, label, pred, rows, with_pred, start):
    R = y.shape[0]
    sp, lb = (split[rows], label[rows]) if rows is not None else (split, label)
    want = [start[k] + int(((pred == lb) & (((sp >> k) & 1) == 1)).sum()) for k in range(3)]
    counts = T(np.array(start, np.int32))
    pred_out = torch.full((R,), -7, dtype=torch.int32, device=DEV) if with_pred else None
    ops.decode_score(T(y), T(W), T(b), T(split), T(label), counts, ld=y.shape[1],
                     rows=T(rows) if rows is not None else None, pred_out=pred_out)
    assert counts.tolist() == want, (R, y.shape[1], W.shape, rows is not None, counts.tolist(), want)
    if with_pred:
        np.testing.assert_array_equal(pred_out.cpu().numpy(), np.where(sp != 0, pred, -1))


@pytest.mark.parametrize("K", [2, 7, 40, 70])
def test_decode_score_exact(K):
    """Every R x ld x Cd of the issue's table (one row, one short of / exactly / one past a
    wavefront, several tiles; a decoder on the whole state and on its first half) under a
    mixed split pattern, with and without ``rows`` and ``pred_out``, into non-zero counts."""
    rng = np.random.default_rng(100 + K)
    for R in (1, 63, 64, 65, 257):
        for ld in (4, 80, 162):
            for Cd in (ld, ld // 2):
                split = rng.choice(SPLITS, R).astype(np.uint8)
                y, W, b, label, pred = _score_case(rng, R, ld, Cd, K, split)
                rows = rng.permutation(R).astype(np.int32)
                for use_rows, with_pred in ((False, True), (True, False), (True, True), (False, False)):
                    _check_score(y, W, b, split, label, pred, rows if use_rows else None, with_pred, (3, 0, 11))


@pytest.mark.parametrize("value", [0, 1, 2, 4, 3, 7])
def test_decode_score_uniform_splits(value):
    """All rows unscored, in one split, in two and in all three."""
    rng = np.random.default_rng(value)
    R, ld, K = 257, 80, 7
    split = np.full(R, value, np.uint8)
    y, W, b, label, pred = _score_case(rng, R, ld, ld, K, split)
    label[::3] = pred[::3]  # hits for certain
    _check_score(y, W, b, split, label, pred, None, True, (0, 5, 0))
    _check_score(y, W, b, split, label, pred, rng.permutation(R).astype(np.int32), True, (1, 1, 1))


def test_decode_score_unscored_rows_are_not_read():
    """A row outside every split costs no state read: NaN there changes nothing."""
    rng = np.random.default_rng(9)
    R, ld, K = 65, 80, 7
    split = rng.choice(SPLITS, R).astype(np.uint8)
    y, W, b, label, pred = _score_case(rng, R, ld, ld, K, split)
    y[split == 0] = np.nan
    _check_score(y, W, b, split, label, pred, None, True, (0, 0, 0))


def test_decode_score_wide_decoder_tiles_and_fallback():
    """The widest supported decoder (K = 128, Cd = 512: several column chunks) in the
    kernel, and one past it through the torch restatement — the same exact counts."""
    rng = np.random.default_rng(12)
    for K, Cd in ((128, 512), (129, 16), (5, 513)):
        R = 65
        split = rng.choice(SPLITS, R).astype(np.uint8)
        y, W, b, label, pred = _score_case(rng, R, Cd, Cd, K, split)
        label[::2] = pred[::2]
        _check_score(y, W, b, split, label, pred, rng.permutation(R).astype(np.int32), True, (2, 0, 0))


def check_abi_errors():
    """The argument errors of gnpde_decode_score_f32 (host-side validation: nothing is
    launched, so the pointers are never read)."""
    lib = _lib.load()
    vp = ctypes.c_void_p
    P = vp(4096)

    def call(R=8, ld=16, Cd=16, K=5, y=P, W=P, split=P, label=P, counts=P):
        return lib.gnpde_decode_score_f32(y, R, ld, Cd, W, P, K, split, label, vp(0), counts, vp(0), vp(0))
    assert call(Cd=17) == -1 and b"Cd" in lib.gnpde_last_error()
    assert call(Cd=0) == -1
    assert call(K=0) == -1 and b"K=" in lib.gnpde_last_error()
    assert call(R=-1) == -1
    for null in ("y", "W", "split", "label", "counts"):
        assert call(**{null: vp(0)}) == -1 and b"NULL" in lib.gnpde_last_error(), null
    assert call(K=129) == -3 and b"K <= 128" in lib.gnpde_last_error()
    assert call(ld=600, Cd=513) == -3
    assert call(K=129, Cd=17) == -1  # a bad argument before an unsupported one
    assert call(R=0, y=vp(0), split=vp(0), label=vp(0)) == 0  # nothing to score


def test_decode_score_argument_errors():
    check_abi_errors()


# --------------------------------------------------------------------------- the solve
N_NODES, N_EDGES, WIDTH, CLASSES = 300, 2400, 16, 5
# (kind, B) -> T, earlystopxT, tol_scale, seed: chosen on the CPU with the oracle (module docstring)
PROBLEMS = {('laplacian', 1): (6.0, 5.0, 10000.0, 3), ('laplacian', 2): (6.0, 5.0, 10000.0, 1),
            ('transformer', 1): (8.0, 5.0, 3000.0, 4), ('transformer', 2): (8.0, 5.0, 3000.0, 1)}
RK4_T = 1.2  # the rk4 case's horizon: six steps of 1.0 over [0, earlystopxT * 1.2] (inside rk4's stability range)
ALPHA = 0.3
_CACHE = {}


class Problem(object):
    pass


def build_problem(kind, B, width=WIDTH, Cd=WIDTH, seed=None):
    """The problem's arrays, its oracle RHS and the early-stop oracle's result (CPU only;
    computed once and shared)."""
    key = (kind, B, width, Cd, seed)
    if key in _CACHE:
        return _CACHE[key]
    Tt, xT, ts, seed0 = PROBLEMS[(kind, B)]
    seed = seed0 if seed is None else seed
    rng = np.random.default_rng(seed)
    p = Problem()
    p.kind, p.B, p.T, p.xT, p.tol_scale = kind, B, Tt, xT, ts
    p.t_end = float(np.float32(xT * Tt))
    p.atol, p.rtol = ts * 1e-7, ts * 1e-9  # ODEblock.set_tol
    src = rng.integers(0, N_NODES, size=(B, N_EDGES - N_NODES))
    dst = (src + 1 + rng.integers(0, N_NODES - 1, size=src.shape)) % N_NODES  # no self loops: N are added per graph
    raw = np.stack([src, dst], 1)
    eis, ws = O.get_rw_adj(raw, norm_dim=1, fill_value=1.0, num_nodes=N_NODES)
    p.ei, p.w = np.stack(eis, 0), np.stack(ws, 0)
    p.y0 = rng.standard_normal((B, N_NODES, width)).astype(np.float32)
    p.W = rng.standard_normal((CLASSES, Cd)).astype(np.float32)
    p.b = (rng.standard_normal(CLASSES) * 0.5).astype(np.float32)
    R = B * N_NODES
    part = rng.integers(0, 4, R)  # 0: in no split
    p.masks = [part == 1, part == 2, part == 3]
    if kind == 'laplacian':
        p.f = lambda t, y: O.laplacian_rhs(p.ei, y, None, ALPHA, 0.0, edge_weight=p.w)
    else:
        h, att = 2, 8
        p.proj = [(rng.standard_normal((att, width)) * 0.2).astype(np.float32), (rng.standard_normal(att) * 0.1).astype(
            np.float32), (rng.standard_normal((att, width)) * 0.2).astype(np.float32),
            (rng.standard_normal(att) * 0.1).astype(np.float32)]
        p.heads, p.att = h, att
        p.f = lambda t, y: O.transformer_rhs(p.ei, y, None, *p.proj, h, 1, ALPHA, 0.0, score_mode='per_edge')
    # labels: random, then the validation rows' from the oracle's predictions at a middle accepted step
    labels = rng.integers(0, CLASSES, R)
    Wd = p.W if Cd == width else np.concatenate([p.W, np.zeros((CLASSES, width - Cd), np.float32)], 1)
    p.Wd = Wd  # the decoder over the whole state width (zero columns past Cd): what the oracle scores with
    probe = EO.early_stop_adaptive(p.f, p.y0, p.t_end, 'dopri5', p.rtol, p.atol, Wd, p.b, p.masks, labels, 10 ** 6)
    p.mid = probe.n_accepted // 2
    labels[p.masks[1]] = probe.steps[p.mid].pred[p.masks[1]]
    p.labels = labels
    p.ref = EO.early_stop_adaptive(p.f, p.y0, p.t_end, 'dopri5', p.rtol, p.atol, Wd, p.b, p.masks, labels, 10 ** 6)
    p.data = types.SimpleNamespace(
        y=torch.from_numpy(labels.reshape(B, N_NODES)), train_mask=torch.from_numpy(p.masks[0].reshape(B, N_NODES)),
        val_mask=torch.from_numpy(p.masks[1].reshape(B, N_NODES)),
        test_mask=torch.from_numpy(p.masks[2].reshape(B, N_NODES)))
    _CACHE[key] = p
    return p


def check_problem(p):
    """What the problem was chosen for (asserted in the test, checked on the CPU when chosen)."""
    ref = p.ref
    assert ref.n_accepted >= 8 and ref.n_rejected >= 1, (ref.n_accepted, ref.n_rejected)
    vals = [s.counts[1] for s in ref.steps]
    best = int(np.argmax(vals))
    assert vals.count(max(vals)) == 1 and 0 < best < len(vals) - 1 and best == p.mid, vals
    masked = p.masks[0] | p.masks[1] | p.masks[2]
    for s in ref.steps:
        und = EO.undecided(s, p.Wd) & masked
        assert und.sum() <= 0.02 * masked.sum(), (s.t1, int(und.sum()))


def make_func(p, width=WIDTH):
    d = {"alpha_train": ALPHA, "beta_train": 0.0, "edge_index": p.ei, "weights": p.w.astype(np.float32),
         "x0": np.zeros((p.B, N_NODES, width), np.float32)}
    m = {"C": width, "block": "constant", "add_source": False, "no_alpha_sigmoid": False, "heads": 2}
    if p.kind == 'laplacian':
        return make_laplacian(d, m)
    d.update(Wq=p.proj[0], bq=p.proj[1], Wk=p.proj[2], bk=p.proj[3])
    m.update(heads=p.heads, attention_dim=p.att, attention_norm_idx=1, attention_type='scaled_dot')
    return make_transformer(d, m, score_mode='per_edge')


def make_integrator(p, method='dopri5', cap=100, record_pred=True, T_=None):
    opt = dict(OPT, method=method, earlystopxT=p.xT, max_test_steps=cap, tol_scale=p.tol_scale)
    es = EarlyStopInt(p.T if T_ is None else T_, opt, device=DEV)
    es.data = p.data
    es.m2_weight, es.m2_bias = T(p.W), T(p.b)
    es.record_pred = record_pred
    return es


def check_against_oracle(p, s, ref, masks=None):
    """Checks 1, 3 and 4 of the issue for a solver result ``s`` against the oracle's ``ref``."""
    masks = p.masks if masks is None else masks
    assert len(s.times) == ref.n_accepted and s.n_attempts == ref.n_attempts
    np.testing.assert_allclose(s.times, [st.t1 for st in ref.steps], rtol=1e-5)
    preds = s.preds.cpu().numpy()
    for k, st in enumerate(ref.steps):
        und = EO.undecided(st, p.Wd)
        scored = masks[0] | masks[1] | masks[2]
        decided = scored & ~und
        np.testing.assert_array_equal(preds[k][decided], st.pred[decided])
        assert (preds[k][~scored] == -1).all()
        for i, m in enumerate(masks):
            assert abs(s.counts[k][i] - st.counts[i]) <= int((und & m).sum()), (k, i)
    assert s.sizes == ref.sizes
    assert (s.best_val, s.best_test, s.best_train) == (ref.best_val, ref.best_test, ref.best_train)
    assert abs(s.best_time - ref.best_time) <= 1e-5 * max(1.0, abs(ref.best_time))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("kind", ["laplacian", "transformer"])
def test_early_stop_dopri5_vs_oracle(kind, B):
    p = build_problem(kind, B)
    check_problem(p)
    func = make_func(p)
    es = make_integrator(p)
    y0 = T(p.y0)
    got = es(func, y0, torch.tensor([0.0, 0.5], device=DEV), method='rk4', rtol=p.rtol, atol=p.atol)
    path = gi.odeint.last_path
    assert path in ('fused_krylov', 'fused_stage')
    assert got.shape == (2,) + p.y0.shape and not es.solver.capped
    check_against_oracle(p, es.solver, p.ref)
    assert 0 < es.solver.best_time < es.solver.times[-1] and es.solver.best_val == 1.0
    assert rel(got[1], p.ref.y) <= 1e-5
    # scoring does not move the trajectory: bit-equal to the plain solve of the same interval
    with torch.no_grad():
        plain = gnpde.odeint(func, y0, es.t, rtol=p.rtol, atol=p.atol, method='dopri5')
    assert gi.odeint.last_path == path and gi.odeint.last_n_steps == es.solver.n_attempts
    assert torch.equal(got, plain)
    # a second call starts its bests from 0 and repeats them (the record is zeroed per solve)
    first = (es.solver.best_val, es.solver.best_test, es.solver.best_train, es.solver.best_time, es.solver.counts)
    es(func, y0, None, rtol=p.rtol, atol=p.atol)
    assert (es.solver.best_val, es.solver.best_test, es.solver.best_train, es.solver.best_time,
            es.solver.counts) == first


@pytest.mark.parametrize("kind", ["laplacian", "transformer"])
def test_early_stop_cap(kind):
    """max_test_steps at half the oracle's attempts: the state at the last accepted t1, the
    bests of the scored prefix only."""
    p = build_problem(kind, 1)
    cap = p.ref.n_attempts // 2
    ref = EO.early_stop_adaptive(p.f, p.y0, p.t_end, 'dopri5', p.rtol, p.atol, p.Wd, p.b, p.masks, p.labels, cap)
    assert ref.capped and 1 <= ref.n_accepted < p.ref.n_accepted
    es = make_integrator(p, cap=cap)
    got = es(make_func(p), T(p.y0), None, rtol=p.rtol, atol=p.atol)
    assert es.solver.capped and es.solver.n_attempts == cap
    assert rel(got[1], ref.y) <= 1e-5
    assert torch.equal(got[0], T(p.y0))
    check_against_oracle(p, es.solver, ref)
    assert es.solver.best_time <= es.solver.times[-1]


def rk4_reference(p):
    t_end = float(np.float32(p.xT * RK4_T))
    h = t_end / 6.0
    return t_end, h, EO.early_stop_rk4(p.f, p.y0, t_end, h, p.Wd, p.b, p.masks, p.labels)


def test_early_stop_rk4_six_steps():
    p = build_problem('laplacian', 1)
    t_end, h, ref = rk4_reference(p)
    assert len(ref.steps) == 6
    func = make_func(p)
    es = make_integrator(p, method='rk4', T_=RK4_T)
    y0 = T(p.y0)
    for _ in range(2):  # (the second call replays the one-step graphs)
        got = es(func, y0, None, options={'step_size': h})
        s = es.solver
        assert len(s.times) == 6
        s.n_attempts = 6
        check_against_oracle(p, s, ref)
        assert rel(got[1], ref.y) <= 1e-5
    with torch.no_grad():
        plain = gnpde.odeint(func, y0, es.t, method='rk4', options={'step_size': h})
    assert torch.equal(got, plain)


def test_early_stop_under_the_node_layout(monkeypatch):
    """A solve in the graph's in-degree numbering (forced as tests/test_gpu_layout.py's
    graphs reach it: the size thresholds lowered) scores through ``rows``: the same counts,
    bests and bits as the solve in the caller's numbering."""
    p = build_problem('laplacian', 2)
    y0 = T(p.y0)
    out = {}
    for order in ("none", "degree"):
        monkeypatch.setattr(ops, "NODE_ORDER", order)
        monkeypatch.setattr(ops, "LAYOUT_MIN_ROWS", 1)
        monkeypatch.setattr(ops, "LAYOUT_MIN_BYTES", 1)
        func = make_func(p)
        assert (func.node_layout(y0) is not None) == (order == "degree")
        es = make_integrator(p)
        got = es(func, y0, None, rtol=p.rtol, atol=p.atol)
        s = es.solver
        out[order] = (got, s.counts, s.times, (s.best_val, s.best_test, s.best_train, s.best_time), s.preds)
        if order == "degree":
            lay = func._graph.node_layout
            # the predictions are per state row: internal row k is user row order[k]
            user = torch.empty_like(s.preds)
            user[:, lay.order] = s.preds
            out[order] = out[order][:4] + (user,)
    a, b = out["none"], out["degree"]
    assert a[1] == b[1] and a[3] == b[3]
    np.testing.assert_allclose(a[2], b[2], rtol=1e-9)  # (the error norm sums the rows in another order)
    assert torch.equal(a[4], b[4])
    assert rel(b[0][1], a[0][1].double().cpu().numpy()) <= 1e-6


def test_early_stop_augmented_state():
    """augment: the state is twice the decoder's width and its first half is scored."""
    p = build_problem('laplacian', 1, width=2 * WIDTH, Cd=WIDTH, seed=18)  # (chosen like PROBLEMS' seeds)
    check_problem(p)
    es = make_integrator(p)
    es(make_func(p, width=2 * WIDTH), T(p.y0), None, rtol=p.rtol, atol=p.atol)
    assert es.m2_weight.shape[1] == WIDTH
    check_against_oracle(p, es.solver, p.ref)


def test_block_forward_with_the_early_stop_integrator():
    """A ConstantODEblock in eval() with test_integrator = EarlyStopInt and data / m2_weight /
    m2_bias assigned as GNNEarly does: forward leaves solver.best_* populated, and later
    forwards replay the captured step graphs of the module's cache entry without capturing anything new."""
    p = build_problem('laplacian', 1)
    opt = dict(OPT, hidden_dim=WIDTH, method='dopri5', tol_scale=p.tol_scale, earlystopxT=p.xT, max_test_steps=100,
               max_nfe=10 ** 7)
    blk = gnpde.ConstantODEblock(gnpde.LaplacianODEFunc, [], opt, DEV, t=torch.tensor([0, p.T])).to(DEV).eval()
    with torch.no_grad():
        blk.odefunc.alpha_train.fill_(ALPHA)
    blk.test_integrator = EarlyStopInt(p.T, opt, DEV)
    blk.test_integrator.data = p.data
    blk.test_integrator.m2_weight, blk.test_integrator.m2_bias = T(p.W), T(p.b)
    data = gnpde.GraphData()
    data.new_graph(T(p.ei), N_NODES)
    x = T(p.y0)
    with torch.no_grad():
        z = blk(x, data)
        s = blk.test_integrator.solver
        assert s.best_val > 0 and s.best_time > 0 and len(s.times) >= 8
        entry = gi._ADAPTIVE_CACHE[blk.odefunc]
        z2 = blk(x, data)
        assert gi._ADAPTIVE_CACHE[blk.odefunc] is entry  # the cached state and its graphs, not a new entry
        # (a plain solve's second call captures the variant of the step after the initial-step probe, which
        # the first call ran eagerly while the module was cold; from then on nothing is captured)
        graphs = dict(entry[1].graphs)
        assert graphs and gi.adaptive_step_graph(blk.odefunc) is not None
        z3 = blk(x, data)
        assert gi._ADAPTIVE_CACHE[blk.odefunc] is entry and entry[1].graphs == graphs
        assert torch.equal(z3, z2)
    s2 = blk.test_integrator.solver
    assert s2 is not s and (s2.best_val, s2.best_test, s2.best_time, s2.counts) == (s.best_val, s.best_test,
                                                                                    s.best_time, s.counts)
    assert torch.equal(z, z2)


def test_bf16_state_raises():
    p = build_problem('laplacian', 1)
    es = make_integrator(p)
    with pytest.raises(NotImplementedError, match="bf16|bfloat16"):
        es(make_func(p), T(p.y0).to(torch.bfloat16), None, rtol=p.rtol, atol=p.atol)
