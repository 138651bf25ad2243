"""gnpde.early_stop_solver's control flow on CPU: the injected linear RHS of
tests/host_stage.py under the fused solvers and an injected torch scorer
(ops.decode_score_torch, the product restatement) or a scripted one — no GPU."""
import types

import numpy as np
import pytest
import torch

import early_stop_oracle as EO
import gnpde.integrator as gode
from gnpde import ops
from gnpde.early_stop_solver import EarlyStopInt
from host_stage import HostLinearRHS

C, K, N = 6, 4, 40


def _problem(seed=3, B=1):
    rng = np.random.default_rng(seed)
    A = (rng.standard_normal((C, C)) * 0.7).astype(np.float32)
    y0 = rng.standard_normal((B, N, C)).astype(np.float32)
    W = rng.standard_normal((K, C)).astype(np.float32)
    b = rng.standard_normal(K).astype(np.float32)
    R = B * N
    kind = rng.integers(0, 4, R)  # 0: in no split
    masks = [kind == 1, kind == 2, kind == 3]
    labels = rng.integers(0, K, R)
    data = types.SimpleNamespace(y=torch.from_numpy(labels.reshape(B, N)), train_mask=torch.from_numpy(masks[0].reshape(B, N)),
                                 val_mask=torch.from_numpy(masks[1].reshape(B, N)),
                                 test_mask=torch.from_numpy(masks[2].reshape(B, N)))
    return A, y0, W, b, masks, labels, data


def _integrator(T, opt, data, W, b, scorer=ops.decode_score_torch):
    es = EarlyStopInt(T, opt, device='cpu', scorer=scorer)
    es.data = data
    es.m2_weight, es.m2_bias = torch.from_numpy(W), torch.from_numpy(b)
    return es


def _opt(method='dopri5', xT=2.0, cap=100):
    return {'method': method, 'earlystopxT': xT, 'max_test_steps': cap}


def _scripted(script):
    """A scorer that adds the k-th scripted count triple at its k-th call."""
    calls = []

    def scorer(y, W, b, split, label, counts_out, ld=None, rows=None, pred_out=None):
        counts_out += torch.tensor(script[len(calls)], dtype=counts_out.dtype)
        calls.append(y.clone())
    return scorer, calls


def test_interval_override_shape_and_plain_solve_equality():
    """The passed t and method are ignored for [0, earlystopxT T] and opt['method']; a solve
    that does not reach its cap returns bit for bit what gnpde.odeint returns over that
    interval on the same RHS."""
    A, y0, W, b, masks, labels, data = _problem()
    es = _integrator(0.75, _opt(xT=2.0), data, W, b)
    assert es.t.tolist() == [0.0, 1.5] and es.t.dtype == torch.float32
    f = HostLinearRHS(torch.from_numpy(A))
    got = es(f, torch.from_numpy(y0), torch.tensor([0.0, 0.1]), method='euler', rtol=1e-5, atol=1e-7)
    assert got.shape == (2,) + y0.shape
    assert not es.solver.capped and es.solver.n_attempts == gode.odeint.last_n_steps
    with torch.no_grad():
        want = gode.odeint(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), es.t, rtol=1e-5, atol=1e-7,
                           method='dopri5', combine=gode._Combine())
    assert gode.odeint.last_n_steps == es.solver.n_attempts
    assert torch.equal(got, want)
    assert len(es.solver.times) >= 2 and es.solver.times[-1] >= 1.5
    # every accepted step was scored, with the counts of the float64 restatement
    ref = EO.early_stop_adaptive(lambda t, y: y @ A.astype(np.float64).T, y0, 1.5, 'dopri5', 1e-5, 1e-7, W, b, masks,
                                 labels, 100)
    assert len(es.solver.times) == ref.n_accepted and es.solver.n_attempts == ref.n_attempts
    np.testing.assert_allclose(es.solver.times, [s.t1 for s in ref.steps], rtol=1e-4)
    for k, s in enumerate(ref.steps):
        und = EO.undecided(s, W)
        for i, m in enumerate(masks):
            assert abs(es.solver.counts[k][i] - s.counts[i]) <= int((und & m).sum())


def test_method_assert():
    A, y0, W, b, masks, labels, data = _problem()
    es = _integrator(1.0, _opt(method='euler'), data, W, b)
    with pytest.raises(AssertionError, match="dopri5 and rk4"):
        es(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), None)


def test_rk4_scores_every_grid_step_strict_improvement_and_reset():
    """rk4: one score per grid step, on the state that step produced; best_* follow the
    strict val > best_val rule (the earliest of equal steps wins) and restart at 0 in
    every call."""
    A, y0, W, b, masks, labels, data = _problem()
    sizes = [int(m.sum()) for m in masks]
    script = [(1, 1, 5), (2, 3, 4), (5, 3, 9), (0, 2, 1)]
    scorer, calls = _scripted(script)
    es = _integrator(0.5, _opt(method='rk4', xT=2.0), data, W, b, scorer=scorer)
    f = HostLinearRHS(torch.from_numpy(A))
    got = es(f, torch.from_numpy(y0), None, options={'step_size': 0.25})
    s = es.solver
    assert s.times == [0.25, 0.5, 0.75, 1.0] and s.counts == [list(c) for c in script]
    assert (s.best_val, s.best_train, s.best_test, s.best_time) == (3 / sizes[1], 2 / sizes[0], 4 / sizes[2], 0.5)
    with torch.no_grad():
        want = gode.odeint(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), es.t, method='rk4',
                           options={'step_size': 0.25}, combine=gode._Combine())
    assert torch.equal(got, want)
    assert torch.equal(calls[-1], want[1])  # the scored states are the steps' results
    assert f.nfe == 16
    # a second call starts from 0 again: lower scores give lower bests
    script2 = [(1, 0, 1), (1, 1, 1), (1, 1, 2), (1, 1, 3)]
    es.scorer, _ = _scripted(script2)
    es(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), None, options={'step_size': 0.25})
    s = es.solver
    assert (s.best_val, s.best_test, s.best_time) == (1 / sizes[1], 1 / sizes[2], 0.5)
    # no step improves on 0: the bests stay 0
    es.scorer, _ = _scripted([(1, 0, 1)] * 4)
    es(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), None, options={'step_size': 0.25})
    assert (es.solver.best_val, es.solver.best_test, es.solver.best_train, es.solver.best_time) == (0, 0, 0, 0)


def test_cap_returns_the_last_accepted_state():
    """max_test_steps counts attempts; reached before the end time, the solve returns the
    state at the last accepted t1 and the bests of the scored prefix."""
    A, y0, W, b, masks, labels, data = _problem()
    A64 = A.astype(np.float64)
    full = EO.early_stop_adaptive(lambda t, y: y @ A64.T, y0, 3.0, 'dopri5', 1e-5, 1e-7, W, b, masks, labels, 1000)
    cap = full.n_attempts // 2
    assert cap >= 2
    ref = EO.early_stop_adaptive(lambda t, y: y @ A64.T, y0, 3.0, 'dopri5', 1e-5, 1e-7, W, b, masks, labels, cap)
    assert ref.capped and 1 <= ref.n_accepted < full.n_accepted
    es = _integrator(1.5, _opt(xT=2.0, cap=cap), data, W, b)
    got = es(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0), None, rtol=1e-5, atol=1e-7)
    s = es.solver
    assert s.capped and s.n_attempts == cap and len(s.times) == ref.n_accepted
    assert torch.equal(got[0], torch.from_numpy(y0))
    err = np.abs(got[1].double().numpy() - ref.y).max() / np.abs(ref.y).max()
    assert err <= 1e-5, err
    np.testing.assert_allclose(s.times, [st.t1 for st in ref.steps], rtol=1e-4)
    assert s.best_time <= s.times[-1]


@pytest.mark.parametrize("fused", [True, False])
def test_cap_before_any_accepted_step_returns_y0(fused):
    """A first attempt that is rejected under a cap of one attempt: the result is y0, nothing
    was scored (the fused loop and the restated tableau loop)."""
    A, y0, W, b, masks, labels, data = _problem()
    scorer, calls = _scripted([])
    es = _integrator(1.5, _opt(xT=2.0, cap=1), data, W, b, scorer=scorer)
    if fused:
        f = HostLinearRHS(torch.from_numpy(A))
    else:
        At = torch.from_numpy(A)
        f = lambda t, y: y @ At.T  # noqa: E731
        gode_combine = gode._torch_combine
    y0t = torch.from_numpy(y0)
    if fused:
        got = es(f, y0t, None, rtol=1e-6, atol=1e-8, options={'first_step': 40.0})
    else:
        # the restated loop takes the host combine (as the other host-logic tests inject it)
        hook_opts = {'first_step': 40.0, 'gnpde_max_attempts': 1, 'gnpde_accept_hook': lambda y, t1, lay: calls.append(y)}
        got = gode.odeint(f, y0t, es.t, rtol=1e-6, atol=1e-8, method='dopri5', options=hook_opts, combine=gode_combine)
        assert gode.odeint.last_path == 'restated' and gode.odeint.last_capped
    assert not calls
    assert torch.equal(got[1], y0t) and torch.equal(got[0], y0t)
    if fused:
        assert es.solver.capped and es.solver.n_attempts == 1 and es.solver.times == []
        assert (es.solver.best_val, es.solver.best_time) == (0, 0)


def test_restated_loop_hook_and_cap_match_the_fused_loop():
    """The tableau loop (_RKAdaptive) with the hook and the cap: the same accepted times and
    attempt count as the fused loop, the hook on every accepted state."""
    A, y0, W, b, masks, labels, data = _problem()
    At, y0t = torch.from_numpy(A).double(), torch.from_numpy(y0).double()  # (float64: the two loops' error norms agree)
    ts = torch.tensor([0.0, 3.0], dtype=torch.float64)
    runs = []
    for f, comb in ((HostLinearRHS(At), gode._Combine()), (lambda t, y: y @ At.T, gode._torch_combine)):
        seen = []
        with torch.no_grad():
            out = gode.odeint(f, y0t, ts, rtol=1e-5, atol=1e-7, method='dopri5', combine=comb,
                              options={'gnpde_max_attempts': 5, 'gnpde_accept_hook': lambda y, t1, lay: seen.append(
                                  (t1, y.clone()))})
        runs.append((out, seen, gode.odeint.last_n_steps, gode.odeint.last_capped, gode.odeint.last_path))
    (a, sa, na, ca, pa), (b_, sb, nb, cb, pb) = runs
    assert pa != 'restated' and pb == 'restated'
    assert na == nb == 5 and ca and cb and len(sa) == len(sb) >= 1
    np.testing.assert_allclose([t for t, _ in sa], [t for t, _ in sb], rtol=1e-9)
    assert torch.equal(a[1], sa[-1][1]) and torch.equal(b_[1], sb[-1][1])
    # float64 both: the loops differ by the reassociation of the Krylov restatement only
    assert float((a[1] - b_[1]).abs().max()) <= 1e-9 * float(b_[1].abs().max())


def test_plain_solves_are_untouched_by_the_hook_plumbing():
    """Without hook and cap the adaptive solve makes the same RHS calls as before."""
    A, y0, W, b, masks, labels, data = _problem()
    f = HostLinearRHS(torch.from_numpy(A))
    with torch.no_grad():
        gode.odeint(f, torch.from_numpy(y0), torch.tensor([0.0, 1.5]), rtol=1e-5, atol=1e-7, method='dopri5',
                    combine=gode._Combine())
    assert not gode.odeint.last_capped
    assert f.nfe == 2 + gode._adaptive_plan('dopri5').ns * gode.odeint.last_n_steps


def test_bf16_state_is_refused():
    A, y0, W, b, masks, labels, data = _problem()
    es = _integrator(1.0, _opt(), data, W, b)
    with pytest.raises(NotImplementedError, match="bf16|bfloat16"):
        es(HostLinearRHS(torch.from_numpy(A)), torch.from_numpy(y0).to(torch.bfloat16), None)


@pytest.mark.parametrize("B", [1, 2])
def test_pack_splits(B):
    rng = np.random.default_rng(5)
    n = 37
    R = B * n
    tr, va, te = (rng.random(R) < 0.4 for _ in range(3))  # overlapping on purpose
    assert (tr & va).any() and (tr & va & te).any()
    y = rng.integers(0, 7, R)
    shape = (n,) if B == 1 else (B, n)
    data = types.SimpleNamespace(y=torch.from_numpy(y.reshape(shape)), train_mask=torch.from_numpy(tr.reshape(shape)),
                                 val_mask=torch.from_numpy(va.reshape(shape)),
                                 test_mask=torch.from_numpy(te.reshape(shape)))
    split, label, sizes = ops.pack_splits(data, R, 'cpu')
    assert split.dtype == torch.uint8 and label.dtype == torch.int32 and split.shape == label.shape == (R,)
    np.testing.assert_array_equal(split.numpy(), tr * 1 + va * 2 + te * 4)
    np.testing.assert_array_equal(label.numpy(), y)
    assert sizes == (int(tr.sum()), int(va.sum()), int(te.sum())) and all(isinstance(v, int) for v in sizes)
    assert ops.pack_splits(data, R, 'cpu')[0] is split  # cached by tensor identity
    data.val_mask = data.val_mask.clone()
    assert ops.pack_splits(data, R, 'cpu')[0] is not split
    if B == 1:  # a per-node set under a batched state repeats over the batch elements
        s2, l2, z2 = ops.pack_splits(data, 2 * R, 'cpu')
        np.testing.assert_array_equal(s2.numpy(), np.tile(split.numpy(), 2))
        np.testing.assert_array_equal(l2.numpy(), np.tile(y, 2))
        assert z2 == tuple(2 * v for v in sizes)
        with pytest.raises(ValueError):
            ops.pack_splits(data, R + 1, 'cpu')


@pytest.mark.parametrize("ld,Cd,Kc", [(4, 4, 2), (8, 4, 7), (10, 10, 3)])
def test_torch_scorer_matches_numpy_on_exact_data(ld, Cd, Kc):
    """The torch restatement (the fallback of the kernel and these tests' scorer) on
    integer-valued data, where every logit is exact and ties are frequent: predictions and
    counts equal numpy's, through ``rows``, on the first Cd columns, added to the counts."""
    rng = np.random.default_rng(ld * 31 + Kc)
    R = 65
    y = rng.integers(-3, 4, (R, ld)).astype(np.float32)
    W = rng.integers(-2, 3, (Kc, Cd)).astype(np.float32)
    b = rng.integers(-1, 2, Kc).astype(np.float32)
    split = rng.choice([0, 1, 2, 4, 3, 7], R).astype(np.uint8)
    label = rng.integers(0, Kc, R).astype(np.int32)
    rows = rng.permutation(R).astype(np.int32)
    logits = np.maximum(y[:, :Cd], 0).astype(np.float64) @ W.T.astype(np.float64) + b
    pred = logits.argmax(1)
    for use_rows in (False, True):
        sp, lb = (split[rows], label[rows]) if use_rows else (split, label)
        want = [int(((pred == lb) & ((sp >> k) & 1 == 1)).sum()) for k in range(3)]
        counts = torch.tensor([5, 0, 2], dtype=torch.int32)
        pred_out = torch.empty(R, dtype=torch.int32)
        ops.decode_score_torch(torch.from_numpy(y), torch.from_numpy(W), torch.from_numpy(b), torch.from_numpy(split),
                               torch.from_numpy(label), counts, ld=ld, rows=torch.from_numpy(rows) if use_rows else None,
                               pred_out=pred_out)
        assert counts.tolist() == [want[0] + 5, want[1], want[2] + 2]
        np.testing.assert_array_equal(pred_out.numpy(), np.where(sp != 0, pred, -1))


def test_decode_score_argument_errors_without_a_device():
    """gnpde_decode_score_f32 validates on the host: -1 / -3 before any launch (the GPU
    suite's check, which needs no device)."""
    from test_gpu_early_stop import check_abi_errors
    check_abi_errors()


def test_gpu_suite_problems_meet_their_conditions():
    """The solve problems of tests/test_gpu_early_stop.py, checked here on the CPU with the
    oracle alone: enough accepted and rejected steps, a unique interior validation maximum,
    at most 2 % undecided rows per step."""
    import test_gpu_early_stop as G
    for key in G.PROBLEMS:
        G.check_problem(G.build_problem(*key))
    G.check_problem(G.build_problem('laplacian', 1, width=2 * G.WIDTH, Cd=G.WIDTH, seed=18))
