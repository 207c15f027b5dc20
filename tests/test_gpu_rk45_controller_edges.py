"""The boundary branches of the device RK45 step controller (csrc/rk45.hip: rk45_decide_kernel, begin_attempt, rk45_record_kernel) and
of its host loop (samplers.py: ODESampler._solve / run) against scipy.integrate.RK45 on the float64 field: the edge problems of
tests/rk45_edge_cases.py, each shown by tests/test_rk45_edge_cases_cpu.py to take its branch in the reference.  Strict problems are held
to scipy's schedule attempt for attempt, path-sensitive ones to the float64 replay of the device's own attempts (rr.replay_check);
the terminal paths (log and trajectory capacity, attempt budget, too-small step, a non-finite state) to what scipy does or refuses."""
import math

import numpy as np
import pytest
import torch

import rk45_edge_cases as ec
import rk45_reference as rr
from oracle import genpose_oracle as go

pytestmark = pytest.mark.gpu

_SNET, _REF = {}, {}
CANARY = -7.25


def _snet(problem):
    if problem not in _SNET:
        from genpose_amd.scorenet import ScoreNetHIP
        _SNET[problem] = ScoreNetHIP(ec.nets()[problem].state_dict(go.make_state_dict(0, "score")), "cuda")
    return _SNET[problem]


def _ref(name, B, K):
    """problem, scipy solve on the float64 field, exact end state and scipy's own global error: computed once, never modified"""
    key = (name, B, K)
    if key not in _REF:
        p = ec.setup(name, B, K)
        e, net = p["edge"], p["net"]
        sc = ec.scipy_reference(p)
        x64 = p["Y0"][:, :9]
        exact = rr.exact_solution(net, "score", x64, p["c_rows"], e.T0, [e.t_bound])[0]
        if e.model == "likelihood":
            pr = p["probe"].astype(np.float64)
            dlogp = np.einsum("ri,ij,rj->r", pr, net.A, pr) * rr.phi(rr.a_score, e.T0, e.t_bound)
            exact = np.concatenate([exact, dlogp[:, None]], 1)
        scipy_err = np.abs(sc["states"][-1].reshape(p["Y0"].shape) - exact).max()
        _REF[key] = (p, sc, exact, scipy_err)
    return _REF[key]


def _sampler(e, B, K, **kw):
    from genpose_amd.samplers import ODESampler
    return ODESampler(_snet(e.problem), B, K, "cuda", model=e.model, tile=ec.PLAN_OF_SHAPE[(B, K)], **kw)


def _cvec(p):
    return _snet(p["edge"].problem).cloud_embed(torch.from_numpy(p["pf"]).cuda())


def _solve(smp, p, cvec=None):
    e = p["edge"]
    probe = torch.from_numpy(p["probe"]).cuda() if e.model == "likelihood" else None
    runs = rr.solve_raw(smp, _cvec(p) if cvec is None else cvec, torch.from_numpy(p["Y0"]).cuda(), e.T0, e.t_bound, e.rtol, e.atol, probe=probe,
                        max_attempts=e.max_attempts)
    return runs[0]


def _end_state_ratio(run, exact, scipy_err):
    """the tolerance rule of test_gpu_rk45_exact.py::test_score_solve_replay_and_ground_truth: 4 x scipy's own global error + the float32
    floor; returns |end - exact| / tolerance"""
    tol = 4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max())
    return float(np.abs(run["states"][-1] - exact).max() / tol)


def _device_log(run):
    return dict(err=run["log_err"], acc=run["log_acc"].astype(bool), h=run["log_h"])


def _same_schedule(run, sc):
    assert int(run["nfev"]) == sc["nfev"], (int(run["nfev"]), sc["nfev"])
    assert int(run["n_attempts"]) == len(sc["acc"]) and int(run["n_accepted"]) == int(sc["acc"].sum())
    np.testing.assert_array_equal(run["log_acc"].astype(bool), sc["acc"])


def _steps_fixed_by_the_controller(run, sc, p):
    """log_t / log_h against scipy's OWN t / h (rr.replay_check holds them to the controller applied to the device's error norms) on
    every attempt whose step does not depend on the value of an error norm: a first attempt at 100 h0 with h0 = 1e-6 or over the whole
    interval, an attempt after a factor capped at MAX_FACTOR (in scipy's log and in the device's), an attempt clipped to t_bound - each
    following a start time fixed in the same way.  Same tolerances as rr.replay_check: 2 u |t| on the start, 4 u (|h| + |t|) on the step.
    Returns (attempts compared, worst ratio)."""
    e = p["edge"]
    h0, h_abs, *_ = ec.initial_step_of(p)
    interval = abs(e.t_bound - e.T0)
    lt, lh, le = run["log_t"], run["log_h"], run["log_err"]
    capped = lambda err: err == 0 or ec.raw_factor(err) > rr.MAX_FACTOR
    fixed = h_abs == interval or (h0 == min(1e-6, interval) and h_abs == 100 * h0)
    n, worst = 0, 0.0
    for i in range(len(sc["acc"])):
        if not fixed:
            break
        t, h = sc["t"][i], sc["h"][i]
        assert abs(lt[i] - t) <= 2 * rr.U64 * abs(t), f"attempt {i} starts at {lt[i]!r}, scipy's at {t!r}"
        dh = abs(lh[i] - h) / (4 * rr.U64 * abs(h) + 4 * rr.U64 * abs(t))
        assert dh <= 1.0, f"attempt {i}: h {lh[i]!r} vs scipy's {h!r}"
        n, worst = n + 1, max(worst, dh)
        clipped_next = i + 1 < len(sc["acc"]) and sc["h"][i + 1] == e.t_bound - sc["t"][i + 1]
        fixed = bool(sc["acc"][i]) and ((capped(sc["err"][i]) and capped(float(le[i]))) or clipped_next)
    return n, worst


def _record(tag, run, sc, **ratios):
    bc, dc = ec.branch_counts(sc, 0, 1), ec.branch_counts(_device_log(run), 0, 1)
    keys = ("attempts", "accepted", "err_zero", "cap", "clamp", "floor")
    print(f"EDGE {tag}: f64 " + " ".join(f"{k}={bc[k]}" for k in keys) + f" nfev={sc['nfev']} | device nfev={int(run['nfev'])} n_attempts={int(run['n_attempts'])} "
          + " ".join(f"{k}={dc[k]}" for k in keys[1:]) + " | worst/bound " + " ".join(f"{k}={v:.3g}" for k, v in ratios.items()))


STRICT_CASES = [c for c in ec.CASES if ec.BY_NAME[c[0]].strict]
PATH_CASES = [c for c in ec.CASES if not ec.BY_NAME[c[0]].strict and "log_cap" not in ec.BY_NAME[c[0]].branches and c[0] != "dense_one_point"]


# ----------------------------------------------------------------------------- strict entries: scipy's schedule, attempt for attempt
@pytest.mark.parametrize("name,B,K", STRICT_CASES)
def test_strict_edges_take_scipys_schedule(name, B, K):
    p, sc, exact, scipy_err = _ref(name, B, K)
    e = p["edge"]
    smp = _sampler(e, B, K)
    run = _solve(smp, p)
    assert int(run["status"]) == 1
    _same_schedule(run, sc)
    assert float(run["t"]) == e.t_bound, "the solve ends at t_bound bit for bit"
    ratios = {}
    if e.exact:
        # the zero field: every stage derivative is 0, every error norm 0, every step a power-of-ten multiple formed in float64 exactly as
        # rk.py forms it - nothing carries a rounding of the device's own
        assert np.array_equal(run["log_t"], sc["t"]) and np.array_equal(run["log_h"], sc["h"]), (run["log_t"], sc["t"], run["log_h"], sc["h"])
        assert np.all(run["log_err"] == 0.0)
        assert all(np.array_equal(s, p["Y0"]) for s in run["states"]), "the state never moves"
    else:
        ratios.update(rr.replay_check(p["field"], run, e.T0, e.t_bound, e.rtol, e.atol))
        n, worst = _steps_fixed_by_the_controller(run, sc, p)
        assert n >= 1
        ratios["scipy_steps"] = worst
        dev, ref = ec.branch_counts(_device_log(run), e.T0, e.t_bound), ec.branch_counts(sc, e.T0, e.t_bound)
        # (an error norm of 1e-30 in float64 may be an exact 0 on the device: both take the MAX_FACTOR branch)
        assert dev["cap"] + dev["err_zero"] == ref["cap"] + ref["err_zero"] and dev["clamp"] == ref["clamp"] and dev["interval"] == ref["interval"]
    ratios["end_state"] = _end_state_ratio(run, exact, scipy_err)
    assert ratios["end_state"] <= 1.0
    _record(f"{name} {B}x{K}", run, sc, **ratios)


@pytest.mark.parametrize("name", ["zero_state_small_offset", "min_step"])
def test_ragged_launch_with_a_padding_group(name):
    """capacity two groups, one in use: the controller of the padding group (grows <= 0) ends it at once, the live group's solve is the
    2 x 3 solve of the equal-groups launch"""
    from genpose_amd.samplers import ODESampler
    B, K = 2, 3
    p, sc, exact, scipy_err = _ref(name, B, K)
    e = p["edge"]
    smp = ODESampler(_snet(e.problem), 3, K, "cuda", group_clouds=[2, 1], tile=16)
    smp.set_groups([2])
    run = _solve(smp, p)
    _same_schedule(run, sc)
    assert float(run["t"]) == e.t_bound
    ratios = rr.replay_check(p["field"], run, e.T0, e.t_bound, e.rtol, e.atol)
    ratios["end_state"] = _end_state_ratio(run, exact, scipy_err)
    assert ratios["end_state"] <= 1.0
    pad = smp._read_states()[1]
    assert int(pad["status"]) == 1 and int(pad["n_attempts"]) == 0 and int(pad["n_accepted"]) == 0
    _record(f"{name} ragged [2]+padding", run, sc, **ratios)


# ----------------------------------------------------------------------------- path-sensitive entries: the float64 replay
@pytest.mark.parametrize("name,B,K", PATH_CASES)
def test_path_sensitive_edges_replay(name, B, K):
    p, sc, exact, scipy_err = _ref(name, B, K)
    e = p["edge"]
    smp = _sampler(e, B, K)
    smp.TRAJ_CAP = 3 * smp.TRAJ_CAP  # (this instance: room for every accepted state of the overflow problem; solve_raw sizes its buffer by it)
    run = _solve(smp, p)
    assert int(run["status"]) == 1 and float(run["t"]) == e.t_bound
    ratios = rr.replay_check(p["field"], run, e.T0, e.t_bound, e.rtol, e.atol)
    ratios["end_state"] = _end_state_ratio(run, exact, scipy_err)
    assert ratios["end_state"] <= 1.0
    _record(f"{name} {B}x{K}", run, sc, **ratios)


# ----------------------------------------------------------------------------- the 512-entry log
@pytest.mark.parametrize("name", ["log_overflow", "log_overflow_f32"])
def test_log_stops_at_512_attempts_and_the_solve_goes_on(name):
    """log_overflow is the issue's problem at rtol = atol = 1e-9, below the float32 network's resolution (tests/rk45_edge_cases.py): the
    device needs several times scipy's 568 attempts there and runs under a larger budget; log_overflow_f32 overflows the log at 1e-5."""
    import dataclasses
    B, K = ec.BY_NAME[name].shapes[0]
    p, sc, exact, scipy_err = _ref(name, B, K)
    e = p["edge"]
    smp = _sampler(e, B, K)
    smp.TRAJ_CAP = e.max_attempts + 64  # (this instance: room for every accepted state within the budget)
    run = _solve(smp, p)
    n = int(run["n_attempts"])
    assert int(run["status"]) == 1 and float(run["t"]) == e.t_bound
    assert n > ec.LOG_CAP and int(run["nfev"]) == 2 + 6 * n
    assert all(len(run[k]) == ec.LOG_CAP for k in ("log_t", "log_h", "log_err", "log_acc"))
    ratios = rr.replay_check(p["field"], run, e.T0, e.t_bound, e.rtol, e.atol)  # the first 512 attempts, from the device's own states
    ratios["end_state"] = _end_state_ratio(run, exact, scipy_err)
    assert ratios["end_state"] <= 1.0
    _record(f"{name} {B}x{K}", run, sc, **ratios)
    # a second solve on the same sampler (same network, a short solve at 1e-5) logs from entry 0 again
    e2 = dataclasses.replace(e, T0=0.15, rtol=1e-5, atol=1e-5, max_attempts=4096)
    p2 = ec.setup(e2, B, K)
    run2 = _solve(smp, p2)
    assert int(run2["status"]) == 1 and int(run2["n_attempts"]) == len(run2["log_t"]) < ec.LOG_CAP
    assert run2["log_t"][0] == e2.T0 and float(run2["t"]) == e2.t_bound
    rr.replay_check(p2["field"], run2, e2.T0, e2.t_bound, e2.rtol, e2.atol)


# ----------------------------------------------------------------------------- trajectory capacity
def _canary_traj(rows, width):
    return torch.full((rows, width), CANARY, dtype=torch.float64, device="cuda")


@pytest.mark.parametrize("B,K", ec.SHAPES)
def test_trajectory_capacity_is_exact(B, K):
    """N accepted states (scipy's count: a strict problem) need N + 1 slots.  The trajectory is the head of a larger buffer whose tail is
    a canary: a record past the capacity would land there.  On this field (A = 0: a step's error does not feed back into later steps) the
    device takes scipy's steps exactly (every factor capped or clipped), so accepted state k is scipy's to within the sum of the first
    k steps' bounds rr.step_bound - the per-step rule of rr.replay_check, accumulated."""
    name = "zero_state_small_offset"
    p, sc, exact, scipy_err = _ref(name, B, K)
    e = p["edge"]
    N = int(sc["acc"].sum())
    R = B * K
    smp = _sampler(e, B, K)
    smp.TRAJ_CAP = N + 1
    big = _canary_traj(N + 1 + 4, R * 9)
    smp._raw_traj = big[: N + 1]
    run = _solve(smp, p)
    _same_schedule(run, sc)
    assert run["states"].shape[0] == N + 1
    ratios = rr.replay_check(p["field"], run, e.T0, e.t_bound, e.rtol, e.atol)
    assert np.array_equal(run["states"][0], p["Y0"])
    fun = rr.fun_flat(p["field"], R)
    acc_bound, worst = np.zeros(R * 9), 0.0
    for k in range(N):  # (every attempt of this solve is accepted: attempt k produces state k + 1)
        t, h, y = sc["t"][k], sc["h"][k], sc["states"][k]
        _, _, _, _, stage_y = rr.dp_attempt(fun, t, y, fun(t, y), h, e.rtol, e.atol)
        acc_bound = acc_bound + rr.step_bound(p["field"], t, h, stage_y)
        r = np.max(np.abs(run["states"][k + 1].reshape(-1) - sc["states"][k + 1]) / acc_bound)
        worst = max(worst, r)
        assert r <= 1.0, f"accepted state {k + 1} off scipy's by {r:.2f} x the accumulated step bounds"
    ratios["scipy_states"] = worst
    assert bool((big[N + 1:] == CANARY).all()), "a record went past the trajectory's capacity"
    _record(f"{name} {B}x{K} TRAJ_CAP=N+1", run, sc, **ratios)
    # one slot fewer: the host refuses, the device has not written past the capacity, the slots it has hold the same states
    cvec = _cvec(p)
    small = _sampler(e, B, K)
    small.TRAJ_CAP = N
    bigN = _canary_traj(N + 4, R * 9)
    small.traj = bigN[:N]
    with pytest.raises(RuntimeError, match="trajectory capacity"):
        small.run(cvec, torch.zeros(B, 3, device="cuda"), torch.from_numpy(p["x"]).cuda(), e.T0, return_process=True)
    assert bool((bigN[N:] == CANARY).all()), "a record went past the trajectory's capacity"
    assert torch.equal(bigN[:N], big[:N])


def test_trajectory_overflow_at_the_default_capacity():
    from genpose_amd.samplers import ODESampler
    name, (B, K) = "traj_overflow", ec.BY_NAME["traj_overflow"].shapes[0]
    p, sc, _, _ = _ref(name, B, K)
    e = p["edge"]
    smp = _sampler(e, B, K)
    assert smp.TRAJ_CAP == ODESampler.TRAJ_CAP
    budget = 1024
    big = _canary_traj(smp.TRAJ_CAP + budget + 64, B * K * 9)  # every accepted state of a solve within the attempt budget lands inside
    smp.traj = big[: smp.TRAJ_CAP]
    with pytest.raises(RuntimeError, match="trajectory capacity"):
        smp.run(_cvec(p), torch.zeros(B, 3, device="cuda"), torch.from_numpy(p["x"]).cuda(), e.T0, return_process=True, max_attempts=budget)
    st = smp._read_states()[0]
    assert int(st["status"]) == 1 and int(st["n_accepted"]) + 1 > smp.TRAJ_CAP
    assert bool((big[smp.TRAJ_CAP:] == CANARY).all()), "a record went past the trajectory's capacity"
    assert bool((big[: smp.TRAJ_CAP] != CANARY).any(dim=1).all()), "every slot within the capacity was recorded"
    print(f"EDGE {name} {B}x{K} default capacity: f64 accepted={int(sc['acc'].sum())} | device nfev={int(st['nfev'])} n_attempts={int(st['n_attempts'])} "
          f"accepted={int(st['n_accepted'])} -> capacity error, canary intact")


# ----------------------------------------------------------------------------- dense output with one point
@pytest.mark.parametrize("B,K", ec.SHAPES)
def test_dense_output_with_one_point(B, K):
    """t_eval = [T0]: scipy's dense output there is y0 itself (test_rk45_edge_cases_cpu.py), so the one emitted state is the finished
    (normalised, centred) y0 - the rule of test_gpu_rk45_exact.py::test_dense_output_exact for the first row"""
    p, sc, _, _ = _ref("dense_one_point", B, K)
    e = p["edge"]
    smp = _sampler(e, B, K)
    centre = torch.randn(B, 3, generator=torch.Generator().manual_seed(1)).cuda()
    xs, x = smp.run(_cvec(p), centre, torch.from_numpy(p["x"]).cuda(), e.T0, num_steps=e.num_steps, return_process=True)
    assert xs.shape == (B * K, 1, 9) and bool(torch.isfinite(x).all())
    y0p = torch.from_numpy(p["Y0"].copy())
    y0p[:, :6] = go.normalize_rotation(y0p[:, :6])
    y0p[:, 6:] += centre.cpu().double().repeat_interleave(K, 0)
    got = xs[:, 0].cpu().numpy()
    ratio = np.max(np.abs(got - y0p.numpy()) / (4 * rr.U64 + 4 * rr.U64 * np.abs(y0p.numpy())))
    np.testing.assert_allclose(got, y0p.numpy(), rtol=4 * rr.U64, atol=4 * rr.U64)
    st = smp.last_stats
    print(f"EDGE dense_one_point {B}x{K}: f64 attempts={len(sc['acc'])} | device nfev={int(st['nfev'])} n_attempts={int(st['n_attempts'])} | worst/bound emitted={ratio:.3g}")


# ----------------------------------------------------------------------------- failures: budget, non-finite state, and the sampler afterwards
_CONTRACT = ("interval_1e-4", 1.0)  # the 'contract' network (the entry's), solved from T0 = 1 like rk45_reference.problems()'s users do


def _contract(B, K):
    """contract / T0 = 1 at this shape: inputs, scipy's attempt count, and a FRESH sampler's results (computed once)"""
    key = ("contract_T1", B, K)
    if key not in _REF:
        e = ec.BY_NAME[_CONTRACT[0]]
        net, T0 = ec.nets()[e.problem], _CONTRACT[1]
        pf, x, _ = rr.inputs(B, K, T0)
        fld = rr.Field(net, "score", np.repeat(net.offsets(pf), K, 0))
        sc = rr.scipy_run(rr.fun_flat(fld, B * K), T0, x.astype(np.float64).reshape(-1), rr.EPS)
        cvec = _snet(e.problem).cloud_embed(torch.from_numpy(pf).cuda())
        centre = torch.randn(B, 3, generator=torch.Generator().manual_seed(1)).cuda()
        fresh = _sampler(e, B, K)
        _, xf = fresh.run(cvec, centre, torch.from_numpy(x).cuda(), T0)
        st = fresh.last_stats
        _REF[key] = dict(e=e, T0=T0, x=x, cvec=cvec, centre=centre, sc=sc, x_fresh=xf.clone(), nfev=int(st["nfev"]), log_acc=st["log_acc"].copy())
    return _REF[key]


def _reused_like_fresh(smp, c):
    """after a failed solve the same sampler solves contract / T0 = 1 exactly as a freshly constructed one does"""
    _, x = smp.run(c["cvec"], c["centre"], torch.from_numpy(c["x"]).cuda(), c["T0"])
    assert torch.equal(x, c["x_fresh"])
    assert int(smp.last_stats["nfev"]) == c["nfev"] and np.array_equal(smp.last_stats["log_acc"], c["log_acc"])


def test_attempt_budget_and_reuse():
    B, K = 2, 3
    c = _contract(B, K)
    needed = len(c["sc"]["acc"])
    smp = _sampler(c["e"], B, K)
    budget = needed // 2
    assert budget + smp.poll + 1 < needed, "the solve cannot finish within the budget and the chunk that overshoots it"
    with pytest.raises(RuntimeError, match="attempt budget exhausted"):
        smp.run(c["cvec"], c["centre"], torch.from_numpy(c["x"]).cuda(), c["T0"], max_attempts=budget)
    st = smp._read_states()[0]
    assert int(st["status"]) == 0 and budget <= int(st["n_attempts"]) < needed
    assert smp._attempt_hist == {}
    _reused_like_fresh(smp, c)
    print(f"EDGE budget contract T0=1 {B}x{K}: f64 attempts={needed} | budget {budget} -> budget error after n_attempts={int(st['n_attempts'])}; reuse == fresh")


def test_trajectory_capacity_failure_and_reuse():
    B, K = 2, 3
    c = _contract(B, K)
    smp = _sampler(c["e"], B, K)
    smp.TRAJ_CAP = 3
    big = _canary_traj(3 + len(c["sc"]["acc"]) + 64, B * K * 9)
    smp.traj = big[:3]
    with pytest.raises(RuntimeError, match="trajectory capacity"):
        smp.run(c["cvec"], c["centre"], torch.from_numpy(c["x"]).cuda(), c["T0"], return_process=True)
    assert bool((big[3:] == CANARY).all())
    assert smp._attempt_hist == {}, "a failed solve leaves no attempt-count expectation behind"
    _reused_like_fresh(smp, c)


@pytest.mark.parametrize("B,K", ec.SHAPES)
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_nonfinite_state_fails_the_solve(bad, B, K):
    """One component of the last row NaN / +inf (contract, T0 = 1).  scipy refuses such a y0 at construction (ValueError); the device does
    not look at the state, and what it does follows from its arithmetic:

    - the network: the bad component enters the pose encoder as float32; every hidden unit it reaches with a zero weight becomes NaN
      (0 x NaN, 0 x inf) and the ReLUs are fmaxf(v, 0) = 0 on NaN - so the stage derivatives of the row are finite (NaN) or +-inf / NaN
      (inf), those of every other row finite;
    - the norms: the element's own scale is atol + rtol |y| = NaN / inf, so y / scale, K / scale and err / scale are NaN (inf / inf for
      +inf) and every sum of squares the controller reads is NaN: d0, d1, d2 and every error norm;
    - the initial step: neither d0 < 1e-5 nor d1 < 1e-5 holds, h0 = 0.01 d0 / d1 = NaN, fmin(NaN, interval) = interval; h1 = NaN and
      fmin(fmin(100 h0, NaN), interval) = interval: the first attempt spans the whole interval;
    - every attempt: err = NaN, `err < 1` is false -> rejected, factor fmax(MIN_FACTOR, NaN) = MIN_FACTOR (the floor no finite analytic
      problem reaches); the step shrinks by 5 until begin_attempt finds h_abs < 10 ulp(T0) after a rejection: status -1 after
      ec.halving_attempts(T0, eps) attempts at the most, none accepted, and _solve raises scipy's TOO_SMALL_STEP message.
    The solve therefore fails, at its end instead of its start, and returns no poses.  The same sampler then works as a fresh one."""
    c = _contract(B, K)
    T0 = c["T0"]
    bound = ec.halving_attempts(T0, rr.EPS)
    direction = -1.0
    min_step = 10 * abs(np.nextafter(T0, direction * np.inf) - T0)
    assert bound == int(math.ceil(math.log((T0 - rr.EPS) / min_step) / math.log(5.0))) + 1
    x = torch.from_numpy(c["x"]).clone()
    x[-1, 4] = bad
    smp = _sampler(c["e"], B, K)
    out = None
    with pytest.raises(RuntimeError, match="step size"):
        out = smp.run(c["cvec"], c["centre"], x.cuda(), T0, max_attempts=4 * bound)
    assert out is None
    st = smp._read_states()[0]
    n = int(st["n_attempts"])
    assert int(st["status"]) == -1 and int(st["n_accepted"]) == 0
    assert 1 <= n <= bound, f"{n} attempts, the halving rule allows {bound}"
    assert int(st["nfev"]) == 2 + 6 * n
    assert not np.any(np.isfinite(st["log_err"])) and not st["log_acc"].any()
    # the MIN_FACTOR floor, by the rule of rr.replay_check: each step is clip_step of MIN_FACTOR x the one before, from the same t
    assert np.all(st["log_t"] == T0) and st["log_h"][0] == rr.EPS - T0
    worst = 0.0
    for i in range(n - 1):
        h_pred, _ = rr.clip_step(T0, rr.MIN_FACTOR * abs(st["log_h"][i]), direction, rr.EPS, True)
        dh = abs(st["log_h"][i + 1] - h_pred) / (4 * rr.U64 * abs(h_pred) + 4 * rr.U64 * T0)
        worst = max(worst, dh)
        assert dh <= 1.0, f"attempt {i + 1}: h {st['log_h'][i + 1]!r} vs MIN_FACTOR x the previous {h_pred!r}"
    assert rr.clip_step(T0, rr.MIN_FACTOR * abs(st["log_h"][n - 1]), direction, rr.EPS, True) is None, "the device stopped where scipy's rule stops"
    assert smp._attempt_hist == {}
    _reused_like_fresh(smp, c)
    print(f"EDGE nonfinite({bad}) contract T0=1 {B}x{K}: scipy ValueError | device n_attempts={n} (bound {bound}) nfev={int(st['nfev'])} status=-1 "
          f"floor={n} nan_err={int(np.isnan(st['log_err']).sum())} | worst/bound h={worst:.3g}; reuse == fresh")
