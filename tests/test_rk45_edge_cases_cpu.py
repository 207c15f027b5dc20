"""The float64 reference of tests/test_gpu_rk45_controller_edges.py held, on the CPU, to the conditions those tests rely on: every edge
problem of tests/rk45_edge_cases.py takes its named branch in scipy.integrate.RK45 itself, the strictly compared ones keep their error
norms away from every value at which the controller switches branch, the overflow problems overflow with room to spare, and the
restatement of scipy's controller (rk45_reference.replay_run) takes scipy's steps on the new branches too."""
import math

import numpy as np
import pytest
from scipy.integrate import RK45

import rk45_edge_cases as ec
import rk45_reference as rr

_REF = {}


def _ref(name, B, K):
    """the problem and its scipy solve, computed once per (entry, shape)"""
    key = (name, B, K)
    if key not in _REF:
        p = ec.setup(name, B, K)
        _REF[key] = (p, ec.scipy_reference(p))
    return _REF[key]


STRICT_CASES = [c for c in ec.CASES if ec.BY_NAME[c[0]].strict]


@pytest.mark.parametrize("name,B,K", ec.CASES)
def test_reference_takes_the_named_branch(name, B, K):
    from genpose_amd.samplers import ODESampler
    p, sc = _ref(name, B, K)
    e = p["edge"]
    bc = ec.branch_counts(sc, e.T0, e.t_bound)
    h0, h_abs, d0, d1, d2 = ec.initial_step_of(p)
    interval = abs(e.t_bound - e.T0)
    direction = np.sign(e.t_bound - e.T0)
    assert sc["ts"][-1] == e.t_bound, "scipy ends at t_bound bit for bit"
    assert sc["nfev"] == 2 + 6 * bc["attempts"]
    for b in e.branches:
        if b == "h0_tiny":
            assert (d0 < 1e-5 or d1 < 1e-5) and h0 == min(1e-6, interval)
        elif b == "h1_tiny":
            assert d1 <= 1e-15 and d2 <= 1e-15 and h_abs == min(100 * h0, max(1e-6, 1e-3 * h0), interval) == 1e-6
            assert sc["h"][0] == (e.T0 + direction * h_abs) - e.T0  # (rk.py: h = t_new - t)
        elif b == "interval":
            assert bc["interval"] == 1 and bc["attempts"] == 1 and h_abs == interval
            assert sc["h"][0] == e.t_bound - e.T0  # (t_new = t_bound, h = t_new - t)
        elif b == "min_step":
            # invisible from the outside (the clamped step is clipped to t_bound again): the restatement of rk.py's step start shows it
            min_step = 10 * abs(np.nextafter(e.T0, direction * np.inf) - e.T0)
            assert h_abs == interval < min_step
            assert rr.clip_step(e.T0, h_abs, direction, e.t_bound, True) is None, "the same step after a rejection fails the solve"
            h, t_new = rr.clip_step(e.T0, h_abs, direction, e.t_bound, False)
            assert t_new == e.t_bound and h == e.t_bound - e.T0 and abs(e.T0 + direction * min_step - e.T0) > interval
            assert bc["attempts"] == 1 and sc["h"][0] == h
        elif b == "err_zero":
            assert bc["err_zero"] == bc["attempts"] >= 2
            # every step is then exact: y never moves
            assert all(np.array_equal(s, sc["states"][0]) for s in sc["states"])
        elif b == "cap":
            assert bc["cap"] >= 1 and bc["err_zero"] == 0
            if e.strict:  # a capped attempt that is FOLLOWED by another attempt: the factor is used, not just computed
                follow = [i for i in range(bc["attempts"] - 1) if sc["acc"][i] and 0 < sc["err"][i] and ec.raw_factor(sc["err"][i]) > rr.MAX_FACTOR]
                assert follow and all(abs(sc["h"][i + 1]) <= rr.MAX_FACTOR * abs(sc["h"][i]) * (1 + 1e-15) for i in follow)
                assert any(abs(abs(sc["h"][i + 1]) - rr.MAX_FACTOR * abs(sc["h"][i])) <= 4 * rr.U64 * abs(sc["h"][i + 1]) for i in follow)
        elif b == "clamp":
            assert bc["clamp"] >= 1
        elif b == "log_cap":
            assert bc["attempts"] >= 560, "10 % over the 512 entries of the device's log"
        elif b == "traj_cap":
            assert bc["accepted"] >= math.ceil(1.1 * ODESampler.TRAJ_CAP)
        elif b == "dense_one":
            import scipy.integrate
            R = B * K
            sol = scipy.integrate.solve_ivp(rr.fun_flat(p["field"], R), (e.T0, e.t_bound), p["Y0"].reshape(-1), method="RK45", rtol=e.rtol,
                                            atol=e.atol, t_eval=np.linspace(e.T0, e.t_bound, e.num_steps))
            assert sol.y.shape == (R * 9, 1) and np.array_equal(sol.y[:, 0], p["Y0"].reshape(-1)), "scipy's dense output at T0 is y0"
        else:
            raise AssertionError(f"unknown branch {b}")


# error norms at which the controller takes another branch: accept / reject; the MAX_FACTOR cap; factor 1 (the clamp after a rejection);
# the MIN_FACTOR floor
SWITCH_POINTS = (1.0, (rr.SAFETY / rr.MAX_FACTOR) ** 5, rr.SAFETY ** 5, (rr.SAFETY / rr.MIN_FACTOR) ** 5)


@pytest.mark.parametrize("name,B,K", STRICT_CASES)
def test_strict_edges_keep_err_norm_away_from_every_switch(name, B, K):
    """The margin of test_rk45_reference_cpu.py::test_strict_problems_keep_err_norm_away_from_one - no float64 error norm within the
    float32 noise band rr.err_noise of 1, and a schedule that survives float32-size noise - and the same band around the other error
    norms at which the controller's factor changes form: the device's decisions and capped / clamped factors must then be scipy's."""
    p, sc = _ref(name, B, K)
    e = p["edge"]
    fun = rr.fun_flat(p["field"], B * K)
    k = 0
    for i, (t, h, acc) in enumerate(zip(sc["t"], sc["h"], sc["acc"])):
        y = sc["states"][k]
        _, _, _, err, stage_y = rr.dp_attempt(fun, t, y, fun(t, y), h, e.rtol, e.atol)
        assert err == pytest.approx(sc["err"][i], rel=1e-12, abs=1e-300)
        band = rr.err_noise(p["field"], t, y, h, stage_y, e.rtol, e.atol)
        # (the factor of the attempt that ends the solve is never used: only its accept / reject decision counts)
        for sw in SWITCH_POINTS[: 1 if i + 1 == len(sc["acc"]) else None]:
            assert abs(err - sw) > band, f"attempt {i} at t={t}: err_norm {err} within {band:.1e} of {sw}"
        k += int(acc)
    assert len(sc["states"]) <= 192
    if not e.exact:  # (the zero field has no float32 noise at all: its bound is 0)
        assert rr.robust_schedule(p["field"], e.T0, p["Y0"], e.t_bound, e.rtol, e.atol)


@pytest.mark.parametrize("name", [e.name for e in ec.EDGES if not e.strict and e.name != "dense_one_point"])
def test_path_sensitive_edges_are_so(name):
    """the edge solves exempt from the schedule comparison are exempt for a reason: an error norm inside the noise band of a switch point"""
    e = ec.BY_NAME[name]
    B, K = e.shapes[0]
    p, sc = _ref(name, B, K)
    fun = rr.fun_flat(p["field"], B * K)
    k, inside = 0, 0
    for t, h, acc in zip(sc["t"], sc["h"], sc["acc"]):
        y = sc["states"][k]
        _, _, _, err, stage_y = rr.dp_attempt(fun, t, y, fun(t, y), h, e.rtol, e.atol)
        band = rr.err_noise(p["field"], t, y, h, stage_y, e.rtol, e.atol)
        inside += any(abs(err - sw) <= band for sw in SWITCH_POINTS)
        k += int(acc)
    assert inside > 0 or not rr.robust_schedule(p["field"], e.T0, p["Y0"], e.t_bound, e.rtol, e.atol)


@pytest.mark.parametrize("name,B,K", STRICT_CASES)
def test_replay_run_takes_scipys_steps_on_the_edges(name, B, K):
    p, sc = _ref(name, B, K)
    e = p["edge"]
    log, states = rr.replay_run(rr.fun_flat(p["field"], B * K), e.T0, p["Y0"].reshape(-1), e.t_bound, e.rtol, e.atol)
    assert len(log) == len(sc["acc"]) and sc["nfev"] == 2 + 6 * len(log)
    np.testing.assert_array_equal([a["acc"] for a in log], sc["acc"])
    np.testing.assert_allclose([a["err"] for a in log], sc["err"], rtol=1e-14, atol=0)
    np.testing.assert_allclose([a["h"] for a in log], sc["h"], rtol=1e-14, atol=0)
    np.testing.assert_allclose([a["t"] for a in log], sc["t"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.stack(states), np.stack(sc["states"]), rtol=1e-14, atol=1e-14 * max(1.0, np.abs(p["Y0"]).max()))
    if e.exact:
        assert [a["h"] for a in log] == list(sc["h"]) and [a["t"] for a in log] == list(sc["t"])


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_scipy_refuses_a_nonfinite_initial_state(bad):
    """the reference behaviour the device's non-finite-state case is measured against: scipy never starts such a solve"""
    y0 = np.ones(9)
    y0[3] = bad
    with pytest.raises(ValueError):
        RK45(lambda t, y: -y, 1.0, y0, rr.EPS, rtol=1e-5, atol=1e-5)


def test_halving_bound_is_the_restated_controller_on_nan():
    """ec.halving_attempts is what the restated controller does when every error norm is NaN: rejected (NaN < 1 is false) with factor
    max(MIN_FACTOR, NaN) taken as MIN_FACTOR (fmax semantics of the device), from a first attempt over the whole interval"""
    for T0, t_bound in ((1.0, rr.EPS), (0.55, rr.EPS), (rr.EPS, 1.0)):
        direction = np.sign(t_bound - T0)
        h_abs, n, rejected = abs(t_bound - T0), 0, False
        while rr.clip_step(T0, h_abs, direction, t_bound, rejected) is not None:
            n += 1
            h_abs *= rr.MIN_FACTOR
            rejected = True
        assert n <= ec.halving_attempts(T0, t_bound) <= n + 1


def test_no_analytic_problem_reaches_the_min_factor_floor():
    """the record says the MIN_FACTOR floor is reached by the non-finite case only: the search behind that statement"""
    assert ec.search_min_factor_floor() == []
    for name, B, K in ec.CASES:
        p, sc = _ref(name, B, K)
        assert ec.branch_counts(sc, p["edge"].T0, p["edge"].t_bound)["floor"] == 0
