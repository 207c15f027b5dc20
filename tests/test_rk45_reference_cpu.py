"""The float64 ground truth of tests/test_gpu_rk45_exact.py checked on the CPU: the analytic-field state dicts through the oracle's
networks, the exact solutions against DOP853, the attempt / controller replay against scipy's RK45 itself, and the property of every
analytic problem that makes a strict schedule comparison with the float32 device legitimate."""
import numpy as np
import pytest
import torch

import rk45_reference as rr
from oracle import genpose_oracle as go


def _sd64(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}


@pytest.mark.parametrize("name", ["contract", "time", "energy", "likelihood"])
def test_analytic_state_dict_is_the_closed_form_field(name):
    net, _ = rr.problems()[name]
    template = go.make_state_dict(0, "score")
    sd = net.state_dict(template)
    assert sd.keys() == template.keys() and all(sd[k].shape == template[k].shape and sd[k].dtype == template[k].dtype for k in sd)
    sd = _sd64(sd)
    B, K = 3, 7
    gen = torch.Generator().manual_seed(5)
    pf = torch.randn(B, 1024, generator=gen, dtype=torch.float64).abs()
    feat = pf.repeat_interleave(K, 0)
    c = np.repeat(net.offsets(pf.numpy()), K, 0)
    x = torch.randn(B * K, 9, generator=gen, dtype=torch.float64) * 3
    probe = torch.randn(B * K, 9, generator=gen, dtype=torch.float64)
    for t in (1e-5, 0.15, 0.55, 1.0):
        tt = torch.full((B * K, 1), t, dtype=torch.float64)
        f = go._trunk(sd, feat, x, tt).numpy()
        ref = net.f_theta(t, x.numpy(), c)
        np.testing.assert_allclose(f, ref, rtol=0, atol=1e-12 * max(1.0, np.abs(ref).max()))
        # energy model's score = d/dx <x, f / sigma> = ((A + A^T) x + c + d tau) / sigma, its energy <x, f> / sigma
        g, e = go.energy_score(sd, feat, x, tt)
        sig = rr.sigma(t)
        e_ref = np.sum(x.numpy() * ref, axis=1) / sig
        g_ref = (ref + x.numpy() @ net.A) / sig
        np.testing.assert_allclose(e.numpy(), e_ref, rtol=0, atol=1e-12 * np.abs(e_ref).max())
        np.testing.assert_allclose(g.numpy(), g_ref, rtol=0, atol=1e-12 * np.abs(g_ref).max())
        # likelihood: score f / (sigma + 1e-7), Hutchinson term eps^T A eps / (sigma + 1e-7)
        s, div = go.score_and_divergence(sd, feat, x, tt, probe)
        div_ref = np.einsum("ri,ij,rj->r", probe.numpy(), net.A, probe.numpy()) / (sig + 1e-7)
        np.testing.assert_allclose(s.numpy(), ref / (sig + 1e-7), rtol=0, atol=1e-12 * np.abs(ref / sig).max())
        np.testing.assert_allclose(div.numpy(), div_ref, rtol=0, atol=1e-12 * max(1.0, np.abs(div_ref).max()))
        # the Field classes are the driver's right-hand sides of these
        for model in ("score", "energy", "likelihood"):
            Y = x.numpy() if model != "likelihood" else np.concatenate([x.numpy(), np.zeros((B * K, 1))], 1)
            fld = rr.Field(net, model, c, probe.numpy())(t, Y)
            want = {"score": -0.5 * rr.g2(t) * ref / (sig + 1e-7), "energy": -0.5 * rr.g2(t) * g_ref,
                    "likelihood": -0.5 * rr.g2(t) * np.concatenate([ref / (sig + 1e-7), div_ref[:, None]], 1)}[model]
            np.testing.assert_allclose(fld, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())


@pytest.mark.parametrize("name,T0", [("contract", 1.0), ("time", 1.0), ("time", 0.55), ("energy", 1.0), ("likelihood", rr.EPS)])
def test_exact_solution_matches_dop853(name, T0):
    net, model = rr.problems()[name]
    lik = model == "likelihood"
    B, K = 2, 5
    pf, x, probe = rr.inputs(B, K, T0, likelihood=lik)
    c = np.repeat(net.offsets(pf), K, 0)
    t1 = 1.0 if lik else rr.EPS
    mid = 0.5 * (T0 + t1)
    got = rr.exact_solution(net, "energy" if model == "energy" else "score", x.astype(np.float64), c, T0, [T0, mid, t1])
    np.testing.assert_array_equal(got[0], x.astype(np.float64))
    fld = rr.Field(net, model, c, probe)
    Y0 = np.concatenate([x, np.zeros((B * K, 1))], 1) if lik else x.astype(np.float64)
    for k, tt in ((1, mid), (2, t1)):
        ref = rr.dop853_solution(fld, Y0, T0, tt)
        np.testing.assert_allclose(got[k], ref[:, :9], rtol=1e-10, atol=1e-10 * np.abs(ref).max())
    if lik:
        z, dlogp, bits = rr.exact_likelihood(net, x.astype(np.float64), probe.astype(np.float64), c)
        ref = rr.dop853_solution(fld, Y0, rr.EPS, 1.0)
        np.testing.assert_allclose(z, ref[:, :9], rtol=1e-10, atol=1e-10 * np.abs(ref).max())
        np.testing.assert_allclose(dlogp, ref[:, 9], rtol=1e-10, atol=1e-10 * np.abs(ref[:, 9]).max())
        assert np.all(np.isfinite(bits))


@pytest.mark.parametrize("name,T0", [("contract", 1.0), ("time", 1.0), ("time", 0.55), ("energy", 1.0), ("likelihood", rr.EPS)])
def test_replay_reproduces_scipy_rk45(name, T0):
    """the helper's attempt + controller, run as a whole solve, take scipy's own steps: err_norm, h and accept / reject sequence"""
    net, model = rr.problems()[name]
    lik = model == "likelihood"
    B, K = 2, 10
    pf, x, probe = rr.inputs(B, K, T0, likelihood=lik)
    c = np.repeat(net.offsets(pf), K, 0)
    fld = rr.Field(net, model, c, probe)
    Y0 = np.concatenate([x, np.zeros((B * K, 1))], 1) if lik else x.astype(np.float64)
    t1 = 1.0 if lik else rr.EPS
    fun = rr.fun_flat(fld, B * K)
    sc = rr.scipy_run(fun, T0, Y0.reshape(-1), t1)
    log, states = rr.replay_run(fun, T0, Y0.reshape(-1), t1)
    assert len(log) == len(sc["acc"]) and sc["nfev"] == 2 + 6 * len(log)
    np.testing.assert_array_equal([a["acc"] for a in log], sc["acc"])
    np.testing.assert_allclose([a["err"] for a in log], sc["err"], rtol=1e-14, atol=0)
    np.testing.assert_allclose([a["h"] for a in log], sc["h"], rtol=1e-14, atol=0)
    np.testing.assert_allclose([a["t"] for a in log], sc["t"], rtol=1e-14, atol=0)
    np.testing.assert_allclose(np.stack(states), np.stack(sc["states"]), rtol=1e-14, atol=1e-14 * np.abs(Y0).max())
    if name == "time" and T0 == 1.0:
        assert not sc["acc"].all(), "the time-forced problem must exercise rejected attempts"


# (problem, T0, clouds, candidates): every analytic solve whose whole schedule the GPU tests compare with scipy's, attempt for attempt
STRICT_SOLVES = [("contract", 1.0, 4, 50), ("contract", 0.15, 4, 50), ("contract", 1.0, 256, 50), ("energy", 1.0, 4, 50),
                 ("likelihood", rr.EPS, 4, 50)]
# solves the GPU tests hold to the float64 replay and the exact solution only: their schedule is path-sensitive (it changes under
# float32-size noise in the evaluations), so no float32 device can be held to scipy's on them
PATH_SENSITIVE = [("contract", 0.55, 4, 50), ("time", 1.0, 4, 50), ("time", 0.55, 4, 50), ("energy", 0.55, 4, 50)]


def _solve_setup(name, T0, B, K):
    net, model = rr.problems()[name]
    lik = model == "likelihood"
    pf, x, probe = rr.inputs(B, K, T0, likelihood=lik)
    c = np.repeat(net.offsets(pf), K, 0)
    fld = rr.Field(net, model, c, probe)
    Y0 = np.concatenate([x, np.zeros((B * K, 1))], 1) if lik else x.astype(np.float64)
    return fld, Y0, (1.0 if lik else rr.EPS)


@pytest.mark.parametrize("name,T0,B,K", STRICT_SOLVES)
def test_strict_problems_keep_err_norm_away_from_one(name, T0, B, K):
    """No float64 attempt of a strictly compared solve has an error norm within the float32 noise band around 1, and its schedule
    survives float32-size noise in every evaluation: the device's decisions must then be scipy's, attempt for attempt."""
    fld, Y0, t1 = _solve_setup(name, T0, B, K)
    fun = rr.fun_flat(fld, B * K)
    log, states = rr.replay_run(fun, T0, Y0.reshape(-1), t1)
    k = 0
    for a in log:
        y = states[k]
        _, _, _, err, stage_y = rr.dp_attempt(fun, a["t"], y, fun(a["t"], y), a["h"], 1e-5, 1e-5)
        band = rr.err_noise(fld, a["t"], y, a["h"], stage_y)
        assert abs(err - 1.0) > band, f"attempt at t={a['t']}: err_norm {err} within {band:.1e} of 1"
        k += a["acc"]
    assert len(states) <= 192  # the device's trajectory capacity (ODESampler.TRAJ_CAP)
    assert rr.robust_schedule(fld, T0, Y0, t1)
    if name in ("energy", "likelihood"):
        assert not all(a["acc"] for a in log), "a strictly compared solve with rejected attempts"


@pytest.mark.parametrize("name,T0,B,K", PATH_SENSITIVE)
def test_path_sensitive_problems_are_so(name, T0, B, K):
    """the solves exempt from the schedule comparison really are path-sensitive (the exemption is not a convenience)"""
    fld, Y0, t1 = _solve_setup(name, T0, B, K)
    assert not rr.robust_schedule(fld, T0, Y0, t1)


def test_exact_f32_problem_is_the_closed_form_field():
    net = rr.exact_f32_problem()
    assert np.all(np.log2(-np.diag(net.A)) == np.round(np.log2(-np.diag(net.A)))) and np.all(net.A == np.diag(np.diag(net.A)))
    sd = _sd64(net.state_dict(go.make_state_dict(0, "score")))
    x = torch.randn(20, 9, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    f = go._trunk(sd, torch.rand(20, 1024, dtype=torch.float64), x, torch.full((20, 1), 0.4, dtype=torch.float64)).numpy()
    np.testing.assert_array_equal(f, x.numpy() @ net.A.T)


def test_netfield_bound_covers_float32_trunk():
    """the float64 field for arbitrary weights and its float32 error bound: the oracle's trunk run in float32 stays inside it"""
    sd = go.make_state_dict(0, "score")
    gen = torch.Generator().manual_seed(4)
    pf = torch.randn(2, 1024, generator=gen).abs()
    fld = rr.NetField(sd, pf.numpy(), 10)
    for t in (1e-5, 0.3, 1.0):
        Y = (torch.randn(20, 9, generator=gen, dtype=torch.float64) * rr.sigma(t)).numpy()
        f64 = fld(t, Y)
        f32 = rr.a_score(t) * go._trunk(sd, pf.repeat_interleave(10, 0), torch.from_numpy(Y).float(), torch.full((20, 1), t)).double().numpy()
        b = fld.bound(t, Y)
        assert np.all(np.abs(f32 - f64) <= b)
        assert np.max(b) < 5e-2 * np.max(np.abs(f64))  # a rounding bound, not a blanket one
