"""CPU (no GPU): the fixed-step Heun solve of the exact-likelihood ODE - its arithmetic against a Gaussian closed form
(tests/heun_likelihood_reference.py is the float64 restatement), the host schedule, the refusals by name and the C ABI's argument checks
(genpose_amd.samplers.HeunLikelihood / heun_likelihood_schedule, likelihood.cond_ode_likelihood(solver='heun'), gp_heun_likelihood_step)."""
import ctypes
import os
import re

import numpy as np
import pytest

import heun_likelihood_reference as hl
import heun_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gp_heun_likelihood_launches", "gp_heun_likelihood_step"]


# ------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("s0", [0.5, 0.05])
def test_second_order_on_the_gaussian_likelihood(s0, kind):
    """Data N(mu, s0^2 I): score = -(x - mu) / (s0^2 + sigma^2), tr J = -9 / (s0^2 + sigma^2); the truth is
    log N(x; mu, (s0^2 + sigma(eps)^2) I).  The worst error in bits over the rows at N = 16 / 32 / 64 falls by at least a factor 3 per
    doubling (second order: 4 asymptotically; the margin covers the pre-asymptotic range).  The ODE ends in the prior N(0, sigma_max^2 I)
    while the diffused data at T are N(mu, (s0^2 + sigma_max^2) I): that model error, about |z . mu| / sigma_max^2 + 4.5 s0^2 / sigma_max^2
    nats, is no discretisation error and does not fall with N, so mu is kept small (|mu| ~ 0.1: a floor near 5e-3 bits, a few per cent of
    the error at N = 64)."""
    rng = np.random.default_rng(0)
    mu = rng.standard_normal(9) * 0.03
    x = mu + rng.standard_normal((7, 9)) * np.sqrt(s0 * s0 + hr.sigma(hr.EPS) ** 2)
    truth = hl.gaussian_truth_bits(x, mu, s0)
    err = []
    for N in (16, 32, 64):
        _, _, bits = hl.solve(hl.gaussian_field(mu, s0), x, N, kind=kind)
        err.append(np.abs(bits - truth).max())
    print(f"s0={s0} {kind}: error in bits {err[0]:.3e} {err[1]:.3e} {err[2]:.3e} (|truth| <= {np.abs(truth).max():.3g})  "
          f"ratios {err[0] / err[1]:.2f} {err[1] / err[2]:.2f}")
    for a, b in zip(err, err[1:]):
        assert a / b >= 3.0, (err, a / b)


def test_reference_is_the_sampler_restatement_on_the_pose_part():
    """The x part of the ten-component solve is tests/heun_reference.py's Heun solver run on the ascending grid: same states, bit for bit."""
    rng = np.random.default_rng(2)
    mu, s0, N = np.zeros(9), 0.5, 8
    x = rng.standard_normal((3, 9)) * 0.4
    z, _, _ = hl.solve(hl.gaussian_field(mu, s0), x, N)
    t, sig, h = hl.grid(N)
    y = x.copy()
    score = hr.gaussian_score(s0)
    for i in range(N):
        d = -sig[i] * score(y, t[i])
        dp = -sig[i + 1] * score(y + h[i] * d, t[i + 1])
        y = y + h[i] * (0.5 * d + 0.5 * dp)
    assert np.array_equal(z, y)


# ------------------------------------------------------------------------------------------------ host schedule
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("N", [1, 6, 17])
def test_host_schedule_follows_the_launch_table(N, eps, kind):
    from genpose_amd import samplers
    t, sig, h = hl.grid(N, eps, 1.0, kind)
    t2, sched = samplers.heun_likelihood_schedule(N, eps, 1.0, kind)
    assert t2.dtype == np.float64 and np.array_equal(t2, t)
    assert t2[0] == eps and t2[-1] == 1.0 and np.all(np.diff(t2) > 0) and np.all(h > 0)
    # the same points as the sampler's grid, in ascending order
    td, sd = samplers.heun_grid(N, 1.0, eps, kind)
    assert np.array_equal(t2, td[::-1]) and np.array_equal(sig, sd[::-1])
    L = samplers.heun_likelihood_launches(N)
    assert L == 2 * N + 1 and sched.dtype == np.float32 and sched.shape == (L, 4)
    f = np.float32
    assert np.array_equal(sched[0], np.array([sig[0], 0, 0, 0]).astype(f))
    for i in range(N):
        last = i == N - 1
        assert np.array_equal(sched[2 * i + 1], np.array([sig[i + 1], -sig[i], h[i], 1.0]).astype(f))  # computed in float64, rounded once
        assert np.array_equal(sched[2 * i + 2], np.array([sig[i + 1], -sig[i + 1], h[i], 3.0 if last else 2.0]).astype(f))
    assert sched[:, 3].astype(int).tolist() == [0] + [1, 2] * (N - 1) + [1, 3]


def test_schedule_refuses_bad_arguments():
    from genpose_amd import samplers
    with pytest.raises(ValueError):
        samplers.heun_likelihood_schedule(0)
    with pytest.raises(ValueError):
        samplers.heun_likelihood_launches(0)
    with pytest.raises(ValueError):
        samplers.heun_likelihood_schedule(4, grid="cosine")
    with pytest.raises(ValueError):
        samplers.heun_likelihood_schedule(4, eps=1.0, T=1.0)
    with pytest.raises(ValueError):
        samplers.heun_likelihood_schedule(4, eps=0.0)


# ------------------------------------------------------------------------------------------------ refusals by name
def test_cond_ode_likelihood_refusals():
    """Raised before anything touches a device: tensors on the CPU, no network."""
    import torch
    from genpose_amd.likelihood import cond_ode_likelihood
    cvec, x = torch.zeros(1, 768), torch.zeros(2, 9)
    with pytest.raises(NotImplementedError, match="heun.*hutchinson"):
        cond_ode_likelihood(None, cvec, 2, x, torch.zeros(2, 9), solver="heun", steps=8, divergence="hutchinson")
    with pytest.raises(ValueError, match="steps"):
        cond_ode_likelihood(None, cvec, 2, x, None, solver="heun", steps=None, divergence="exact")
    with pytest.raises(NotImplementedError, match="euler"):
        cond_ode_likelihood(None, cvec, 2, x, None, solver="euler", divergence="exact")
    with pytest.raises(ValueError, match="cosine"):
        cond_ode_likelihood(None, cvec, 2, x, None, solver="heun", steps=4, grid="cosine", divergence="exact")


def test_agent_refusals_and_config_defaults():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    cfg = get_config()
    assert (cfg.likelihood_solver, cfg.likelihood_steps, cfg.likelihood_grid) == ("rk45", None, "geometric")
    net = PoseNet(get_config(device="cpu")).net
    with pytest.raises(NotImplementedError, match="heun.*hutchinson"):
        net.calc_likelihood({}, solver="heun", steps=8)
    with pytest.raises(ValueError, match="steps"):
        net.calc_likelihood({}, divergence="exact", solver="heun")
    with pytest.raises(NotImplementedError, match="euler"):
        net.calc_likelihood({}, divergence="exact", solver="euler")
    # the config values stand in for the arguments
    net = PoseNet(get_config(device="cpu", likelihood_solver="heun", likelihood_divergence="exact")).net
    with pytest.raises(ValueError, match="steps"):
        net({}, mode="likelihood")
    net = PoseNet(get_config(device="cpu", likelihood_solver="heun", likelihood_divergence="exact", likelihood_steps=8, likelihood_grid="cosine")).net
    with pytest.raises(ValueError, match="cosine"):
        net({}, mode="likelihood")


def test_runners_and_the_likelihood_ranker():
    from genpose_amd import evaluation
    from genpose_amd.config import get_config
    from genpose_amd.pipeline import FullPipelinePredictor
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import SingleFrameRunner, TrackingRunner
    sa = PoseNet(get_config(device="cpu"))
    ea = PoseNet(get_config(device="cpu", posenet_mode="energy"))
    with pytest.raises(NotImplementedError, match="likelihood"):
        TrackingRunner(sa, ea, ranker="likelihood")
    with pytest.raises(NotImplementedError, match="likelihood"):
        FullPipelinePredictor(sa, ea, 2, 4, 8, ranker="likelihood")
    TrackingRunner(sa, ea, use_graphs=False)
    assert SingleFrameRunner(sa).ranker == "energy" and SingleFrameRunner(sa, None, ranker="likelihood").energy_agent is None
    with pytest.raises(NotImplementedError, match="oracle"):
        SingleFrameRunner(sa, None, ranker="oracle")
    with pytest.raises(ValueError, match="energy agent"):
        SingleFrameRunner(sa).evaluate({})
    # 'likelihood_ranker' ranks by the array passed in `energy`, exactly as 'energy_ranker' does
    rng = np.random.default_rng(3)
    sRT = np.tile(np.identity(4), (2, 5, 1, 1))
    sRT[:, :, :3, 3] = rng.standard_normal((2, 5, 3))
    ll = rng.standard_normal((2, 5)).astype(np.float32)
    e = np.stack([ll, ll], axis=-1)
    a = evaluation.sort_sRT_by_energy(sRT, e, ranker="likelihood_ranker", ratio=0.6)
    b = evaluation.sort_sRT_by_energy(sRT, e, ranker="energy_ranker", ratio=0.6)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    order = np.argsort(-ll, axis=1)[:, :3]
    assert np.array_equal(a[0][:, :, :3, 3], np.take_along_axis(sRT[:, :, :3, 3], order[:, :, None], axis=1))
    with pytest.raises(NotImplementedError):
        evaluation.sort_sRT_by_energy(sRT, e, ranker="likelihood")


# ------------------------------------------------------------------------------------------------ C ABI
def _prototype(name):
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/genpose_hip.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbols_are_declared_bound_and_exported(name):
    from genpose_amd import _lib, build
    args = _prototype(name)
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(args), (name, len(sig), len(args))
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else "int"
        assert want == ("int" if ct is ctypes.c_int else "pointer"), (name, decl, ct)
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), name)
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    at = hdr.index("int " + name + "(")
    assert "samplers.py:22-99" in hdr[hdr.rindex("/*", 0, at):at], name


def test_launch_count():
    from genpose_amd import _lib, samplers
    L = _lib.lib()
    for N in (1, 2, 6, 32):
        assert L.gp_heun_likelihood_launches(N) == 2 * N + 1 == samplers.heun_likelihood_launches(N)
    assert L.gp_heun_likelihood_launches(0) == -1 and L.gp_heun_likelihood_launches(-3) == -1


def test_step_argument_checks_without_a_device():
    """Every GP_EINVAL case returns before anything touches the device, and so does R == 0 (GP_OK): host memory stands in for the
    buffers, which are never dereferenced."""
    from genpose_amd import _lib
    fn = _lib.lib().gp_heun_likelihood_step
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    names = [n for n, _ in _lib.GpScoreNet._fields_]
    full = _lib.GpScoreNet(**{n: p.value for n in names})
    N = 4
    good = [2, 3, 0, N, ctypes.byref(full)] + [p] * 9 + [None]  # nclouds, k, launch, nsteps, net, 9 buffers, stream
    for i in range(4, 14):  # null net / buffers
        bad = list(good)
        bad[i] = None
        assert fn(*bad) == -1, i
    for i, v in ((1, 0), (1, -2), (3, 0), (2, -1), (2, 2 * N + 1), (0, -1)):  # k, nsteps, launch, nclouds
        bad = list(good)
        bad[i] = v
        assert fn(*bad) == -1, (i, v)
    for missing in ("w_headx_t", "w_pose2_t", "w_pose0_t"):
        stripped = _lib.GpScoreNet(**{n: (None if n == missing else p.value) for n in names})
        bad = list(good)
        bad[4] = ctypes.byref(stripped)
        assert fn(*bad) == -1, missing
    ok = list(good)
    ok[0] = 0  # no rows: GP_OK, nothing launched
    for launch in (0, 1, 2 * N):
        ok[2] = launch
        assert fn(*ok) == 0
    assert all(v == 0.0 for v in buf)
