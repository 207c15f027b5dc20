"""CPU (no GPU): the fixed-step DPM-Solver++(2M) solver's arithmetic against a closed-form flow, its host schedule, launch count, C ABI,
the agent's contract and - on the trained score checkpoint, in float64 - its accuracy per evaluation against Heun's
(genpose_amd.samplers.Dpm2mSampler; tests/dpm2m_reference.py is the float64 restatement)."""
import ctypes
import os
import re

import numpy as np
import pytest

import dpm2m_reference as dr
import heun_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gp_dpm2m_launches", "gp_dpm2m_step_plan", "gp_dpm2m_step_bf16x9", "gp_dpm2m_solve_tile"]


# ------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55, 0.15])
@pytest.mark.parametrize("s", [0.05, 0.5, 3.0])
def test_second_order_on_the_gaussian_flow(s, T0, kind):
    """Data N(0, s^2 I): score -x / (s^2 + sigma^2), flow x(sigma) = x(sigma_0) sqrt((s^2 + sigma^2) / (s^2 + sigma_0^2)).  The relative
    error falls by a factor in [3.5, 4.5] from N = 64 to N = 128 (second order: 4)."""
    x0 = np.random.default_rng(0).standard_normal((7, 9)) * hr.sigma(T0)
    exact = hr.gaussian_flow(x0, s, T0, hr.EPS)
    err = []
    for N in (64, 128):
        x = dr.dpm2m_solve(hr.gaussian_score(s), x0, N, T0=T0, kind=kind)[-1]
        err.append(np.linalg.norm(x - exact) / np.linalg.norm(exact))
    print(f"s={s} T0={T0} {kind}: rel err {err[0]:.3e} {err[1]:.3e}  ratio {err[0] / err[1]:.2f}")
    assert 3.5 <= err[0] / err[1] <= 4.5, (err, err[0] / err[1])


@pytest.mark.parametrize("T0", [1.0, 0.15])
def test_one_step_is_the_closed_form_first_order_step(T0):
    """N = 1: x_1 = (sigma_1 / sigma_0) x_0 - expm1(-h_0) (x_0 + sigma_0^2 score(x_0, t_0)), h_0 = ln(sigma_0 / sigma_1)."""
    s = 0.5
    x0 = np.random.default_rng(2).standard_normal((4, 9)) * hr.sigma(T0)
    s0, s1 = hr.sigma(T0), hr.sigma(hr.EPS)
    D0 = x0 + s0 * s0 * hr.gaussian_score(s)(x0, T0)
    want = (s1 / s0) * x0 + (1.0 - s1 / s0) * D0  # -expm1(-h) = 1 - sigma_1 / sigma_0
    xs = dr.dpm2m_solve(hr.gaussian_score(s), x0, 1, T0=T0)
    assert xs.shape == (2, 4, 9) and np.array_equal(xs[0], x0)
    np.testing.assert_allclose(xs[1], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55])
def test_fp32_state_agrees_with_fp64_to_three_digits(T0, kind):
    """The device keeps its state in fp32: the device's order of operations on the host schedule's coefficients with every operation
    rounded to float32 lands within 1e-3 (relative) of the float64 loop as the method is written; in float64 the two forms agree to rounding."""
    s, N = 0.5, 32
    x0 = np.random.default_rng(1).standard_normal((5, 9)) * hr.sigma(T0)
    ref = dr.dpm2m_solve(hr.gaussian_score(s), x0, N, T0=T0, kind=kind)[-1]
    f = np.float32
    x = dr.dpm2m_solve_rounded(lambda x, t: (-x / f(s * s + hr.sigma(t) ** 2)).astype(f), x0, N, T0=T0, kind=kind)
    rel = np.linalg.norm(x - ref) / np.linalg.norm(ref)
    print(f"T0={T0} {kind}: fp32 against fp64, relative {rel:.3e}")
    assert x.dtype == np.float32 and rel < 1e-3
    x64 = dr.dpm2m_solve_rounded(hr.gaussian_score(s), x0, N, T0=T0, kind=kind, dtype=np.float64)
    assert np.linalg.norm(x64 - ref) / np.linalg.norm(ref) < 1e-12


# ------------------------------------------------------------------------------------------------ host schedule
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55, 0.15])
@pytest.mark.parametrize("N", [1, 6, 17])
def test_host_schedule_is_the_restatements_coefficients(N, T0, kind, denoise):
    from genpose_amd import samplers
    t, sig, _ = hr.grid(N, T0, hr.EPS, kind)
    want = dr.coefficients(sig)
    got = samplers.dpm2m_coefficients(samplers.heun_grid(N, T0, hr.EPS, kind)[1])
    for g, w in zip(got, want):
        assert g.dtype == np.float64 and np.array_equal(g, w)  # bit for bit in fp64
    s2, ratio, wc, wp = want
    assert wp[0] == 0.0 and np.all(wp[1:] < 0) and np.all(wc > 0) and np.all((0 < ratio) & (ratio < 1))
    # the weights sum to -expm1(-h) = 1 - sigma_{i+1} / sigma_i: a constant denoiser is integrated exactly
    np.testing.assert_allclose(wc + wp, 1.0 - ratio, rtol=1e-12, atol=0)
    t2, sched = samplers.dpm2m_schedule(N, T0, hr.EPS, kind, denoise=denoise)
    t3, _ = samplers.heun_schedule(N, T0, hr.EPS, kind, denoise=denoise)
    L = samplers.dpm2m_launches(N, denoise)
    assert np.array_equal(t2, t) and np.array_equal(t2, t3) and sched.dtype == np.float32 and sched.shape == (L, 8)
    f = np.float32
    assert np.array_equal(sched[0], np.array([sig[0], 0, 0, 0, 0, 0, 0, 0]).astype(f))
    for i in range(N):
        kind_i = 3.0 if i == N - 1 else 2.0
        assert np.array_equal(sched[i + 1], np.array([sig[i + 1], s2[i], ratio[i], kind_i, wc[i], wp[i], 0, 0]).astype(f))  # rounded once
    if denoise:
        g = f(sig[N]) * f(4.1272735595703125)
        assert np.array_equal(sched[N + 1], np.array([f(sig[N]), g, f((1.0 - hr.EPS) / N), 4.0, 0, 0, 0, 0], dtype=f))
        hs = samplers.heun_schedule(N, T0, hr.EPS, kind, denoise=True)[1]
        assert np.array_equal(sched[N + 1, :4], hs[2 * N + 1])  # HEUN_DENOISE's row


def test_schedule_refuses_bad_arguments():
    from genpose_amd import samplers
    with pytest.raises(ValueError):
        samplers.dpm2m_schedule(0)
    with pytest.raises(ValueError):
        samplers.dpm2m_schedule(4, grid="cosine")
    with pytest.raises(ValueError):
        samplers.dpm2m_schedule(4, T0=1e-6)
    with pytest.raises(ValueError):
        samplers.dpm2m_launches(0)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("N", [1, 2, 6, 32])
def test_launch_count_and_nfe(N, denoise):
    """N + 1 launches, one more with denoise; every launch but the last evaluates: NFE = N (+ 1) - half of Heun's 2 N (+ 1)."""
    from genpose_amd import _lib, samplers
    L = samplers.dpm2m_launches(N, denoise)
    assert L == N + 1 + (1 if denoise else 0) and L - 1 == N + (1 if denoise else 0)
    assert _lib.lib().gp_dpm2m_launches(N, int(denoise)) == L
    assert samplers.heun_launches(N, denoise) - L == N
    _, sched = samplers.dpm2m_schedule(N, denoise=denoise)
    assert sched[:, 3].astype(int).tolist() == [0] + [2] * (N - 1) + ([3, 4] if denoise else [3])
    assert _lib.lib().gp_dpm2m_launches(0, 1) == -1


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


def test_entry_points_share_heuns_prototypes():
    for mine, heuns in [("gp_dpm2m_launches", "gp_heun_launches"), ("gp_dpm2m_step_plan", "gp_heun_step_plan"),
                        ("gp_dpm2m_step_bf16x9", "gp_heun_step_bf16x9"), ("gp_dpm2m_solve_tile", "gp_heun_solve_tile")]:
        assert _prototype(mine) == _prototype(heuns), mine
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    for name in NEW_SYMBOLS:
        at = hdr.index("int " + name + "(")
        assert hdr[:at].rstrip().endswith("*/"), f"{name}: no comment in front of the declaration"


def test_plan_and_argument_refusals_need_no_gpu():
    """GP_EINVAL before anything touches a device: the head-split plan, plan 128 for the one-launch form, counts and null buffers."""
    from genpose_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)  # never dereferenced: every call below is refused first
    net = ctypes.pointer(_lib.GpScoreNet())  # (the bf16x9 entry point checks the alignment of its pointers: all null)
    good = dict(tile=16, ngroups=1, nb=3, k=50, launch=1, nsteps=4, denoise=1, net=net, cvec=one, tvec=one, sched=one, centre=one, x=one, d=one,
                score=one, out=one, traj=one)
    step = ("tile", "ngroups", "nb", "k", "launch", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj")
    solve = tuple(k for k in step if k != "launch")
    bad = [dict(tile=16 | _lib.PLAN_HEADSPLIT), dict(tile=48), dict(nsteps=0), dict(ngroups=0), dict(k=0), dict(tile=128, k=5, nb=30), dict(ngroups=2, tile=128)]
    bad += [{name: None} for name in ("net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out")]
    for change in bad:
        a = dict(good, **change)
        assert L.gp_dpm2m_step_plan(*[a[k] for k in step], None) == -1, change
        assert L.gp_dpm2m_solve_tile(*[a[k] for k in solve], None) == -1, change
        if "tile" not in change or change.get("k") == 5:
            assert L.gp_dpm2m_step_bf16x9(*[a[k] for k in step[1:]], one, one, one, None) == -1, change
    for change in (dict(launch=-1), dict(launch=6), dict(launch=5, denoise=0)):  # N = 4: launches 0 .. 5 with denoise, 0 .. 4 without
        a = dict(good, **change)
        assert L.gp_dpm2m_step_plan(*[a[k] for k in step], None) == -1, change
        assert L.gp_dpm2m_step_bf16x9(*[a[k] for k in step[1:]], one, one, one, None) == -1, change
    a = dict(good, tile=128)
    assert L.gp_dpm2m_solve_tile(*[a[k] for k in solve], None) == -1  # the chain form keeps its per-launch kernels


# ------------------------------------------------------------------------------------------------ agent contract
def test_agent_contract_on_the_cpu():
    from genpose_amd.config import encoder_precision_of, get_config
    from genpose_amd.posenet_agent import PoseNet
    with pytest.raises(ValueError, match="sampling_steps"):
        PoseNet(get_config(device="cpu", sampler_mode=["dpm2m"], sampling_steps=None)).net.sample({}, "dpm2m")
    with pytest.raises(NotImplementedError, match="dpm2m"):
        PoseNet(get_config(device="cpu", sampler_mode=["dpm2m"], sampling_steps=8, posenet_mode="energy")).net.sample({}, "dpm2m")
    with pytest.raises(NotImplementedError, match="dpm2m"):
        PoseNet(get_config(device="cpu", sampler_mode=["dpm2m"], sampling_steps=8, posenet_mode="energy")).net({}, mode="dpm2m_sample")
    with pytest.raises(ValueError, match="heun_grid"):
        PoseNet(get_config(device="cpu", sampler_mode=["dpm2m"], sampling_steps=8, heun_grid="cosine")).net.sample({}, "dpm2m")
    assert encoder_precision_of(get_config(sampler_mode=["dpm2m"], sampling_steps=8)) == "f32"
    # no default has moved
    cfg = get_config()
    assert cfg.sampler_mode == ["ode"] and cfg.heun_grid == "geometric"


def test_trackers_name_the_solver():
    import inspect
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import FixedStepTracker, TrackingRunner
    sa = PoseNet(get_config(device="cpu", sampler_mode=["dpm2m"], sampling_steps=8))
    ea = PoseNet(get_config(device="cpu", posenet_mode="energy"))
    with pytest.raises(NotImplementedError, match="dpm2m"):
        TrackingRunner(sa, ea, use_graphs=True)
    TrackingRunner(sa, ea, use_graphs=False)
    assert inspect.signature(FixedStepTracker.__init__).parameters["solver"].default == "heun"
    assert FixedStepTracker.SOLVERS == ("heun", "dpm2m")
    with pytest.raises(ValueError, match="solver"):
        FixedStepTracker(sa, ea, solver="euler")


def test_sampler_class_shares_heuns_constructor():
    import inspect
    from genpose_amd.samplers import Dpm2mSampler, HeunSampler
    assert issubclass(Dpm2mSampler, HeunSampler)
    assert inspect.signature(Dpm2mSampler.__init__) == inspect.signature(HeunSampler.__init__)
    assert inspect.signature(Dpm2mSampler.run) == inspect.signature(HeunSampler.run)
    assert Dpm2mSampler.LAUNCHES == ("chain", "single") and Dpm2mSampler.SCHED_ROW == 8 and HeunSampler.SCHED_ROW == 4


# ------------------------------------------------------------------------------------------------ accuracy per evaluation
def _rotation_distance_deg(a, b):
    def R(p):
        p = hr.normalize_rot6(p)
        c1, c2 = p[:, 0:3], p[:, 3:6]
        return np.stack([c1, c2, np.cross(c1, c2)], -1)
    tr = np.einsum("nij,nij->n", R(a), R(b))
    return np.degrees(np.arccos(np.clip((tr - 1) / 2, -1, 1)))


def test_sixteen_evaluations_beat_heuns_sixteen_on_the_trained_score_network():
    """Float64, the trained score checkpoint, 6 held-out synthetic clouds x 20 candidates from T0 = 0.55 on the geometric grid.  Reference:
    the Heun restatement at N = 512.  At NFE 16 the median rotation distance to it of DPM-Solver++(2M) (N = 16) is below that of Heun
    (N = 8).  Measured: 0.41 against 1.06 degrees; the condition is "smaller", not a fitted factor."""
    import torch
    from genpose_amd import synth
    from oracle import genpose_oracle as go
    B, K, T0 = 6, 20, 0.55
    ckpt = torch.load(os.path.join(ROOT, "tests", "golden", "trained", "ckpt_score.pth"), map_location="cpu")["model_state_dict"]
    sd = {k: v.double() for k, v in ckpt.items()}
    pts = torch.from_numpy(synth.posed_batch(range(1_000_000, 1_000_000 + B))["pts"])
    feat = torch.as_tensor(go.encoder_forward({k: v.float() for k, v in ckpt.items()}, pts.float())).double()
    feat_r = feat.repeat_interleave(K, 0)

    def score(x, t):
        tt = torch.full((B * K, 1), t, dtype=torch.float64)
        return go.score_forward(sd, feat_r, torch.from_numpy(np.ascontiguousarray(x)), tt).numpy()

    x0 = (torch.randn(B * K, 9, generator=torch.Generator().manual_seed(3), dtype=torch.float64) * hr.sigma(T0)).numpy()
    ref = hr.heun_solve(score, x0, 512, T0=T0)[-1]
    heun = float(np.median(_rotation_distance_deg(hr.heun_solve(score, x0, 8, T0=T0)[-1], ref)))
    dpm = float(np.median(_rotation_distance_deg(dr.dpm2m_solve(score, x0, 16, T0=T0)[-1], ref)))
    print(f"median rotation distance to Heun N = 512 at NFE 16: DPM-Solver++(2M) N = 16 {dpm:.3f} deg, Heun N = 8 {heun:.3f} deg")
    assert dpm < heun, (dpm, heun)
