"""CPU (no GPU): the fixed-step Heun solver's arithmetic against a closed-form flow, its host schedule, launch count, C ABI and the
agent's contract (genpose_amd.samplers.HeunSampler; tests/heun_reference.py is the float64 restatement)."""
import ctypes
import os
import re

import numpy as np
import pytest

import heun_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gp_heun_launches", "gp_heun_layout", "gp_heun_step_plan", "gp_heun_step_bf16x9"]


# ------------------------------------------------------------------------------------------------ arithmetic
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55])
@pytest.mark.parametrize("s", [0.5, 0.05])
def test_second_order_on_the_gaussian_flow(s, T0, kind):
    """Data N(0, s^2 I): score -x / (s^2 + sigma^2), flow x(sigma) = x(sigma_0) sqrt((s^2 + sigma^2) / (s^2 + sigma_0^2)).  The relative
    error at N = 16, 32, 64 falls by a factor in [3.5, 5] per doubling (second order: 4)."""
    x0 = np.random.default_rng(0).standard_normal((7, 9)) * hr.sigma(T0)
    exact = hr.gaussian_flow(x0, s, T0, hr.EPS)
    err = []
    for N in (16, 32, 64):
        x = hr.heun_solve(hr.gaussian_score(s), x0, N, T0=T0, kind=kind)[-1]
        err.append(np.linalg.norm(x - exact) / np.linalg.norm(exact))
    print(f"s={s} T0={T0} {kind}: rel err {err[0]:.3e} {err[1]:.3e} {err[2]:.3e}  ratios {err[0] / err[1]:.2f} {err[1] / err[2]:.2f}")
    for a, b in zip(err, err[1:]):
        assert 3.5 <= a / b <= 5.0, (err, a / b)


def test_fp32_state_agrees_with_fp64_to_three_digits():
    """The device keeps its state in fp32: the same loop with every operation rounded to float32 lands within 1e-3 (relative) of float64."""
    s, T0, N = 0.5, 1.0, 32
    x0 = np.random.default_rng(1).standard_normal((5, 9)) * hr.sigma(T0)
    ref = hr.heun_solve(hr.gaussian_score(s), x0, N, T0=T0)[-1]
    t, sig, h = hr.grid(N, T0)
    f = np.float32
    x = x0.astype(f)
    sc = lambda x, t: (-x / f(s * s + hr.sigma(t) ** 2)).astype(f)
    for i in range(N):
        d = f(-sig[i]) * sc(x, t[i])
        xe = x + f(h[i]) * d
        dp = f(-sig[i + 1]) * sc(xe, t[i + 1])
        x = x + f(h[i]) * (f(0.5) * d + f(0.5) * dp)
    assert x.dtype == np.float32
    assert np.linalg.norm(x - ref) / np.linalg.norm(ref) < 1e-3


# ------------------------------------------------------------------------------------------------ host schedule
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("kind", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55, 0.15])
@pytest.mark.parametrize("N", [1, 6, 17])
def test_host_schedule_is_the_restatements_grid(N, T0, kind, denoise):
    from genpose_amd import samplers
    t, sig, h = hr.grid(N, T0, hr.EPS, kind)
    th, sh = samplers.heun_grid(N, T0, hr.EPS, kind)
    assert th.dtype == np.float64 and np.array_equal(th, t) and np.array_equal(sh, sig)  # bit for bit in fp64
    assert t[0] == T0 and t[-1] == hr.EPS and np.all(np.diff(t) < 0) and np.all(h < 0)
    t2, sched = samplers.heun_schedule(N, T0, hr.EPS, kind, denoise=denoise)
    L = samplers.heun_launches(N, denoise)
    assert np.array_equal(t2, t) and sched.dtype == np.float32 and sched.shape == (L, 4)
    f = np.float32
    assert sched[0, 0] == f(sig[0]) and sched[0, 3] == 0
    for i in range(N):
        last = i == N - 1 and not denoise
        assert np.array_equal(sched[2 * i + 1], np.array([sig[i + 1], -sig[i], h[i], 1.0]).astype(f))  # rounded once
        assert np.array_equal(sched[2 * i + 2, 1:], np.array([-sig[i + 1], h[i], 3.0 if last else 2.0]).astype(f))
        if not last:
            assert sched[2 * i + 2, 0] == f(sig[i + 1])
    if denoise:
        g = f(sig[N]) * f(4.1272735595703125)
        assert np.array_equal(sched[2 * N + 1, 1:], np.array([g, f((1.0 - hr.EPS) / N), 4.0], dtype=f))
        assert abs(float(g) - hr.sigma(hr.EPS) * hr.G_FACTOR) < 1e-6 * float(g)


def test_schedule_refuses_bad_arguments():
    from genpose_amd import samplers
    with pytest.raises(ValueError):
        samplers.heun_grid(0)
    with pytest.raises(ValueError):
        samplers.heun_grid(4, grid="cosine")
    with pytest.raises(ValueError):
        samplers.heun_grid(4, T0=1e-6)


@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("N", [1, 2, 6, 32])
def test_launch_count_and_nfe(N, denoise):
    """2 N + 1 launches, one more with denoise; every launch but the last evaluates: NFE = 2 N (+ 1)."""
    from genpose_amd import _lib, samplers
    L = samplers.heun_launches(N, denoise)
    assert L == 2 * N + 1 + (1 if denoise else 0) and L - 1 == 2 * N + (1 if denoise else 0)
    assert _lib.lib().gp_heun_launches(N, int(denoise)) == L
    _, sched = samplers.heun_schedule(N, denoise=denoise)
    kinds = sched[:, 3].astype(int).tolist()
    assert kinds == [0] + [1, 2] * (N - 1) + ([1, 2, 4] if denoise else [1, 3])
    assert _lib.lib().gp_heun_launches(0, 1) == -1


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


def test_header_cites_the_reference_and_the_two_step_entry_points_share_their_buffers():
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    for name in NEW_SYMBOLS:
        at = hdr.index("int " + name + "(")
        comment = hdr[hdr.rindex("/*", 0, at):at]
        assert "samplers.py:230-290" in comment, name
    a, b = _prototype("gp_heun_step_plan"), _prototype("gp_heun_step_bf16x9")
    packs = ["const void *w_pose0_x9", "const void *w_pose2_x9", "const void *w_headx_x9"]
    assert b == a[1:-1] + packs + [a[-1]] and a[0] == "int tile"


def test_layout_shares_the_pc_planner_minus_head_split():
    """Without a GPU the planner assumes a fixed CU count: whatever gp_pc_layout picks for the score model, gp_heun_layout picks too, with
    whole 16-row tiles where the PC planner splits the heads; the head-split plan is refused by name."""
    from genpose_amd import _lib
    L = _lib.lib()
    t, tp, n = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    for groups, B, K in [(1, 5, 50), (1, 64, 50), (1, 256, 50), (10, 64, 50), (1, 3, 5), (2, 3, 50), (1, 640, 50)]:
        rc = L.gp_pc_layout(0, 0, groups, B, K, ctypes.byref(tp), ctypes.byref(n))
        assert L.gp_heun_layout(0, groups, B, K, ctypes.byref(t)) == rc and rc == (-1 if (groups, B, K) == (2, 3, 50) else 0)  # 150 rows per batch: no tile fits
        assert rc != 0 or t.value == tp.value & ~_lib.PLAN_HEADSPLIT, (groups, B, K)
    t.value = -7
    assert L.gp_heun_layout(16 | _lib.PLAN_HEADSPLIT, 1, 5, 50, ctypes.byref(t)) == -1 and t.value == -7
    assert L.gp_heun_layout(48, 1, 5, 50, ctypes.byref(t)) == -1
    assert L.gp_heun_layout(128, 2, 3, 50, ctypes.byref(t)) == -1  # 150 rows per batch: a workgroup would straddle two
    assert L.gp_heun_layout(128, 1, 3, 5, ctypes.byref(t)) == -1   # k = 5: a workgroup's rows would span more than four clouds
    assert L.gp_heun_layout(0, 1, 5, 50, None) == -1 and t.value == -7


# ------------------------------------------------------------------------------------------------ agent contract
def test_agent_contract_on_the_cpu():
    from genpose_amd.config import encoder_precision_of, get_config
    from genpose_amd.posenet_agent import PoseNet
    assert get_config().heun_grid == "geometric"
    with pytest.raises(ValueError, match="sampling_steps"):
        PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=None)).net.sample({}, "heun")
    with pytest.raises(NotImplementedError, match="heun"):
        PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=8, posenet_mode="energy")).net.sample({}, "heun")
    with pytest.raises(NotImplementedError, match="heun"):
        PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=8, posenet_mode="energy")).net({}, mode="heun_sample")
    with pytest.raises(ValueError, match="heun_grid"):
        PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=8, heun_grid="cosine")).net.sample({}, "heun")
    # encoder_level2 'auto' keeps the fp32 MFMA kernels for this sampler
    assert encoder_precision_of(get_config(sampler_mode=["heun"], sampling_steps=8)) == "f32"


def test_frame_graphs_refuse_a_heun_agent_by_name():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import TrackingRunner
    sa = PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=8))
    ea = PoseNet(get_config(device="cpu", posenet_mode="energy"))
    with pytest.raises(NotImplementedError, match="heun"):
        TrackingRunner(sa, ea, use_graphs=True)
    TrackingRunner(sa, ea, use_graphs=False)
