"""CPU (no GPU): the exact-divergence likelihood's host side - argument errors of cond_ode_likelihood / calc_likelihood, the ctypes binding of
gp_score_div_exact against the header, the model value of the RK45 driver, and the float64 ground truth the GPU tests build on
(tests/exact_likelihood_ref.py: closed form == autograd; the share of rows a ReLU kink makes unstable stays under the GPU test's limit)."""
import os
import re

import numpy as np
import pytest
import torch

import exact_likelihood_ref as er
from oracle import genpose_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "genpose_hip.h")).read()


def test_entry_is_declared_bound_and_exported():
    from genpose_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    m = re.search(r"\bint\s+gp_score_div_exact\s*\(([^)]*)\)\s*;", hdr)
    assert m, "gp_score_div_exact is not declared in include/genpose_hip.h"
    params = [a.strip() for a in m.group(1).split(",")]
    sig = _lib.SIGNATURES["gp_score_div_exact"]
    assert len(sig) == len(params) == 10
    # gp_score_div without the probe: same order otherwise
    m2 = re.search(r"\bint\s+gp_score_div\s*\(([^)]*)\)\s*;", hdr)
    probe_less = [a.strip() for a in m2.group(1).split(",") if not a.strip().endswith("*eps")]
    assert params == probe_less
    assert sig == [t for i, t in enumerate(_lib.SIGNATURES["gp_score_div"]) if i != 6]
    assert hasattr(_lib.lib(), "gp_score_div_exact")
    # null pointers are refused before anything touches a device
    assert _lib.lib().gp_score_div_exact(1, 1, None, None, None, None, None, None, None, None) == -1


def test_driver_model_value():
    from genpose_amd import _lib
    from genpose_amd.samplers import ODESampler
    assert int(re.search(r"#define GP_RK45_MODEL_LIKELIHOOD_EXACT (\d+)", _header()).group(1)) == _lib.RK45_MODEL_LIKELIHOOD_EXACT == 4
    assert ODESampler.MODELS == {"score": 0, "energy": 1, "likelihood": 2, "likelihood_exact": 4}
    L = _lib.lib()
    assert L.gp_rk45_plan_rows(4, 1, 640, 50) == 16 and L.gp_rk45_plan_rows_unshared(4, 1, 640, 50) == 16  # 32 000 rows: still tiles, no chain form
    assert L.gp_rk45_plan_rows(4, 2, 3, 5) == -1 and L.gp_rk45_plan_rows(4, 2, 16, 5) == 16                  # several batches: whole tiles per batch
    assert L.gp_rk45_partials_count(4, 0, 1, 2, 50) == 3 * 7
    assert L.gp_rk45_plan_rows(3, 1, 64, 50) < 0 and L.gp_rk45_plan_rows(5, 1, 64, 50) < 0


def test_argument_errors():
    from genpose_amd.config import get_config
    from genpose_amd.likelihood import cond_ode_likelihood, solver_model
    from genpose_amd.posenet import GFObjectPose
    assert get_config().likelihood_divergence == "hutchinson"
    assert solver_model("hutchinson") == "likelihood" and solver_model("exact") == "likelihood_exact"
    cvec, x = torch.zeros(1, 768), torch.zeros(2, 9)
    with pytest.raises(ValueError, match="no probe"):
        cond_ode_likelihood(None, cvec, 2, x, torch.zeros(2, 9), divergence="exact")
    with pytest.raises(ValueError, match="needs the probe"):
        cond_ode_likelihood(None, cvec, 2, x, None)
    with pytest.raises(NotImplementedError, match="'russian-roulette'"):
        cond_ode_likelihood(None, cvec, 2, x, None, divergence="russian-roulette")
    net = GFObjectPose(get_config(posenet_mode="score"), None, None, None, 1e-5, 1.0)
    with pytest.raises(NotImplementedError, match="'hutchinson2'"):
        net.calc_likelihood({}, divergence="hutchinson2")
    enet = GFObjectPose(get_config(posenet_mode="energy"), None, None, None, 1e-5, 1.0)
    enet.pose_score_net = object()  # (weights present: the refusal is about the model, not about loading)
    for div in ("hutchinson", "exact"):
        with pytest.raises(NotImplementedError, match="likelihoods come from the score model"):
            enet.calc_likelihood({}, divergence=div)


def test_closed_form_trace_is_the_autograd_trace():
    """the closed form the float64 solve evaluates == torch.autograd.functional.jacobian on the oracle's network"""
    for seed, (B, K), t in [(0, (3, 5), 1e-5), (1, (1, 17), 0.3), (0, (1, 1), 1.0)]:
        sd64 = er.f64(go.make_state_dict(seed, "score"))
        gen = torch.Generator().manual_seed(9 + seed)
        pfr = torch.randn(B, 1024, generator=gen).abs().repeat_interleave(K, 0)
        x = er.unit_axis_poses(B * K, t, gen)
        s, tr, J = er.trace_autograd(sd64, pfr, x, t)
        s2, tr2 = er.score_and_trace(sd64, pfr, x, t)
        assert float((tr - tr2).abs().max()) <= 1e-12 * float(tr.abs().max())
        assert float((s - s2).abs().max()) <= 1e-12 * float(s.abs().max())
        # nine unit seeds: seed i reaches head i // 3 only - the off-head blocks of J are not zero, the trace needs the diagonal alone
        assert np.allclose(torch.diagonal(J, dim1=1, dim2=2).sum(-1).numpy(), tr.numpy())


def test_kink_share_of_the_gpu_cases():
    """the inputs tests/test_gpu_exact_likelihood.py draws (same generator seeds): rows whose float64 trace moves by more than 1e-3
    relative under a 1e-6 relative move of x stay under 5 % per shape"""
    for seed in (0, 1):
        sd64 = er.f64(go.make_state_dict(seed, "score"))
        for B, K in [(1, 1), (1, 17), (3, 5), (2, 50)]:
            for t in (1e-5, 0.3, 1.0):
                gen = torch.Generator().manual_seed(100 * seed + 7 * B + K)
                pfr = torch.randn(B, 1024, generator=gen).abs().repeat_interleave(K, 0)
                x = er.unit_axis_poses(B * K, t, gen)
                _, tr = er.score_and_trace(sd64, pfr, x, t)
                _, trm = er.score_and_trace(sd64, pfr, x.double() * (1 + 1e-6), t)
                share = float(((trm - tr).abs() > 1e-3 * tr.abs()).double().mean())
                assert share <= 0.05, (seed, B, K, t, share)
