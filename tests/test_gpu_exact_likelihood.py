"""GPU: the exact-divergence likelihood - gp_score_div_exact (score + tr(d score / d x), csrc/score_bwd.h: score_div_exact_tile), the RK45
driver's model 'likelihood_exact', cond_ode_likelihood / calc_likelihood(divergence='exact'), PoseNet.get_likelihood.

Ground truth is float64 and built here (tests/exact_likelihood_ref.py): torch.autograd.functional.jacobian on the oracle's score network
per row and its trace; for the solve, scipy's RK45 restated in tests/rk45_reference.py on the same float64 field.  The kernel's yardstick
is the EXISTING kernel: gp_score_div's error against the float64 e^T J e on the same rows."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_likelihood_ref as er
from oracle import genpose_oracle as go

SHAPES = [(1, 1), (1, 17), (3, 5), (2, 50)]  # single row; partial last tile; tiles that span clouds; more than one full tile
TIMES = (1e-5, 0.3, 1.0)
KINK_SHARE = 0.05      # rows dropped because a ReLU kink sits within 1e-6 relative of x: at most this share per shape
YARDSTICK_FACTOR = 3   # exact kernel's error <= 3 x gp_score_div's on the same rows (it sums nine such terms)
# the band the Hutchinson path is granted against its golden, restated from tests/test_gpu_sampler.py::test_likelihood_golden (fixture G12)
LIKELIHOOD_RTOL = 2e-3
NFEV_MARGIN = 0.05
HERE = os.path.dirname(os.path.abspath(__file__))
CKPT_SCORE = os.path.join(HERE, "golden", "trained", "ckpt_score.pth")

_cache = {}


def _net(seed):
    from genpose_amd.scorenet import ScoreNetHIP
    if ("net", seed) not in _cache:
        _cache["net", seed] = ScoreNetHIP(go.make_state_dict(seed, "score"), "cuda")
    return _cache["net", seed]


def _case(seed, B, K, t):
    """inputs, float64 truth and both kernels' outputs of one (weights seed, shape, time): computed once, read by several tests"""
    key = ("case", seed, B, K, t)
    if key in _cache:
        return _cache[key]
    sd64 = er.f64(go.make_state_dict(seed, "score"))
    gen = torch.Generator().manual_seed(100 * seed + 7 * B + K)
    pf = torch.randn(B, 1024, generator=gen).abs()
    x = er.unit_axis_poses(B * K, t, gen)
    probe = torch.randn(B * K, 9, generator=gen)
    pfr = pf.repeat_interleave(K, 0)
    score, tr, J = er.trace_autograd(sd64, pfr, x, t)
    _, tr_moved = er.score_and_trace(sd64, pfr, x.double() * (1 + 1e-6), t)
    stable = ((tr_moved - tr).abs() <= 1e-3 * tr.abs()).numpy()
    eJe = torch.einsum("ri,rij,rj->r", probe.double(), J, probe.double())
    net = _net(seed)
    cvec = net.cloud_embed(pf.cuda())
    tvec = net.time_embed(torch.tensor([t], device="cuda"))
    sigma = torch.tensor([0.01 * 5000.0 ** t], device="cuda")
    s_x, d_x = net.score_and_exact_divergence(cvec, K, x.cuda(), tvec[0], sigma)
    s_h, d_h = net.score_and_divergence(cvec, K, x.cuda(), probe.cuda(), tvec[0], sigma)
    c = dict(pf=pf, x=x, probe=probe, cvec=cvec, tvec=tvec, sigma=sigma, score=score.numpy(), tr=tr.numpy(), eJe=eJe.numpy(), stable=stable,
             s_x=s_x.cpu().numpy(), d_x=d_x.double().cpu().numpy(), s_h=s_h.cpu().numpy(), d_h=d_h.double().cpu().numpy())
    _cache[key] = c
    return c


@pytest.mark.parametrize("seed", [0, 1])
def test_div_exact_matches_f64_trace(seed):
    """div of gp_score_div_exact against the float64 autograd trace, on rows whose trace is stable under a 1e-6 relative move of x.
    Tolerance: YARDSTICK_FACTOR x the error gp_score_div makes against the float64 e^T J e on the same rows, both relative to max|div|,
    the largest float64 divergence of the case.  Measured on MI355X, weights seed 1, shape (1,1), t = 1e-5 / 0.3 / 1: exact 3.7e-7 / 1.2e-6 /
    2.8e-6, one-probe 8.7e-7 / 6.2e-6 / 7.8e-6 (at t = 1 the nine diagonal terms cancel to a trace of 4.3e-4); over all 24 cases the
    ratio exact / one-probe lies between 0.10 and 0.89.  Both errors are printed per case (pytest -s); profiles/exact_likelihood.txt keeps
    all 24 lines of a run."""
    for B, K in SHAPES:
        dropped = []
        for t in TIMES:
            c = _case(seed, B, K, t)
            keep = c["stable"]
            dropped.append(1.0 - keep.mean())
            # ONE normaliser for both errors, the largest float64 divergence of the case: the yardstick compares what the two kernels
            # lose in absolute terms on the same rows (a quotient by each kernel's own reference would instead compare how much the nine
            # diagonal terms cancel in the trace with how much the 81 terms cancel in e^T J e - a property of the row, not of a kernel)
            scale = np.abs(c["tr"][keep]).max()
            err_h = np.abs(c["d_h"] - c["eJe"])[keep].max() / scale
            err_x = np.abs(c["d_x"] - c["tr"])[keep].max() / scale
            print(f"seed {seed} shape ({B},{K}) t {t:g}: rows kept {int(keep.sum())}/{keep.size}  exact err {err_x:.3e}  one-probe err {err_h:.3e}  "
                  f"ratio {err_x / err_h:.2f}  max|tr| {scale:.4g}  max|eJe| {np.abs(c['eJe'][keep]).max():.4g}")
            assert np.isfinite(c["d_x"]).all()
            assert err_x <= YARDSTICK_FACTOR * err_h, (seed, B, K, t, err_x, err_h)
            # and the score itself is the float64 score at the existing kernels' tolerance (tests/test_gpu_score.py NET_RTOL)
            np.testing.assert_allclose(c["s_x"], c["score"], rtol=2e-4, atol=2e-4 * np.abs(c["score"]).max())
        assert max(dropped) <= KINK_SHARE, (seed, B, K, dropped)


@pytest.mark.parametrize("seed", [0, 1])
def test_score_output_is_gp_score_divs(seed):
    """same forward code: score bit-identical to gp_score_div's at every shape and time of the test above"""
    for B, K in SHAPES:
        for t in TIMES:
            c = _case(seed, B, K, t)
            assert np.array_equal(c["s_x"].view(np.uint32), c["s_h"].view(np.uint32)), (seed, B, K, t)


def test_exact_equals_mean_of_probes():
    """E[e^T J e] = tr J over Gaussian probes: the mean of gp_score_div over 4096 probes lies within 5 standard errors of the exact
    value, row by row - a wrong seed-to-head mapping fails here independently of autograd."""
    B, K, t, NP = 2, 50, 0.3, 4096
    c = _case(0, B, K, t)
    net = _net(0)
    gen = torch.Generator(device="cuda").manual_seed(2024)
    probes = torch.randn(NP * B * K, 9, device="cuda", generator=gen)
    # NP copies of the two clouds back to back: one launch of NP * 100 rows
    _, d = net.score_and_divergence(c["cvec"].repeat(NP, 1).contiguous(), K, c["x"].cuda().repeat(NP, 1).contiguous(), probes, c["tvec"][0], c["sigma"])
    d = d.double().reshape(NP, B * K).cpu().numpy()
    mean, se = d.mean(0), d.std(0, ddof=1) / np.sqrt(NP)
    dev = np.abs(mean - c["d_x"]) / se
    print(f"mean of {NP} probes vs exact: worst deviation {dev.max():.2f} standard errors (standard error / |exact| median {np.median(se / np.abs(c['d_x'])):.3f})")
    assert (dev <= 5.0).all(), dev.max()


def test_sentinels_and_refusals():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    B, K = 2, 50
    c = _case(0, B, K, 0.3)
    net, R, TAIL = _net(0), B * K, 64
    x = c["x"].cuda()
    fn = _lib.lib().gp_score_div_exact

    def outs():
        return torch.full((R * 9 + TAIL,), -7.0, device="cuda"), torch.full((R + TAIL,), -7.0, device="cuda")

    score, div = outs()
    assert fn(B, K, net.w.ref(), ptr(c["cvec"]), ptr(c["tvec"]), ptr(x), ptr(c["sigma"]), ptr(score), ptr(div), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((score[R * 9:] == -7).all()) and bool((div[R:] == -7).all())
    assert np.array_equal(score[: R * 9].reshape(R, 9).cpu().numpy(), c["s_x"]) and np.array_equal(div[:R].double().cpu().numpy(), c["d_x"])
    # refusals: GP_EINVAL, nothing written
    good = [B, K, net.w.ref(), ptr(c["cvec"]), ptr(c["tvec"]), ptr(x), ptr(c["sigma"]), None, None, stream_ptr()]
    score, div = outs()
    good[7], good[8] = ptr(score), ptr(div)
    for i in (2, 3, 4, 5, 6, 7, 8):
        bad = list(good)
        bad[i] = None
        assert fn(*bad) == -1, i
    bad = list(good)
    bad[1] = 0
    assert fn(*bad) == -1
    stripped = _lib.GpScoreNet(**{n: (None if n in ("w_headx_t", "w_pose2_t", "w_pose0_t") else getattr(net.w.struct, n)) for n, _ in _lib.GpScoreNet._fields_})
    bad = list(good)
    bad[2] = ctypes.byref(stripped)
    assert fn(*bad) == -1
    bad = list(good)
    bad[0] = 0  # no rows: GP_OK, nothing to write
    assert fn(*bad) == 0
    torch.cuda.synchronize()
    assert bool((score == -7).all()) and bool((div == -7).all())
    # the driver: no probe for the exact model, no chain plan, and 3 stays an unknown model
    from genpose_amd.samplers import ODESampler
    assert _lib.lib().gp_rk45_plan_rows(_lib.RK45_MODEL_LIKELIHOOD_EXACT, 1, 640, 50) == 16
    smp = ODESampler(net, B, K, "cuda", model="likelihood_exact")
    assert smp.tile == 16 and smp.probe is None and smp.ncomp == 10
    with pytest.raises(ValueError):
        smp.run_likelihood(c["cvec"], x, c["probe"].cuda())
    with pytest.raises(ValueError):
        ODESampler(net, B, K, "cuda", model="likelihood_exact", tile=128)


def test_exact_likelihood_solve():
    """2 clouds x 3 poses at rtol = atol = 1e-5 against the float64 solve of the same ODE (float64 network, float64 exact trace, scipy's
    RK45 as tests/rk45_reference.py restates it): log-likelihood in bits and z inside the band of the Hutchinson path's golden test,
    evaluation count inside its margin."""
    from genpose_amd.likelihood import cond_ode_likelihood
    B, K = 2, 3
    sd = go.make_state_dict(0, "score")
    gen = torch.Generator().manual_seed(5)
    pf = torch.randn(B, 1024, generator=gen).abs()
    x = er.unit_axis_poses(B * K, 1e-5, gen)
    z_ref, bits_ref, att_ref = er.solve_f64(sd, pf.repeat_interleave(K, 0), x)
    net = _net(0)
    st = {}
    z, bits = cond_ode_likelihood(net, net.cloud_embed(pf.cuda()), K, x.cuda(), None, rtol=1e-5, atol=1e-5, stats=st, divergence="exact")
    z, bits = z.cpu().numpy(), bits.cpu().numpy()
    nfev_ref = 2 + 6 * att_ref
    print(f"exact likelihood solve: bits {bits} vs float64 {bits_ref}; worst relative {np.abs(bits - bits_ref).max() / np.abs(bits_ref).max():.2e}; "
          f"z worst {np.abs(z - z_ref).max() / np.abs(z_ref).max():.2e}; attempts {st['attempts']} vs {att_ref}")
    assert bits.dtype == np.float64 and bits.shape == (B * K,)
    np.testing.assert_allclose(bits, bits_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(bits_ref).max())
    np.testing.assert_allclose(z, z_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(z_ref).max())
    assert abs(st["nfev"] - nfev_ref) <= NFEV_MARGIN * nfev_ref, (st["nfev"], nfev_ref)


def _agent(**cfg):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    a = PoseNet(get_config(posenet_mode="score", **cfg))
    a.load_state_dict(go.make_state_dict(0, "score"))
    return a


def test_deterministic_and_generator_untouched(golden):
    from genpose_amd.likelihood import cond_ode_likelihood
    g = golden("g12_likelihood.npz")
    agent = _agent()
    pts = torch.from_numpy(g["pts"]).cuda()
    data = {"pts": pts, "pts_center": pts.mean(dim=1)}
    data["pts_feat"] = agent.net(data, mode="pts_feature")
    data["sampled_pose"] = torch.from_numpy(g["pose"]).cuda()
    tol = dict(atol=1e-4, rtol=1e-4)
    # exact: no prior draw (prior_fn is not even called), the CPU generator stays where it was, equal bits on a second call
    saved = agent.net.prior_fn

    def no_prior(*a, **k):
        raise AssertionError("divergence='exact' drew from the prior")

    agent.net.prior_fn = no_prior
    torch.manual_seed(11)
    state = torch.get_rng_state()
    l1 = agent.net.calc_likelihood(data, divergence="exact", **tol)
    l2 = agent.net.calc_likelihood(data, divergence="exact", **tol)
    assert torch.equal(torch.get_rng_state(), state)
    assert l1.dtype == torch.float64 and l1.shape == (3,) and torch.equal(l1, l2) and bool(torch.isfinite(l1).all())
    agent.net.cfg.likelihood_divergence = "exact"
    assert torch.equal(agent.net(data, mode="likelihood"), agent.net.calc_likelihood(data, divergence="exact"))
    agent.net.cfg.likelihood_divergence = "hutchinson"
    agent.net.prior_fn = saved
    # hutchinson: still the estimator the old call computes from the same draw - and it does advance the generator
    torch.manual_seed(7)
    lh = agent.net.calc_likelihood(data, **tol)
    assert not torch.equal(torch.get_rng_state(), torch.manual_seed(7).get_state())
    torch.manual_seed(7)
    eps = agent.net.prior_fn((3, 9))
    psn = agent.net.pose_score_net
    _, lo = cond_ode_likelihood(psn, psn.cloud_embed(data["pts_feat"].float()), 1, data["sampled_pose"].float().contiguous(), eps.cuda(),
                                agent.net.sampling_eps, 1e-4, 1e-4)
    assert torch.equal(lh, lo)
    assert not torch.equal(lh, l1)
    with pytest.raises(NotImplementedError, match="trace-ish"):
        agent.net.calc_likelihood(data, divergence="trace-ish")


def test_get_likelihood_ranks():
    """PoseNet.get_likelihood on the trained score checkpoint: 4 held-out synthetic clouds x 8 PC-20 candidates -> [4,8] finite bits; fed
    as BOTH energy columns through the existing ranking it orders the candidates by descending likelihood.  (No accuracy claim: how a
    likelihood ranking compares with the energy model's is not measured.)"""
    from genpose_amd import reward, synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import make_batch_sample
    B, K = 4, 8
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=20))
    agent.load_ckpt(model_dir=CKPT_SCORE, model_path=True, load_model_only=True)
    pts = torch.from_numpy(synth.posed_batch(range(1_000_000, 1_000_000 + B))["pts"]).cuda()
    sample = make_batch_sample(pts)
    torch.manual_seed(3)
    pred = agent.pred_func(data=sample, repeat_num=K, save_path=None)
    ll = agent.get_likelihood(sample, pred, extract_pts_feature=False)
    assert ll.shape == (B, K) and ll.dtype == torch.float64 and bool(torch.isfinite(ll).all())
    ll32 = ll.float()
    assert all(len(set(row.tolist())) == K for row in ll32)  # distinct poses: no ties, also not after the cast to the energy dtype
    energy = torch.stack([ll32, ll32], dim=-1).contiguous()
    r = reward.rank_aggregate(pred, energy, ratio=0.6)
    want = torch.argsort(-ll32, dim=1)
    assert torch.equal(r["order"][:, :, 0].long(), want) and torch.equal(r["order"][:, :, 1].long(), want)
    sp, se = reward.sort_poses_by_energy(pred, energy)
    bi = torch.arange(B, device=pred.device).unsqueeze(1)
    assert torch.equal(sp, pred[bi, want]) and torch.equal(se[:, :, 0], ll32[bi, want])
    print("log-likelihood (bits) of the candidates of cloud 0:", ll[0].cpu().numpy(), "attempts", agent.net.last_likelihood_stats["attempts"])
