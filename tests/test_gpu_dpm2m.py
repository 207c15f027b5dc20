"""GPU: the fixed-step DPM-Solver++(2M) solver of the probability-flow ODE (genpose_amd.samplers.Dpm2mSampler; dpm2m_step_kernel<16|32|64>,
dpm2m_step_chain_kernel<2>, dpm2m_step_chain_kernel_bf16x9, dpm2m_solve_kernel<16|32|64>) against its float64 restatement
(tests/dpm2m_reference.py) driving the oracle's score network in float64, seeded synthetic weights, on the shapes, N and inputs of
tests/test_gpu_heun.py.

Tolerance: rtol = atol = 1e-3, the Heun tests' bound (the project's own for its fixed-step samplers); it is not derived from what the
kernels give.  Measured on MI355X, max |device - fp64| / (1e-3 + 1e-3 |fp64|) per plan (profiles/dpm2m_sampler.txt): 1.4e-3 - 3.5e-3 at
T0 = 0.55 (a margin of 280 x or more), 0.059 - 0.48 at T0 = 1 (2.1 x on the bf16x9 chain form with the edm grid, 6.1 - 17 x on the other plans):
as for the Heun solver the random-weight flow from T0 = 1 amplifies fp32 rounding of the score.  The bound remains as a COARSE check (wp
scaled by 1 + 1e-4 passes it at T0 = 0.55); the solver's accuracy claim is carried by tests/test_gpu_solver_f64.py, which holds it to float64
at 3x the fp32 restatement's own error.

Then what the Heun solver's tests hold it to: row locality, replay at another T0 without recapture, the one-launch form equal to the chain
bit for bit, the agent's pred_func and one FixedStepTracker frame equal to their pieces."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

import dpm2m_reference as dr
import heun_reference as hr
import test_gpu_heun as th

RTOL = ATOL = 1e-3
N_STEPS = 6
PLANS = th.PLANS  # tile16: 3 x 5 = 15 rows; tile32 / tile64: 3 x 23 = 69 rows; chain_f32 / chain_bf16x9: 3 x 50 = 150 rows
TILE_PLANS = ("tile16", "tile32", "tile64")
KERNELS = {"tile16": "dpm2m_step_kernel<16>", "tile32": "dpm2m_step_kernel<32>", "tile64": "dpm2m_step_kernel<64>",
           "chain_f32": "dpm2m_step_chain_kernel<2>", "chain_bf16x9": "dpm2m_step_chain_kernel<bf16x9>"}
_net, _inputs = th._net, th._inputs


@functools.lru_cache(maxsize=None)
def _reference(B, K, T0, grid):
    """float64: the states x_1 .. x_N, x_N and the denoised x_N, all finished; the network sees the times the device sees (float32)."""
    feat, centre, x0 = _inputs(B, K, T0)
    sd64 = {k: v.double() for k, v in go.make_state_dict(0, "score").items()}
    feat_r = feat.repeat_interleave(K, 0).double()

    def score(x, t):
        tt = torch.full((B * K, 1), t, dtype=torch.float64)
        return go.score_forward(sd64, feat_r, torch.from_numpy(np.ascontiguousarray(x)), tt).numpy()

    xs = dr.dpm2m_solve(score, x0.double().numpy(), N_STEPS, T0=T0, kind=grid, t32=True)
    den = hr.denoise(score, xs[-1], N_STEPS, t32=True)
    cen_r = centre.repeat_interleave(K, 0).double().numpy()
    return hr.finish(xs[1:], cen_r), hr.finish(xs[-1], cen_r), hr.finish(den, cen_r)


def _sampler(plan, n=N_STEPS, launches="chain", **kw):
    from genpose_amd.samplers import Dpm2mSampler
    B, K, tile, trunk = PLANS[plan]
    smp = Dpm2mSampler(_net(), B, K, n, "cuda", tile=tile, trunk=trunk, launches=launches, **kw)
    want = KERNELS[plan] if launches == "chain" else f"dpm2m_solve_kernel<{tile}>"
    assert smp.kernel_name == want and smp.tile == tile and smp.launches == launches
    return smp


def _run(smp, feat, centre, x0, **kw):
    cvec = _net().cloud_embed(feat.cuda())
    xs, pose = smp.run(cvec, centre.cuda(), x0.cuda(), **kw)
    torch.cuda.synchronize()
    return (None if xs is None else xs.clone()), pose.clone(), smp.x.clone()


worst = {"ratio": 0.0}


def _assert_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ratio = float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"{what}: max |device - fp64| / (atol + rtol |fp64|) = {ratio:.3e} (worst so far {worst['ratio']:.3e})")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)


def _assert_same(a, b, what):
    for u, v, part in zip(a, b, ("trajectory", "pose", "x")):
        assert (u is None) == (v is None), (what, part)
        if u is not None:
            assert torch.isfinite(u).all(), (what, part)
            assert torch.equal(u, v), f"{what} {part}: {int((u != v).sum())} of {u.numel()} words differ, max |diff| {float((u - v).abs().max()):.3e}"


@pytest.mark.parametrize("grid", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("plan", list(PLANS))
def test_every_plan_against_the_restatement(plan, denoise, T0, grid):
    B, K = PLANS[plan][:2]
    traj_ref, last_ref, den_ref = _reference(B, K, T0, grid)
    smp = _sampler(plan, grid=grid, denoise=denoise, record_traj=True)
    xs, pose, _ = _run(smp, *_inputs(B, K, T0), T0=T0)
    st = smp.last_stats
    assert st["nfev"] == N_STEPS + (1 if denoise else 0) and st["nlaunch"] == st["nfev"] + 1 and st["kernel_name"] == KERNELS[plan]
    assert pose.dtype == torch.float32 and xs.dtype == torch.float32 and tuple(xs.shape) == (B * K, N_STEPS, 9)
    what = f"{plan} denoise={denoise} T0={T0} {grid}"
    _assert_close(xs.permute(1, 0, 2).cpu().numpy(), traj_ref, what + " trajectory")
    _assert_close(pose.cpu().numpy(), den_ref if denoise else last_ref, what + " pose")


@pytest.mark.parametrize("plan,Bg,K,tile", [("tile16", 2, 24, 16), ("chain_bf16x9", 2, 64, 128)])
def test_row_locality_bit_for_bit(plan, Bg, K, tile):
    """A batch run alone equals the same batch as group 1 of a groups=2 launch under the same pinned tile."""
    from genpose_amd.samplers import Dpm2mSampler
    net = _net()
    fa, ca, xa = _inputs(Bg, K, 1.0, seed=21)
    fb, cb, xb = _inputs(Bg, K, 1.0, seed=22)
    alone = Dpm2mSampler(net, Bg, K, 4, "cuda", tile=tile, record_traj=True)
    both = Dpm2mSampler(net, 2 * Bg, K, 4, "cuda", groups=2, tile=tile, record_traj=True)
    assert alone.kernel_name == both.kernel_name == KERNELS[plan]
    xs1, p1, _ = _run(alone, fb, cb, xb)
    xs2, p2, _ = _run(both, torch.cat([fa, fb]), torch.cat([ca, cb]), torch.cat([xa, xb]))
    R = Bg * K
    assert torch.equal(p2[R:], p1) and torch.equal(xs2[R:], xs1)
    assert not torch.equal(p2[:R], p1)


@pytest.mark.parametrize("plan", ["tile32", "chain_bf16x9"])
def test_replay_follows_run_time_T0_without_a_second_capture(plan):
    B, K = PLANS[plan][:2]
    fa, ca, xa = _inputs(B, K, 1.0, seed=31)
    fb, cb, xb = _inputs(B, K, 0.55, seed=32)
    smp = _sampler(plan, record_traj=True)
    _run(smp, fa, ca, xa, T0=1.0)
    second = _run(smp, fb, cb, xb, T0=0.55)
    assert smp.captures == 1
    _assert_same(second, _run(_sampler(plan, record_traj=True), fb, cb, xb, T0=0.55), f"{plan} replay against a fresh sampler")
    _assert_same(_run(smp, fb, cb, xb, T0=0.55), second, f"{plan} second replay")
    assert smp.captures == 1
    assert not torch.equal(second[1], _run(smp, fb, cb, xb, T0=0.5)[1]) and smp.captures == 1  # (T0 does reach the kernels)


@pytest.mark.parametrize("record_traj", [True, False])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("n", [1, 6])
@pytest.mark.parametrize("plan", TILE_PLANS)
def test_one_launch_equals_the_chain_bit_for_bit(plan, n, denoise, record_traj):
    """The pose, the state and every trajectory state; then the same two captured graphs replayed at another T0."""
    B, K = PLANS[plan][:2]
    chain = _sampler(plan, n, denoise=denoise, record_traj=record_traj)
    single = _sampler(plan, n, "single", denoise=denoise, record_traj=record_traj)
    what = f"{plan} N={n} denoise={denoise}"
    a = _inputs(B, K, 0.55)
    ref, got = _run(chain, *a, T0=0.55), _run(single, *a, T0=0.55)
    _assert_same(got, ref, what)
    assert (got[0] is not None) == record_traj and not torch.equal(got[2], a[2].cuda())  # (the solve did move the rows)
    st = single.last_stats
    assert st["device_launches"] == 1 and st["kernel_name"] == f"dpm2m_solve_kernel<{PLANS[plan][2]}>"
    assert st["nlaunch"] == chain.last_stats["nlaunch"] == n + 1 + int(denoise) and st["nfev"] == chain.last_stats["nfev"] == n + int(denoise)
    b = _inputs(B, K, 0.15, seed=12)
    _assert_same(_run(single, *b, T0=0.15), _run(chain, *b, T0=0.15), what + " replayed at T0 = 0.15")
    assert single.captures == 1 and chain.captures == 1


def test_the_chain_form_has_no_one_launch_solve():
    from genpose_amd.samplers import Dpm2mSampler
    with pytest.raises(ValueError, match="128"):
        Dpm2mSampler(_net(), 3, 50, 4, "cuda", tile=128, launches="single")
    with pytest.raises(ValueError, match="launches"):
        Dpm2mSampler(_net(), 3, 5, 4, "cuda", launches="graph")
    assert Dpm2mSampler(_net(), 3, 5, 4, "cuda").launches == "chain"


def test_the_first_launch_does_not_read_the_previous_denoiser():
    """`d` holds no D_{-1} at the first step: poisoned with NaN before the run, the result is finite and the same."""
    B, K = PLANS["tile16"][:2]
    a = _inputs(B, K, 0.55)
    smp = _sampler("tile16", use_graph=False)
    ref = _run(smp, *a, T0=0.55)
    smp.d.fill_(float("nan"))
    _assert_same(_run(smp, *a, T0=0.55), ref, "d poisoned")


@pytest.mark.parametrize("warm", [False, True])
def test_agent_pred_func_is_the_sampler_on_the_same_draw(warm):
    from genpose_amd import synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.samplers import Dpm2mSampler
    from test_gpu_sampler import FixedPrior
    B, K = 3, 10
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["dpm2m"], sampling_steps=N_STEPS))
    agent.load_state_dict(go.make_state_dict(0, "score"))
    pts = torch.from_numpy(synth.make_batch(B, start=40)).cuda()
    data = {"pts": pts, "pts_center": pts.mean(dim=1)}
    noise = torch.randn(B * K, 9, generator=torch.Generator().manual_seed(5))
    T0 = 0.15 if warm else None
    init_x = torch.randn(B, 9, generator=torch.Generator().manual_seed(6)).cuda() if warm else None
    with FixedPrior(agent, noise.numpy()):
        pred = agent.pred_func(data, repeat_num=K, save_path=None, init_x=init_x, T0=T0)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (B, K, 9)
    st = agent.net.last_sampler.last_stats
    assert isinstance(agent.net.last_sampler, Dpm2mSampler) and st["nfev"] == N_STEPS + 1 and st["nlaunch"] == N_STEPS + 2
    T = 1.0 if T0 is None else T0
    draw = (noise * (0.01 * (50.0 / 0.01) ** T)).cuda()
    x0 = draw if not warm else init_x.unsqueeze(1).repeat(1, K, 1).view(B * K, 9).float() + draw  # samplers.py:180
    net = agent.net.pose_score_net
    smp = Dpm2mSampler(net, B, K, N_STEPS, "cuda")
    _, pose = smp.run(net.cloud_embed(data["pts_feat"].float()), data["pts_center"].float(), x0, T0=T, eps=agent.net.sampling_eps)
    assert torch.equal(pred.reshape(B * K, 9), pose)
    if not warm:
        with FixedPrior(agent, noise.numpy()):
            xs, res = agent.net({"pts_feat": data["pts_feat"], "pts_center": data["pts_center"], "_repeat": K}, mode="dpm2m_sample")
        assert torch.equal(res, pose) and tuple(xs.shape) == (B * K, N_STEPS, 9)


@pytest.mark.parametrize("launches", ["single", "chain"])
def test_a_tracker_frame_equals_its_pieces_called_one_after_the_other(launches):
    """FixedStepTracker(solver='dpm2m'), one frame of 2 objects x 10 candidates: the host warm-start formula on the dumped draws,
    Dpm2mSampler as a chain, get_energy and rank_aggregate - bit for bit."""
    import test_gpu_fixed_step_tracker as tt
    from genpose_amd import reward
    from genpose_amd.runner import FixedStepTracker, add_noise_to_RT, make_batch_sample
    from genpose_amd.samplers import Dpm2mSampler, dpm2m_schedule, track_prior_fill
    K, STEPS, T0, SEED = tt.K, tt.STEPS, tt.T0, tt.TSEED
    sa, ea = tt._agents()
    pts, names, gt = tt._sequence(0)[0]
    n = pts.shape[0]
    assert (n, K) == (2, 10)
    tr = FixedStepTracker(sa, ea, steps=STEPS, repeat_num=K, T0=T0, seed=SEED, launches=launches, solver="dpm2m")
    got = tr.step([(pts, names, gt)])[0]
    st = tr.last_stats
    assert st["replays"] <= 3 and st["nfev"] == STEPS + 1 and st["launches"] == launches
    assert st["kernel"] == ("dpm2m_solve_kernel<16>" if launches == "single" else "dpm2m_step_kernel<16>")
    # the pieces
    net = sa.net
    sample = make_batch_sample(pts)
    sample["pts_feat"] = net.extract_pts_feature(sample)
    centre = sample["pts_center"]
    g = torch.Generator().manual_seed((SEED * 1000003) % (1 << 63))
    draws = [torch.randn(n, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)]
    fallback = add_noise_to_RT(gt.float(), draws=draws)
    src = torch.full((n,), -1, dtype=torch.int32)
    sigma = torch.tensor([dpm2m_schedule(STEPS, T0, net.sampling_eps, "geometric")[1][0, 0]])
    z = track_prior_fill(SEED, 0, n * K, "cuda", row_base=0)
    x0 = tt._host_warm_start(torch.zeros(1, 4, 4), src, fallback, centre.cpu(), sigma, z.cpu(), K)
    init_x = torch.cat([fallback[:, :3, 0], fallback[:, :3, 1], fallback[:, :3, 3] - centre.cpu()], dim=1).cuda()
    smp = Dpm2mSampler(net.pose_score_net, n, K, STEPS, "cuda")
    _, pose = smp.run(net.pose_score_net.cloud_embed(sample["pts_feat"].float()), centre.float(), x0.cuda(), T0=T0, eps=net.sampling_eps)
    pred = pose.clone().view(n, K, 9)
    energy = ea.get_energy(data=sample, pose_samples=pred, T=1e-5)
    r = reward.rank_aggregate(pred, energy, selected_num=max(1, int(tr.ratio * K)), with_rt=True)
    want = {"init_x": init_x, "pred_pose": pred, "energy": energy, "sorted_RTs": r["sorted_RTs"], "average_sRT": r["avg_RT"], "nfev": STEPS + 1}
    tt._same(got, want, f"solver='dpm2m' {launches}")
    # and it is another solve than the default's
    heun = FixedStepTracker(sa, ea, steps=STEPS, repeat_num=K, T0=T0, seed=SEED, launches=launches).step([(pts, names, gt)])[0]
    assert torch.equal(heun["init_x"], got["init_x"]) and not torch.equal(heun["pred_pose"], got["pred_pose"])
