"""GPU: the fixed-step Heun solver of the probability-flow ODE (genpose_amd.samplers.HeunSampler; heun_step_kernel<16|32|64>,
heun_step_chain_kernel<2>, heun_step_chain_kernel_bf16x9) against its float64 restatement (tests/heun_reference.py) driving the oracle's
score network in float64, seeded synthetic weights.

Tolerance: rtol = atol = 1e-3, the project's own for its other fixed-step sampler (test_gpu_sampler.py: test_pc_agent_golden).  The runs
here do at most 13 evaluations against PC-20's 21 and draw no noise.  Measured on MI355X, max |device - fp64| / (1e-3 + 1e-3 |fp64|) per plan
(profiles/heun_sampler.txt): 1.1e-3 - 3.3e-3 at T0 = 0.55 (a margin of 300 x or more), 0.17 - 0.45 at T0 = 1 (2.2 x on the fp32 chain form, 3.2 - 5.8 x
on the others: NOT the 10 x asked for - the random-weight flow from T0 = 1 amplifies fp32 rounding of the score).  The tolerance stays as
stated; it is not derived from these figures.  It remains as a COARSE check (a corrector weight of 0.50005 passes it at T0 = 0.55); the
solver's accuracy claim is carried by tests/test_gpu_solver_f64.py, which holds it to float64 at 3x the fp32 restatement's own error.

Convergence against the device RK45 solve is checked at T0 = 0.55: with random weights the T0 = 1 flow is chaotic (test_gpu_sampler.py
lets exactly those golden cases drift), so two solvers of different order do not approach one trajectory there at these N."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

import heun_reference as hr

RTOL = ATOL = 1e-3
N_STEPS = 6
# plan -> (B, K, tile, trunk): 15 rows = one ragged 16-row tile; 69 rows = tails of 5 on 32- and 64-row tiles; 150 rows = two 128-row
# workgroups with a 22-row tail on both chain forms
PLANS = {
    "tile16": (3, 5, 16, None),
    "tile32": (3, 23, 32, None),
    "tile64": (3, 23, 64, None),
    "chain_f32": (3, 50, 128, "f32mfma"),
    "chain_bf16x9": (3, 50, 128, "bf16x9"),
}
KERNELS = {"tile16": "heun_step_kernel<16>", "tile32": "heun_step_kernel<32>", "tile64": "heun_step_kernel<64>",
           "chain_f32": "heun_step_chain_kernel<2>", "chain_bf16x9": "heun_step_chain_kernel<bf16x9>"}


@functools.lru_cache(maxsize=None)
def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    return ScoreNetHIP(go.make_state_dict(0, "score"), "cuda")


@functools.lru_cache(maxsize=None)
def _inputs(B, K, T0, seed=11):
    g = torch.Generator().manual_seed(seed + 1000 * B + K)
    feat = torch.randn(B, 1024, generator=g).abs()
    centre = torch.randn(B, 3, generator=g) * 0.3
    x0 = torch.randn(B * K, 9, generator=g) * float(hr.sigma(T0))
    return feat, centre, x0


@functools.lru_cache(maxsize=None)
def _reference(B, K, T0, grid):
    """float64: all states x_0 .. x_N and the denoised x_N, before normalisation; the network sees the times the device sees (float32)."""
    feat, centre, x0 = _inputs(B, K, T0)
    sd64 = {k: v.double() for k, v in go.make_state_dict(0, "score").items()}
    feat_r = feat.repeat_interleave(K, 0).double()

    def score(x, t):
        tt = torch.full((B * K, 1), t, dtype=torch.float64)
        return go.score_forward(sd64, feat_r, torch.from_numpy(np.ascontiguousarray(x)), tt).numpy()

    xs = hr.heun_solve(score, x0.double().numpy(), N_STEPS, T0=T0, kind=grid, t32=True)
    den = hr.denoise(score, xs[-1], N_STEPS, t32=True)
    cen_r = centre.repeat_interleave(K, 0).double().numpy()
    return hr.finish(xs[1:], cen_r), hr.finish(xs[-1], cen_r), hr.finish(den, cen_r)


def _sampler(plan, n=N_STEPS, **kw):
    from genpose_amd.samplers import HeunSampler
    B, K, tile, trunk = PLANS[plan]
    kw.setdefault("B", B)
    B = kw.pop("B")
    smp = HeunSampler(_net(), B, K, n, "cuda", tile=tile, trunk=trunk, **kw)
    assert smp.kernel_name == KERNELS[plan] and smp.tile == tile
    return smp


def _run(smp, feat, centre, x0, **kw):
    cvec = _net().cloud_embed(feat.cuda())
    xs, pose = smp.run(cvec, centre.cuda(), x0.cuda(), **kw)
    torch.cuda.synchronize()
    return (None if xs is None else xs.clone()), pose.clone()


worst = {"ratio": 0.0}


def _assert_close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ratio = float((np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))).max())
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"{what}: max |device - fp64| / (atol + rtol |fp64|) = {ratio:.3e} (worst so far {worst['ratio']:.3e})")
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=what)


@pytest.mark.parametrize("grid", ["geometric", "edm"])
@pytest.mark.parametrize("T0", [1.0, 0.55])
@pytest.mark.parametrize("denoise", [True, False])
@pytest.mark.parametrize("plan", list(PLANS))
def test_every_plan_against_the_restatement(plan, denoise, T0, grid):
    B, K = PLANS[plan][:2]
    traj_ref, last_ref, den_ref = _reference(B, K, T0, grid)
    smp = _sampler(plan, grid=grid, denoise=denoise, record_traj=True)
    xs, pose = _run(smp, *_inputs(B, K, T0), T0=T0)
    assert smp.last_stats["nfev"] == 2 * N_STEPS + (1 if denoise else 0) and smp.last_stats["launches"] == smp.last_stats["nfev"] + 1
    assert pose.dtype == torch.float32 and xs.dtype == torch.float32 and tuple(xs.shape) == (B * K, N_STEPS, 9)
    what = f"{plan} denoise={denoise} T0={T0} {grid}"
    _assert_close(xs.permute(1, 0, 2).cpu().numpy(), traj_ref, what + " trajectory")
    _assert_close(pose.cpu().numpy(), den_ref if denoise else last_ref, what + " pose")


@pytest.mark.parametrize("plan,Bg,K,tile", [("tile16", 2, 24, 16), ("chain_bf16x9", 2, 64, 128)])
def test_row_locality_bit_for_bit(plan, Bg, K, tile):
    """A batch run alone equals the same batch as group 1 of a groups=2 launch under the same pinned tile."""
    from genpose_amd.samplers import HeunSampler
    net = _net()
    fa, ca, xa = _inputs(Bg, K, 1.0, seed=21)
    fb, cb, xb = _inputs(Bg, K, 1.0, seed=22)
    alone = HeunSampler(net, Bg, K, 4, "cuda", tile=tile, record_traj=True)
    both = HeunSampler(net, 2 * Bg, K, 4, "cuda", groups=2, tile=tile, record_traj=True)
    assert alone.kernel_name == both.kernel_name == KERNELS[plan]
    xs1, p1 = _run(alone, fb, cb, xb)
    xs2, p2 = _run(both, torch.cat([fa, fb]), torch.cat([ca, cb]), torch.cat([xa, xb]))
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
    xs2, p2 = _run(smp, fb, cb, xb, T0=0.55)
    assert smp.captures == 1
    fresh = _sampler(plan, record_traj=True)
    xs3, p3 = _run(fresh, fb, cb, xb, T0=0.55)
    assert torch.equal(p2, p3) and torch.equal(xs2, xs3)
    xs4, p4 = _run(smp, fb, cb, xb, T0=0.55)
    assert torch.equal(p2, p4) and torch.equal(xs2, xs4) and smp.captures == 1
    assert not torch.equal(p2, _run(smp, fb, cb, xb, T0=0.5)[1]) and smp.captures == 1  # (T0 does reach the kernels)


def test_output_contract():
    B, K = PLANS["tile16"][:2]
    feat, centre, x0 = _inputs(B, K, 1.0)
    smp = _sampler("tile16", record_traj=True)
    xs, pose = _run(smp, feat, centre, x0)
    xs0, pose0 = _run(smp, feat, torch.zeros_like(centre), x0)
    cen_r = centre.repeat_interleave(K, 0).cuda()
    assert pose.dtype == torch.float32 and xs.dtype == torch.float32
    # translations include the centre, in the trajectory too; the rotation block does not move with it
    assert torch.allclose(pose[:, 6:] - pose0[:, 6:], cen_r, rtol=0, atol=1e-6 * float(pose0[:, 6:].abs().max() + 1))
    assert torch.allclose(xs[:, :, 6:] - xs0[:, :, 6:], cen_r.unsqueeze(1).expand(-1, N_STEPS, -1), rtol=0, atol=1e-6 * float(xs0[:, :, 6:].abs().max() + 1))
    assert torch.equal(pose[:, :6], pose0[:, :6]) and torch.equal(xs[:, :, :6], xs0[:, :, :6])
    for v in (pose, xs.reshape(-1, 9)):
        a, b = v[:, 0:3].double(), v[:, 3:6].double()
        assert float((a.norm(dim=1) - 1).abs().max()) < 1e-6 and float((b.norm(dim=1) - 1).abs().max()) < 1e-6
        assert float((a * b).sum(dim=1).abs().max()) < 1e-6


def _agent(steps=N_STEPS, **kw):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["heun"], sampling_steps=steps, **kw))
    agent.load_state_dict(go.make_state_dict(0, "score"))
    return agent


@pytest.mark.parametrize("warm", [False, True])
def test_agent_pred_func_is_the_sampler_on_the_same_draw(warm):
    from genpose_amd import synth
    from genpose_amd.samplers import HeunSampler
    from test_gpu_sampler import FixedPrior
    B, K = 3, 10
    agent = _agent()
    pts = torch.from_numpy(synth.make_batch(B, start=40)).cuda()
    data = {"pts": pts, "pts_center": pts.mean(dim=1)}
    noise = torch.randn(B * K, 9, generator=torch.Generator().manual_seed(5))
    T0 = 0.15 if warm else None
    init_x = None
    if warm:
        init_x = torch.randn(B, 9, generator=torch.Generator().manual_seed(6)).cuda()
    with FixedPrior(agent, noise.numpy()):
        pred = agent.pred_func(data, repeat_num=K, save_path=None, init_x=init_x, T0=T0)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (B, K, 9)
    assert agent.net.last_sampler.last_stats["nfev"] == 2 * N_STEPS + 1
    T = 1.0 if T0 is None else T0
    draw = (noise * (0.01 * (50.0 / 0.01) ** T)).cuda()
    x0 = draw if not warm else init_x.unsqueeze(1).repeat(1, K, 1).view(B * K, 9).float() + draw  # samplers.py:180
    net = agent.net.pose_score_net
    smp = HeunSampler(net, B, K, N_STEPS, "cuda")
    _, pose = smp.run(net.cloud_embed(data["pts_feat"].float()), data["pts_center"].float(), x0, T0=T, eps=agent.net.sampling_eps)
    assert torch.equal(pred.reshape(B * K, 9), pose)
    if not warm:
        with FixedPrior(agent, noise.numpy()):
            xs, res = agent.net({"pts_feat": data["pts_feat"], "pts_center": data["pts_center"], "_repeat": K}, mode="heun_sample")
        assert torch.equal(res, pose) and tuple(xs.shape) == (B * K, N_STEPS, 9)


def test_converges_to_the_device_rk45_solve():
    """Same x0, denoise off, N = 8, 16, 32 against ODESampler at rtol = atol = 1e-5: the distance decreases strictly with N (random weights:
    no ratio asserted)."""
    from genpose_amd.samplers import HeunSampler, ODESampler
    B, K, T0 = 3, 5, 0.55
    feat, centre, x0 = _inputs(B, K, T0)
    net = _net()
    cvec = net.cloud_embed(feat.cuda())
    _, ref = ODESampler(net, B, K, "cuda").run(cvec, centre.cuda(), x0.cuda(), T0, rtol=1e-5, atol=1e-5, denoise=False)
    dist = []
    for n in (8, 16, 32):
        _, pose = HeunSampler(net, B, K, n, "cuda", denoise=False).run(cvec, centre.cuda(), x0.cuda(), T0=T0)
        dist.append(float((pose.double() - ref).norm(dim=1).pow(2).mean().sqrt()))
    print(f"RMS pose distance to RK45 (rtol = atol = 1e-5), T0 = {T0}, N = 8 / 16 / 32: {dist[0]:.3e} / {dist[1]:.3e} / {dist[2]:.3e}")
    assert dist[0] > dist[1] > dist[2], dist


def test_refusals_and_einval_write_nothing():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.samplers import HeunSampler
    net = _net()
    with pytest.raises(NotImplementedError, match="head-split"):
        HeunSampler(net, 3, 5, 4, "cuda", tile=16 | _lib.PLAN_HEADSPLIT)
    with pytest.raises(ValueError):
        HeunSampler(net, 3, 5, 4, "cuda", trunk="bf16x3")
    with pytest.raises(ValueError):
        HeunSampler(net, 3, 5, 4, "cuda", grid="cosine")
    with pytest.raises(ValueError):
        HeunSampler(net, 3, 5, 0, "cuda")
    with pytest.raises(ValueError):
        HeunSampler(net, 3, 5, 4, "cuda", tile=128)  # k = 5: no chain form
    with pytest.raises(ValueError):
        HeunSampler(net, 3, 5, 4, "cuda", groups=2)
    B, K, n = 3, 50, 4
    R = B * K
    L = _lib.lib()
    poison = lambda *s: torch.full(s, -777.0, device="cuda")
    x, d, score, out, traj = poison(R, 9), poison(R, 9), poison(R, 9), poison(R, 9), poison(n, R, 9)
    cvec, tvec, sched, centre = torch.zeros(B, 768, device="cuda"), torch.zeros(n + 1, 768, device="cuda"), torch.zeros(2 * n + 2, 4, device="cuda"), torch.zeros(B, 3, device="cuda")
    x9 = [ptr(w) for w in net.w.bf16x9_packs()]
    good = dict(tile=16, ngroups=1, nb=B, k=K, launch=1, nsteps=n, denoise=1, net=net.w.ref(), cvec=ptr(cvec), tvec=ptr(tvec), sched=ptr(sched),
                centre=ptr(centre), x=ptr(x), d=ptr(d), score=ptr(score), out=ptr(out), traj=ptr(traj))
    bad = [dict(nsteps=0), dict(nsteps=-3), dict(launch=-1), dict(launch=2 * n + 2), dict(launch=2 * n + 1, denoise=0), dict(tile=16 | _lib.PLAN_HEADSPLIT),
           dict(tile=48), dict(tile=128, k=5, nb=30), dict(ngroups=0), dict(k=0), dict(ngroups=2, tile=128)]
    bad += [{name: None} for name in ("net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out")]
    for change in bad:
        a = dict(good, **change)
        args = [a[k_] for k_ in ("ngroups", "nb", "k", "launch", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj")]
        assert L.gp_heun_step_plan(a["tile"], *args, stream_ptr()) == -1, change
        if "tile" not in change or change.get("k") == 5:
            assert L.gp_heun_step_bf16x9(*args, *x9, stream_ptr()) == -1, change
    for i in range(3):
        a = [good[k_] for k_ in ("ngroups", "nb", "k", "launch", "nsteps", "denoise", "net", "cvec", "tvec", "sched", "centre", "x", "d", "score", "out", "traj")]
        packs = list(x9)
        packs[i] = None
        assert L.gp_heun_step_bf16x9(*a, *packs, stream_ptr()) == -1
    torch.cuda.synchronize()
    for buf in (x, d, score, out, traj):
        assert bool((buf == -777.0).all())
    t = ctypes.c_int(-7)
    assert L.gp_heun_layout(16 | _lib.PLAN_HEADSPLIT, 1, 5, 50, ctypes.byref(t)) == -1 and t.value == -7
    assert L.gp_heun_layout(0, 1, 5, 50, ctypes.byref(t)) == 0 and t.value == 16  # the latency regime: whole 16-row tiles, not head-split
