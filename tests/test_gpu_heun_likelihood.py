"""GPU: the fixed-step Heun solve of the exact-likelihood ODE - heun_likelihood_step_kernel (csrc/heun_likelihood.hip) behind
gp_heun_likelihood_step, samplers.HeunLikelihood, cond_ode_likelihood / calc_likelihood / PoseNet.get_likelihood(solver='heun') and the
likelihood ranker of SingleFrameRunner.

Ground truth is float64 and built here: tests/heun_likelihood_reference.py (the same Heun steps on the same grid, float64 network in closed
form) for the solve itself, tests/exact_likelihood_ref.py's adaptive float64 solve for its convergence.  The kernel's evaluation is held
bit for bit to the existing gp_score_div_exact."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import exact_likelihood_ref as er
import heun_likelihood_reference as hl
from oracle import genpose_oracle as go

SHAPES = [(1, 1), (1, 17), (3, 5), (2, 50)]  # single row; partial tile; tiles that span clouds; more than one tile
EPS = 1e-5
NSTEPS = 4
# the band the RK45 exact solve is granted against its float64 solve (tests/test_gpu_exact_likelihood.py: LIKELIHOOD_RTOL), restated
LIKELIHOOD_RTOL = 2e-3
CONVERGED_N = 1024  # the N of test_converges_to_the_adaptive_solve that must lie inside that band (its docstring says why not 32)
HERE = os.path.dirname(os.path.abspath(__file__))
CKPT_SCORE = os.path.join(HERE, "golden", "trained", "ckpt_score.pth")

_cache = {}


def _net(seed):
    from genpose_amd.scorenet import ScoreNetHIP
    if ("net", seed) not in _cache:
        _cache["net", seed] = ScoreNetHIP(go.make_state_dict(seed, "score"), "cuda")
    return _cache["net", seed]


def _inputs(seed, B, K):
    """cloud features, poses near the data (t = 1e-5) and the cloud embedding of one (weights seed, shape): drawn once"""
    key = ("in", seed, B, K)
    if key not in _cache:
        gen = torch.Generator().manual_seed(100 * seed + 7 * B + K)
        pf = torch.randn(B, 1024, generator=gen).abs()
        x = er.unit_axis_poses(B * K, EPS, gen)
        _cache[key] = dict(pf=pf, x=x, cvec=_net(seed).cloud_embed(pf.cuda()), xd=x.cuda())
    return _cache[key]


def _solve(seed, B, K, N=NSTEPS, grid="geometric"):
    """the device solve of one case through HeunLikelihood: (z [R,9] f32, delta_logp [R] f64, bits [R] f64) as numpy, computed once"""
    from genpose_amd.likelihood import cond_ode_likelihood
    key = ("solve", seed, B, K, N, grid)
    if key not in _cache:
        c = _inputs(seed, B, K)
        st = {}
        z, bits = cond_ode_likelihood(_net(seed), c["cvec"], K, c["xd"], None, eps=EPS, divergence="exact", solver="heun", steps=N, grid=grid, stats=st)
        assert st == {"nfev": 2 * N, "attempts": N}
        assert z.dtype == torch.float32 and bits.dtype == torch.float64 and z.shape == (B * K, 9) and bits.shape == (B * K,)
        _cache[key] = (z.cpu().numpy(), bits.cpu().numpy())
    return _cache[key]


def _reference(seed, B, K, N=NSTEPS, dtype="float64"):
    key = ("ref", seed, B, K, N, dtype)
    if key not in _cache:
        c = _inputs(seed, B, K)
        field = hl.closed_form_field(go.make_state_dict(seed, "score"), c["pf"].repeat_interleave(K, 0), dtype)
        z, _, bits = hl.solve(field, c["x"].double().numpy(), N, eps=EPS)
        _cache[key] = (z, bits)
    return _cache[key]


def _solver(seed, B, K, N=NSTEPS, **kw):
    from genpose_amd.samplers import HeunLikelihood
    return HeunLikelihood(_net(seed), B, K, "cuda", N, **kw)


# ------------------------------------------------------------------------------------------------ 1. the first launches
@pytest.mark.parametrize("seed", [0, 1])
def test_first_launches_are_gp_score_div_exact_and_its_products(seed):
    """Launch 0 alone leaves score / div bit-identical to gp_score_div_exact(x_0, t_0) - the right tvec_all row and sigma; after launch 1,
    d holds the fp32 products c * score and c * div - the right factor."""
    from genpose_amd.samplers import heun_likelihood_schedule
    net = _net(seed)
    for B, K in SHAPES:
        c = _inputs(seed, B, K)
        smp = _solver(seed, B, K, use_graph=False)
        smp.cvec.copy_(c["cvec"])
        smp.x.copy_(c["xd"])
        smp._write_schedule(EPS, 1.0)
        smp.d.fill_(-7.0)
        smp.launch_step(0)
        torch.cuda.synchronize()
        t, sched = heun_likelihood_schedule(NSTEPS, EPS)
        assert torch.equal(smp.sched.cpu(), torch.from_numpy(sched).reshape(-1)) and torch.equal(smp.t_dev.cpu(), torch.from_numpy(t.astype(np.float32)))
        t0, sigma0 = smp.t_dev[:1].clone(), smp.sched[:1].clone()
        assert float(t0) == float(np.float32(EPS)) and float(sigma0) == float(sched[0, 0])
        s_ref, d_ref = net.score_and_exact_divergence(c["cvec"], K, c["xd"], net.time_embed(t0)[0], sigma0)
        score0, div0 = smp.score.clone(), smp.div.clone()
        assert torch.equal(score0, s_ref) and torch.equal(div0, d_ref), (seed, B, K)
        assert bool((smp.d == -7).all()) and torch.equal(smp.x, c["xd"])  # launch 0 stores nothing else
        smp.launch_step(1)
        torch.cuda.synchronize()
        cf = smp.sched.view(-1, 4)[1, 1]
        assert float(cf) == -float(sigma0)
        assert torch.equal(smp.d[:, :9], cf * score0) and torch.equal(smp.d[:, 9], cf * div0), (seed, B, K)
        assert torch.equal(smp.x, c["xd"])  # the Euler point is evaluated, never stored


# ------------------------------------------------------------------------------------------------ 2. the whole solve
@pytest.mark.parametrize("seed", [0, 1])
def test_solve_matches_the_float64_restatement(seed):
    """N = 4 on the same grid against the float64 network: bits and z of EVERY row inside rtol = 2e-3, atol = 2e-3 max|ref| - no row is
    excluded.  The float32 closed form of the same network (the reference in the kernels' precision, CPU) is held to the same band first:
    were a ReLU kink to flip a row there, the band could not be asked of the kernel either."""
    for B, K in SHAPES:
        z_ref, bits_ref = _reference(seed, B, K)
        z32, bits32 = _reference(seed, B, K, dtype="float32")
        z, bits = _solve(seed, B, K)
        band = lambda a, ref: np.abs(a - ref) <= LIKELIHOOD_RTOL * (np.abs(ref) + np.abs(ref).max())
        e = lambda a, ref: np.abs(a - ref).max() / np.abs(ref).max()
        print(f"seed {seed} shape ({B},{K}): bits err {e(bits, bits_ref):.2e} z err {e(z, z_ref):.2e}  |  float32 closed form: bits {e(bits32, bits_ref):.2e} "
              f"z {e(z32, z_ref):.2e}  max|bits| {np.abs(bits_ref).max():.4g}")
        assert band(bits32, bits_ref).all() and band(z32, z_ref).all(), (seed, B, K)
        assert np.isfinite(bits).all() and np.isfinite(z).all()
        np.testing.assert_allclose(bits, bits_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(bits_ref).max())
        np.testing.assert_allclose(z, z_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(z_ref).max())


@pytest.mark.parametrize("grid", ["geometric", "edm"])
def test_both_grids(grid):
    """the 'edm' grid through the same kernel (the kernel knows nothing about the grid): the float64 restatement on that grid"""
    B, K, N = 2, 50, 6
    c = _inputs(0, B, K)
    field = hl.closed_form_field(go.make_state_dict(0, "score"), c["pf"].repeat_interleave(K, 0))
    z_ref, _, bits_ref = hl.solve(field, c["x"].double().numpy(), N, eps=EPS, kind=grid)
    z, bits = _solve(0, B, K, N, grid)
    np.testing.assert_allclose(bits, bits_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(bits_ref).max())
    np.testing.assert_allclose(z, z_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(z_ref).max())


# ------------------------------------------------------------------------------------------------ 3. row-locality
def test_a_row_is_a_function_of_itself_bit_for_bit():
    """Row (cloud 1, pose 3) solved alone, inside (2,50) and inside a call that holds only the first 7 candidates of its cloud: identical z
    and delta_logp.  The same through PoseNet.get_likelihood(solver='heun')."""
    B, K, cl, j = 2, 50, 1, 3
    c = _inputs(0, B, K)
    r = cl * K + j
    out = []
    for cv, k, x, pick in ((c["cvec"], K, c["xd"], r), (c["cvec"][cl:cl + 1], 1, c["xd"][r:r + 1], 0),
                           (c["cvec"][cl:cl + 1], 7, c["xd"][cl * K:cl * K + 7], j)):
        smp = _solver(0, cv.shape[0], k)
        z, l = smp.run(cv.contiguous(), x.contiguous(), eps=EPS)
        out.append((z[pick].clone(), l[pick].clone()))
    for z, l in out[1:]:
        assert torch.equal(z, out[0][0]) and torch.equal(l, out[0][1])
    assert np.array_equal(out[0][0].cpu().numpy(), _solve(0, B, K)[0][r])
    # the agent: the same cloud features, one row per cloud; three calls of different shapes
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    agent = PoseNet(get_config(posenet_mode="score"))
    agent.load_state_dict(go.make_state_dict(0, "score"))
    feat, poses, centre = c["pf"].cuda(), c["xd"].view(B, K, 9), torch.zeros(B, 3, device="cuda")
    ll = []
    for sl_c, sl_k, pick in ((slice(0, B), slice(0, K), (cl, j)), (slice(cl, cl + 1), slice(j, j + 1), (0, 0)), (slice(cl, cl + 1), slice(0, 7), (0, j))):
        data = {"pts_feat": feat[sl_c].contiguous(), "pts_center": centre[sl_c]}
        v = agent.get_likelihood(data, poses[sl_c, sl_k].contiguous(), extract_pts_feature=False, solver="heun", steps=NSTEPS)
        assert v.dtype == torch.float64 and agent.net.last_likelihood_stats == {"nfev": 2 * NSTEPS, "attempts": NSTEPS}
        ll.append(v[pick].item())
    assert ll[0] == ll[1] == ll[2]
    assert ll[0] == _solve(0, B, K)[1][r]


# ------------------------------------------------------------------------------------------------ 4. convergence
def test_converges_to_the_adaptive_solve():
    """2 clouds x 3 poses (test_gpu_exact_likelihood.py::test_exact_likelihood_solve's inputs) against the adaptive float64 solve of the same
    ODE: the error of N = 8 / 16 / 32 falls monotonically and N = CONVERGED_N lies inside the 2e-3 band.

    N = 32 is NOT inside, and the band is not widened.  Measured on MI355X (profiles/heun_likelihood.txt), worst |bits - ref| / max|ref| and
    worst |z - ref| / max|ref| over the six rows, geometric grid: N = 8: 9.8e-1 / 8.8e-1, 16: 9.2e-1 / 7.3e-1, 32: 7.1e-1 / 4.7e-1, 64: 3.7e-1 /
    2.1e-1, 128: 1.4e-1 / 7.3e-2, 256: 4.2e-2 / 2.2e-2, 512: 1.1e-2 / 5.7e-3, 1024: 2.8e-3 / 1.4e-3 (3.8 - 3.95 per doubling from 256 on).  With
    these random weights the rows sit at -3 300 .. -16 000 bits and the flow is stiff near the data; the solve is second order but far from
    converged at tens of steps.  The smallest N found inside the band is 856 (bisection between 512 and 1024; bits 3.98e-3 against the 4e-3
    that rtol + atol grant the largest row) - but the boundary is jagged at the level of fp32 rounding (856 inside, 857 and 858 outside, 859
    inside), so the asserted N is the next doubling, 1024, which is inside with a margin of 30 %."""
    B, K = 2, 3
    sd = go.make_state_dict(0, "score")
    gen = torch.Generator().manual_seed(5)
    pf = torch.randn(B, 1024, generator=gen).abs()
    x = er.unit_axis_poses(B * K, EPS, gen)
    z_ref, bits_ref, _ = er.solve_f64(sd, pf.repeat_interleave(K, 0), x)
    net = _net(0)
    cvec = net.cloud_embed(pf.cuda())
    from genpose_amd.likelihood import cond_ode_likelihood
    res = {}
    for N in sorted({8, 16, 32, CONVERGED_N}):
        z, bits = cond_ode_likelihood(net, cvec, K, x.cuda(), None, eps=EPS, divergence="exact", solver="heun", steps=N)
        res[N] = (z.cpu().numpy(), bits.cpu().numpy())
    eb = {N: np.abs(b - bits_ref).max() / np.abs(bits_ref).max() for N, (_, b) in res.items()}
    ez = {N: np.abs(z - z_ref).max() / np.abs(z_ref).max() for N, (z, _) in res.items()}
    print("Heun vs adaptive float64 solve, worst |bits - ref| / max|ref|:", {N: f"{v:.2e}" for N, v in eb.items()}, " z:", {N: f"{v:.2e}" for N, v in ez.items()})
    assert eb[8] > eb[16] > eb[32]
    z, bits = res[CONVERGED_N]
    np.testing.assert_allclose(bits, bits_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(bits_ref).max())
    np.testing.assert_allclose(z, z_ref, rtol=LIKELIHOOD_RTOL, atol=LIKELIHOOD_RTOL * np.abs(z_ref).max())


# ------------------------------------------------------------------------------------------------ 5. sentinels and refusals
@pytest.mark.parametrize("B,K", [(2, 50), (1, 17)])
def test_sentinels_and_refusals(B, K):
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.samplers import heun_likelihood_schedule
    c = _inputs(0, B, K)
    net, R, TAIL, N = _net(0), B * K, 64, NSTEPS
    fn = _lib.lib().gp_heun_likelihood_step
    t, sched = heun_likelihood_schedule(N, EPS)
    sched_d = torch.from_numpy(sched).cuda()
    tvec_all = net.time_embed(torch.from_numpy(t.astype(np.float32)).cuda())

    def bufs():
        f = lambda n, dt=torch.float32: torch.full((n + TAIL,), -7.0, device="cuda", dtype=dt)
        return dict(x=f(R * 9), d=f(R * 10), score=f(R * 9), div=f(R), logp=f(R, torch.float64), z=f(R * 9))

    def args(b, launch):
        return [B, K, launch, N, net.w.ref(), ptr(c["cvec"]), ptr(tvec_all), ptr(sched_d), ptr(b["x"]), ptr(b["d"]), ptr(b["score"]), ptr(b["div"]),
                ptr(b["logp"]), ptr(b["z"]), stream_ptr()]

    b = bufs()
    b["x"][: R * 9] = c["xd"].reshape(-1)
    for launch in range(2 * N + 1):
        assert fn(*args(b, launch)) == 0
    torch.cuda.synchronize()
    for name, n in (("x", R * 9), ("d", R * 10), ("score", R * 9), ("div", R), ("logp", R), ("z", R * 9)):
        assert bool((b[name][n:] == -7).all()), name
        assert not bool((b[name][:n] == -7).any()), name
    z, bits = _solve(0, B, K)
    assert np.array_equal(b["z"][: R * 9].reshape(R, 9).cpu().numpy(), z)
    prior = -9 / 2.0 * np.log(2 * np.pi * 2500.0) - (z.astype(np.float64) ** 2).sum(-1) / 5000.0
    np.testing.assert_allclose((prior + b["logp"][:R].cpu().numpy()) / np.log(2), bits, rtol=1e-12)
    # refusals: GP_EINVAL, nothing written
    b = bufs()
    good = args(b, 2)
    for i in range(4, 14):
        bad = list(good)
        bad[i] = None
        assert fn(*bad) == -1, i
    for i, v in ((1, 0), (3, 0), (2, -1), (2, 2 * N + 1)):
        bad = list(good)
        bad[i] = v
        assert fn(*bad) == -1, (i, v)
    stripped = _lib.GpScoreNet(**{n: (None if n in ("w_headx_t", "w_pose2_t", "w_pose0_t") else getattr(net.w.struct, n)) for n, _ in _lib.GpScoreNet._fields_})
    bad = list(good)
    bad[4] = ctypes.byref(stripped)
    assert fn(*bad) == -1
    bad = list(good)
    bad[0] = 0  # no rows: GP_OK, nothing to write
    assert fn(*bad) == 0
    torch.cuda.synchronize()
    assert all(bool((v == -7).all()) for v in b.values())


# ------------------------------------------------------------------------------------------------ 6. replay and capture
def test_replay_capture_and_generator():
    B, K = 2, 50
    c = _inputs(0, B, K)
    smp = _solver(0, B, K)
    torch.manual_seed(11)
    state = torch.get_rng_state()
    z1, l1 = (v.clone() for v in smp.run(c["cvec"], c["xd"], eps=EPS))
    z2, l2 = (v.clone() for v in smp.run(c["cvec"], c["xd"], eps=EPS))
    assert smp.captures == 1 and torch.equal(z1, z2) and torch.equal(l1, l2)
    assert np.array_equal(z1.cpu().numpy(), _solve(0, B, K)[0])
    z3, l3 = (v.clone() for v in smp.run(c["cvec"], c["xd"], eps=1e-3))  # another eps: the tables are refilled, the chain is not recaptured
    assert smp.captures == 1 and not torch.equal(l3, l1)
    ref = _solver(0, B, K, use_graph=False)
    z4, l4 = ref.run(c["cvec"], c["xd"], eps=1e-3)
    assert ref.captures == 0 and torch.equal(z3, z4) and torch.equal(l3, l4)
    z5, l5 = smp.run(c["cvec"], c["xd"], eps=EPS)
    assert smp.captures == 1 and torch.equal(z5, z1) and torch.equal(l5, l1)
    assert torch.equal(torch.get_rng_state(), state)
    assert smp.last_stats["nfev"] == 2 * NSTEPS and smp.last_stats["launches"] == 2 * NSTEPS + 1


# ------------------------------------------------------------------------------------------------ 7. ranking
def test_likelihood_ranker():
    """PoseNet.get_likelihood(solver='heun', steps=8) on the trained score checkpoint: 4 held-out synthetic clouds x 8 PC-20 candidates ->
    [4,8] finite bits without ties; as both energy columns it orders the candidates by descending likelihood; SingleFrameRunner(score_agent,
    None, ranker='likelihood') returns what its own pieces return when called by hand."""
    from genpose_amd import reward, rotation, synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import SingleFrameRunner, make_batch_sample
    B, K = 4, 8
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=20, likelihood_solver="heun", likelihood_steps=8))
    agent.load_ckpt(model_dir=CKPT_SCORE, model_path=True, load_model_only=True)
    pts = torch.from_numpy(synth.posed_batch(range(1_000_000, 1_000_000 + B))["pts"]).cuda()
    sample = make_batch_sample(pts)
    torch.manual_seed(3)
    pred = agent.pred_func(data=sample, repeat_num=K, save_path=None, T0=0.55)
    ll = agent.get_likelihood(sample, pred, extract_pts_feature=False, solver="heun", steps=8)
    assert ll.shape == (B, K) and ll.dtype == torch.float64 and bool(torch.isfinite(ll).all())
    assert torch.equal(ll, agent.get_likelihood(sample, pred, extract_pts_feature=False))  # the config's solver and steps
    ll32 = ll.float()
    assert all(len(set(row.tolist())) == K for row in ll32)  # no ties, also not after the cast to the energy dtype
    energy = torch.stack([ll32, ll32], dim=-1).contiguous()
    r = reward.rank_aggregate(pred, energy, ratio=0.6)
    want = torch.argsort(-ll32, dim=1)
    assert torch.equal(r["order"][:, :, 0].long(), want) and torch.equal(r["order"][:, :, 1].long(), want)
    runner = SingleFrameRunner(agent, None, repeat_num=K, T0=0.55, batch_size=B, ratio=0.6, ranker="likelihood")
    torch.manual_seed(3)
    out = runner.infer_tensors(pts)
    assert out["sorted_RTs"].shape == (B, K, 4, 4) and out["average_sRT"].shape == (B, 4, 4) and out["energy"].shape == (B, K, 2)
    assert torch.equal(out["pred_pose"], pred) and torch.equal(out["energy"], energy)
    assert torch.equal(out["sorted_RTs"], rotation.pose9_to_RT(r["sorted_poses"]))
    assert torch.equal(out["average_sRT"], rotation.quat_trans_to_RT(r["avg_pose"].double()))
    print("Heun-8 log-likelihood (bits) of the candidates of cloud 0:", ll[0].cpu().numpy())
