"""GPU: ODESampler(trunk='bf16x9') - the 128-row chain plan of the device RK45 solver with the score trunk as exact-product split bf16 on
the BF16 matrix pipe (csrc/rk45.hip: rk45_stage_chain_kernel_bf16x9, gp_rk45_phase_bf16x9) - held to what the fp32 chain stage kernels are
held to: the first evaluation against fp64 (the gate of tests/test_gpu_bf16x9.py), every logged attempt replayed in float64, scipy's
schedule on the strict solves, the exact solution, dense output, per-group step control - and compared with the fp32 chain itself.

Shapes: the smallest at which a 128-row workgroup can go wrong (k >= 43: a workgroup spans at most 4 clouds) - 3 x 43 = 129 rows (a second
workgroup with one live row), 4 x 50 = 200 rows (the shape of the existing solves), 6 x 64 in 3 groups (one workgroup per group, each
with its own step controller)."""
import ctypes

import numpy as np
import pytest
import torch

import rk45_reference as rr
import test_gpu_bf16x9 as x9
import test_gpu_rk45_exact as ex
from oracle import genpose_oracle as go

pytestmark = pytest.mark.gpu

X9_KERNEL = "rk45_stage_chain_kernel<bf16x9>"


def _sampler(snet, B, K, trunk, groups=1, **kw):
    from genpose_amd.samplers import ODESampler
    smp = ODESampler(snet, B, K, "cuda", tile=128, groups=groups, trunk=trunk, **kw)
    assert smp.plan == 128 and smp.trunk == trunk
    assert smp.kernel_name == (X9_KERNEL if trunk == "bf16x9" else "rk45_stage_chain_kernel<2>")
    return smp


# ----------------------------------------------------------------------------- 1. option surface
def test_option_surface():
    from genpose_amd import _lib
    from genpose_amd.samplers import ODESampler
    net = x9._net()
    assert ODESampler(net, 640, 50, "cuda", groups=10).trunk == "f32mfma"
    assert ODESampler(net, 640, 50, "cuda", groups=10, trunk="f32mfma").trunk == "f32mfma"
    smp = ODESampler(net, 640, 50, "cuda", groups=10, trunk="bf16x9")
    assert smp.plan == 128 and smp.trunk == "bf16x9" and smp.kernel_name == X9_KERNEL
    # off the score model's equal-group chain plan the option is ignored
    tile_plan = ODESampler(net, 64, 50, "cuda", trunk="bf16x9")
    assert tile_plan.plan != 128 and tile_plan.trunk == "f32mfma" and tile_plan.kernel_name != X9_KERNEL
    energy = ODESampler(net, 640, 50, "cuda", groups=10, model="energy", tile=128, trunk="bf16x9")
    assert energy.trunk == "f32mfma" and energy.kernel_name != X9_KERNEL
    ragged = ODESampler(net, 8, 50, "cuda", group_clouds=[4, 4], trunk="bf16x9")
    assert ragged.trunk == "f32mfma" and ragged.kernel_name != X9_KERNEL
    with pytest.raises(ValueError):
        ODESampler(net, 640, 50, "cuda", groups=10, trunk="f16")
    # the entry point refuses what plan 128 refuses: k = 30 (a workgroup's rows would span more than four clouds), 3 x 43 rows per group
    s = _sampler(net, 4, 50, "bf16x9")
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    cd = ctypes.c_double

    def phase0(groups, bpg, k):
        return _lib.lib().gp_rk45_phase_bf16x9(0, groups, bpg, k, net.w.ref(), ptr(s.cvec), ptr(s.tvec), ptr(s.centre), ptr(s.state), ptr(s.y), ptr(s.ynew),
                                               ptr(s.Kbuf), ptr(s.partials), None, 0, cd(1.0), cd(1e-5), cd(1e-5), cd(1e-5), cd(0.0), 1, 0, ptr(s.x_out), None, 0,
                                               *(ptr(w) for w in s._x9), None)

    assert phase0(1, 4, 30) == -1 and phase0(2, 3, 43) == -1 and phase0(0, 4, 50) == -1
    assert phase0(1, 4, 50) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 2. fp64 gate on the first evaluation
def test_first_evaluation_against_fp64():
    """tests/test_gpu_bf16x9.py::test_first_evaluation_against_fp64 on the ODE's stage kernel: the same 6 400 rows (128 x 50, two groups), the
    same weights, the score recovered from K[0] = -g^2/2 . score of phases 0-1 at t = 1; its bound (5e-6) and its ratio (1.5)."""
    net = x9._net()
    B, K, groups = 128, 50, 2
    feat, centre, x0, _, _ = x9._inputs(B, K, 2, 5)
    cvec = net.cloud_embed(feat.cuda())
    first = {}
    for trunk in ("f32mfma", "bf16x9"):
        smp = _sampler(net, B, K, trunk, groups=groups)
        smp.cvec.copy_(cvec), smp.centre.zero_(), smp.y.copy_(x0.double().reshape(-1).cuda())
        smp._phase(0, None, t0=1.0, t_bound=rr.EPS, rtol=1e-5, atol=1e-5)
        smp._phase(1, None)
        torch.cuda.synchronize()
        first[trunk] = (smp.Kbuf[0].cpu() / (-0.5 * rr.g2(1.0))).reshape(B * K, 9)
    sd64 = {k: v.double() for k, v in go.make_state_dict(0, "score").items()}
    ref = go.score_forward(sd64, feat.repeat_interleave(K, 0).double(), x0.double(), torch.ones(B * K, 1, dtype=torch.float64))
    scale = float(ref.abs().max())
    e32 = float((first["f32mfma"] - ref).abs().max()) / scale
    e9 = float((first["bf16x9"] - ref).abs().max()) / scale
    print(f"first ODE evaluation vs fp64, max error / score scale: fp32 chain {e32:.2e}, bf16x9 {e9:.2e} (ratio {e9 / e32:.2f})")
    assert e32 < 5e-6, e32
    assert e9 <= x9.GATE_VS_F32 * e32, (e32, e9)
    assert not torch.equal(first["f32mfma"], first["bf16x9"])  # (it IS a different arithmetic)


# ----------------------------------------------------------------------------- 3. replay and ground truth
X9_SOLVES = [("contract", 1.0, 4, 50, True), ("contract", 0.15, 4, 50, True), ("time", 0.55, 4, 50, False), ("time", 1.0, 3, 43, False)]


@pytest.mark.parametrize("name,T0,B,K,strict", X9_SOLVES)
def test_solve_replay_and_ground_truth(name, T0, B, K, strict):
    """what plan 128 gets in test_gpu_rk45_exact.py::test_score_solve_replay_and_ground_truth, under the bf16x9 trunk"""
    anet, model, snet = ex._net(name)
    cvec, x, _, c_rows, fld, Y0 = ex._problem(anet, snet, model, B, K, T0)
    sc = ex._scipy_reference(fld, Y0, T0, rr.EPS)
    exact = rr.exact_solution(anet, model, Y0, c_rows, T0, [rr.EPS])[0]
    scipy_err = np.abs(sc["states"][-1].reshape(Y0.shape) - exact).max()
    smp = _sampler(snet, B, K, "bf16x9")
    run = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)[0]
    worst = rr.replay_check(fld, run, T0, rr.EPS)
    print(f"replay {name} T0={T0} {B}x{K} bf16x9: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    if strict:
        ex._same_schedule(run, sc, 128)
    end = run["states"][-1]
    assert np.abs(end - exact).max() <= 4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max())
    # the production path (denoise, normalize_rotation, centre) from the same start
    centre = torch.randn(B, 3, generator=torch.Generator().manual_seed(1)).cuda()
    _, xout = smp.run(cvec, centre, torch.from_numpy(x).cuda(), T0)
    cen_rows = centre.cpu().double().numpy().repeat(K, 0)
    xd = exact + fld(rr.EPS, exact) * 2.0 * (1 - rr.EPS) / 1000
    ref = torch.from_numpy(xd.copy())
    ref[:, :6] = go.normalize_rotation(ref[:, :6])
    ref[:, 6:] += torch.from_numpy(cen_rows)
    col = np.minimum(np.linalg.norm(xd[:, 0:3], axis=1), np.linalg.norm(xd[:, 3:6], axis=1)).min()
    tol = (4 * scipy_err + 1e-5 * max(1.0, np.abs(exact).max())) * (1 + 4 / col)
    assert np.abs(xout.cpu().numpy() - ref.numpy()).max() <= tol


# ----------------------------------------------------------------------------- 4. dense output
@pytest.mark.parametrize("num_steps", [2, 20])
def test_dense_output_exact(num_steps):
    """test_gpu_rk45_exact.py::test_dense_output_exact's problem and bound"""
    name, T0, B, K = "time", 0.55, 4, 50
    anet, model, snet = ex._net(name)
    cvec, x, _, c_rows, fld, Y0 = ex._problem(anet, snet, model, B, K, T0)
    t_eval = np.linspace(T0, rr.EPS, num_steps)
    exact = rr.exact_solution(anet, model, Y0, c_rows, T0, t_eval)
    import scipy.integrate
    sol = scipy.integrate.solve_ivp(rr.fun_flat(fld, B * K), (T0, rr.EPS), Y0.reshape(-1), method="RK45", rtol=1e-5, atol=1e-5, t_eval=t_eval)
    dense_err = np.abs(sol.y.T.reshape(num_steps, B * K, 9) - exact).max()
    smp = _sampler(snet, B, K, "bf16x9")
    xs, _ = smp.run(cvec, torch.zeros(B, 3, device="cuda"), torch.from_numpy(x).cuda(), T0, num_steps=num_steps, return_process=True)
    xs = xs.cpu().numpy().transpose(1, 0, 2)  # [S, R, 9]
    ref = torch.from_numpy(exact.reshape(-1, 9).copy())
    ref[:, :6] = go.normalize_rotation(ref[:, :6])
    ref = ref.numpy().reshape(num_steps, B * K, 9)
    y0p = torch.from_numpy(Y0.copy())
    y0p[:, :6] = go.normalize_rotation(y0p[:, :6])
    np.testing.assert_allclose(xs[0], y0p.numpy(), rtol=4 * rr.U64, atol=4 * rr.U64)
    col = min(np.linalg.norm(exact[..., 0:3], axis=-1).min(), np.linalg.norm(exact[..., 3:6], axis=-1).min())
    tol = (4 * dense_err + 1e-5 * max(1.0, np.abs(exact).max())) * (1 + 4 / col)
    assert np.abs(xs - ref).max() <= tol, (np.abs(xs - ref).max(), tol)


# ----------------------------------------------------------------------------- 5. groups
def test_grouped_solves_replay_per_group():
    """test_gpu_rk45_exact.py::test_grouped_solves_replay_per_group's 3 x (2 x 64) case: one workgroup per group, scales 1, 1e-2 and 30"""
    anet, model, snet = ex._net("time")
    G, B1, K, T0 = 3, 2, 64, 1.0
    cvec, x, _, c_rows, fld, Y0 = ex._problem(anet, snet, model, G * B1, K, T0)
    rows = B1 * K
    Y0 = Y0.copy()
    for g, s in enumerate((1.0, 1e-2, 30.0)):
        Y0[g * rows:(g + 1) * rows] *= s
    smp = _sampler(snet, G * B1, K, "bf16x9", groups=G)
    runs = rr.solve_raw(smp, cvec, torch.from_numpy(Y0).cuda(), T0, rr.EPS)
    assert len({int(r["n_attempts"]) for r in runs}) > 1 or len({tuple(r["log_h"][:3]) for r in runs}) > 1, "schedules must differ"
    for g, run in enumerate(runs):
        fg = rr.Field(anet, model, c_rows[g * rows:(g + 1) * rows])
        worst = rr.replay_check(fg, run, T0, rr.EPS)
        print(f"replay grouped bf16x9 group {g}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ----------------------------------------------------------------------------- 6. against the fp32 chain, and replays
@pytest.mark.parametrize("B,K,groups", [(3, 43, 1), (4, 50, 1), (128, 50, 2)])
def test_against_fp32_chain_and_graph_replay(B, K, groups):
    """Random weights, the tracking warm start (T0 = 0.15: short): both trunks take the same accept / reject sequence, the final poses agree
    to the bound of test_gpu_bf16x9.py::test_ragged_and_grouped_against_fp32_chain, and a second run() (the graph replay) gives equal bits."""
    net = x9._net()
    T0 = 0.15
    feat, centre, x0, _, _ = x9._inputs(B, K, 1, B + K)
    x0 = x0 / 50.0 * float(go.ve_sigma(T0))  # the prior draw's scale at T0
    cvec = net.cloud_embed(feat.cuda())
    out, acc = {}, {}
    for trunk in ("f32mfma", "bf16x9"):
        smp = _sampler(net, B, K, trunk, groups=groups)
        a = smp.run(cvec, centre.cuda(), x0.cuda(), T0)[1].clone()
        acc[trunk] = [np.asarray(s["log_acc"]).astype(bool).tolist() for s in smp.group_stats]
        b = smp.run(cvec, centre.cuda(), x0.cuda(), T0)[1]
        torch.cuda.synchronize()
        assert torch.equal(a, b), trunk
        out[trunk] = a.cpu().numpy()
    print(f"{B} x {K} in {groups}: attempts per group {[len(s) for s in acc['bf16x9']]}, "
          f"max |bf16x9 - fp32| / max |fp32| {np.abs(out['bf16x9'] - out['f32mfma']).max() / np.abs(out['f32mfma']).max():.2e}")
    assert acc["bf16x9"] == acc["f32mfma"], "the two trunks took different accept / reject sequences: the shape is path-sensitive"
    np.testing.assert_allclose(out["bf16x9"], out["f32mfma"], rtol=0, atol=2e-5 * float(np.abs(out["f32mfma"]).max()))


# ----------------------------------------------------------------------------- 7. sharded controller on the chain plan
class _OneRank:
    """torch.distributed as a world of one rank sees it: the sum of a buffer over the ranks is the buffer."""

    class ReduceOp:
        SUM = "sum"

    @staticmethod
    def all_reduce(t, op=None, group=None):
        pass


@pytest.mark.parametrize("trunk", [None, "bf16x9"])
def test_sharded_controller_on_the_chain_plan(trunk):
    """Phases 11-13 (a sharded batch: per-group sums, the caller's all-reduce, the controller on the reduced sums) through plan 128 and through
    gp_rk45_phase_bf16x9, in a world of one rank and no process group: the sums the controller reads are the sums it forms itself, added in
    another place.  Same attempt count, poses within the bound test_gpu_coupled.py holds this identity to on RCCL."""
    from genpose_amd import _lib
    from genpose_amd.samplers import ODESampler
    net = x9._net()
    B, K, groups, T0 = 4, 50, 1, 0.4
    feat, centre, x0, _, _ = x9._inputs(B, K, 1, B + K)
    x0 = x0 / 50.0 * float(go.ve_sigma(T0))
    cvec = net.cloud_embed(feat.cuda())
    smp = ODESampler(net, B, K, "cuda", use_graph=False, groups=groups, tile=128, trunk=trunk)
    assert smp.plan == 128 and smp.kernel_name == (X9_KERNEL if trunk == "bf16x9" else "rk45_stage_chain_kernel<2>")
    alone = smp.run(cvec, centre.cuda(), x0.cuda(), T0)[1].cpu().numpy()
    n_alone = int(smp.group_stats[0]["n_attempts"])
    smp.ext_sums = torch.zeros(2, groups, dtype=torch.float64, device="cuda")
    smp.ext_rows = smp.R // groups
    smp._dist = _OneRank
    sharded = smp.run(cvec, centre.cuda(), x0.cuda(), T0)[1].cpu().numpy()
    n_sharded = int(smp.group_stats[0]["n_attempts"])
    print(f"trunk {trunk}: attempts {n_alone} / {n_sharded}, max |sharded - alone| {np.abs(sharded - alone).max():.2e}")
    assert n_sharded == n_alone
    np.testing.assert_allclose(sharded, alone, rtol=0, atol=1e-9 * max(1.0, np.abs(alone).max()))
    # the entry points themselves: the controller phases need the sums, the bf16x9 one needs every pack
    ptr, cd = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_double
    solve = (net.w.ref(), ptr(smp.cvec), ptr(smp.tvec), ptr(smp.centre), ptr(smp.state), ptr(smp.y), ptr(smp.ynew), ptr(smp.Kbuf), ptr(smp.partials),
             None, 0, cd(T0), cd(rr.EPS), cd(1e-5), cd(1e-5), cd(0.0), 1, 0, ptr(smp.x_out))
    packs = [ptr(w) for w in net.w.bf16x9_packs()]
    lib = _lib.lib()
    assert lib.gp_rk45_phase_model(0, 128, None, 11, groups, B, K, *solve, None, 0, None) == -1
    assert lib.gp_rk45_phase_bf16x9(11, groups, B, K, *solve, None, 0, *packs, None) == -1
    assert lib.gp_rk45_phase_bf16x9(0, groups, B, K, *solve, None, 0, packs[0], None, packs[2], None) == -1
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 8. agent pass-through
def test_config_flag_reaches_the_sampler():
    """get_config(ode_trunk='bf16x9'): GFObjectPose.sample builds the ODE sampler with it (part of its cache key); at a chain-plan shape
    (640 clouds x 50) the poses are those of a directly built ODESampler(trunk='bf16x9') on the same prior draw."""
    from genpose_amd import synth
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.samplers import ODESampler
    assert get_config().ode_trunk is None
    B, K, T0 = 640, 50, 0.15
    pts = torch.from_numpy(synth.make_batch(B, start=0)).cuda()
    centre = pts.mean(dim=1)
    prior = torch.randn(B * K, 9, generator=torch.Generator().manual_seed(1))
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["ode"], ode_trunk="bf16x9"))
    agent.load_state_dict(go.make_state_dict(0, "score"))
    agent.net.prior_fn = lambda shape, T=1.0: prior * (0.01 * 5000.0 ** T)
    data = {"pts": pts, "pts_center": centre}
    pred = agent.pred_func(data, K, save_path=None, T0=T0).clone()
    smp = agent.net.last_sampler
    assert smp.trunk == "bf16x9" and smp.kernel_name == X9_KERNEL and smp.plan == 128
    assert any(k[0] == "ode" and k[-1] == "bf16x9" for k in agent.net._samplers.keys())
    snet = agent.net.pose_score_net
    direct = ODESampler(snet, B, K, "cuda", trunk="bf16x9")
    assert direct.trunk == "bf16x9"
    x0 = (prior * (0.01 * 5000.0 ** T0)).float().cuda()
    _, x = direct.run(snet.cloud_embed(data["pts_feat"].float()), centre.float(), x0, T0, num_steps=None, eps=agent.net.sampling_eps)
    assert torch.equal(pred.reshape(B * K, 9), x)
    # the default configuration keeps the fp32 chain
    plain = PoseNet(get_config(posenet_mode="score", sampler_mode=["ode"]))
    plain.load_state_dict(go.make_state_dict(0, "score"))
    plain.net.prior_fn = agent.net.prior_fn
    plain.pred_func({"pts": pts, "pts_center": centre}, K, save_path=None, T0=T0)
    assert plain.net.last_sampler.trunk == "f32mfma" and plain.net.last_sampler.kernel_name == "rk45_stage_chain_kernel<2>"
