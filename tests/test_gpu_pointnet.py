"""GPU parity of the vanilla PointNet encoder (csrc/pointnet.hip, genpose_amd/pointnet_encoder.py) and of the pointnet_and_pointnet2 agent
against the reference's results in g18_pointnet.npz (scratch/gen_pointnet_golden.py)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from genpose_amd import _lib
from genpose_amd.weights_synth import make_state_dict

ENC_RTOL, ENC_ATOL = 2e-4, 2e-4  # tests/test_gpu_encoder.py, G3
SHAPES = ((3, 1024), (2, 37), (1, 1), (2, 1100))
FUSED = "pointnet_and_pointnet2"


@pytest.fixture(scope="module")
def enc():
    from genpose_amd.pointnet_encoder import PointNetEncoderHIP
    return PointNetEncoderHIP(make_state_dict(0, "score", pts_encoder="pointnet"), "cuda")


def fused_agent(mode, sampler="pc", steps=5, sd=None):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    agent = PoseNet(get_config(posenet_mode=mode, sampler_mode=[sampler], sampling_steps=steps, pts_encoder=FUSED))
    agent.load_state_dict(make_state_dict(0, mode, pts_encoder=FUSED) if sd is None else sd)
    return agent


@pytest.fixture(scope="module")
def agents():
    return fused_agent("score"), fused_agent("energy")


@pytest.mark.parametrize("B,n", SHAPES)
def test_features_against_the_fixture(enc, golden, B, n):
    """(1, 1): a single point; (2, 37): the masked partial tile; (2, 1100): 23 tiles of 48 rows, the last one partial - the signed maximum
    across workgroups."""
    g = golden("g18_pointnet.npz")
    feat, trans = enc.forward(torch.from_numpy(g[f"clouds_{B}x{n}"]).cuda(), return_trans=True)
    feat, trans = feat.cpu().numpy(), trans.cpu().numpy()
    want_f, want_t = g[f"feat_{B}x{n}"], g[f"trans_{B}x{n}"]
    print(f"({B}, {n}): max |trans - ref| = {np.abs(trans - want_t).max():.3e}, max |feat - ref| = {np.abs(feat - want_f).max():.3e}")
    np.testing.assert_allclose(trans, want_t, rtol=ENC_RTOL, atol=ENC_ATOL)
    np.testing.assert_allclose(feat, want_f, rtol=ENC_RTOL, atol=ENC_ATOL)
    big = np.abs(want_f) > 1e-3
    assert (want_f[big] < 0).any() and np.array_equal(np.sign(feat[big]), np.sign(want_f[big]))


def test_zero_cloud_equals_the_single_zero_point(enc):
    """Every row of an all-zero cloud equals the bias chain - and so does a row that pads the tile: the result must be the single-point
    one, bit for bit (a padding row that reaches the maximum shows where real rows and padding rows differ, e.g. through trans)."""
    f37, t37 = enc.forward(torch.zeros(2, 37, 3, device="cuda"), return_trans=True)
    f1, t1 = enc.forward(torch.zeros(1, 1, 3, device="cuda"), return_trans=True)
    assert torch.equal(t37, t1.expand(2, 3, 3)) and torch.equal(f37, f1.expand(2, 1024))
    # and with a transform that moves the padding rows' (zero) points nowhere but real points somewhere: one real point, 36 copies of it
    p = torch.tensor([0.3, -0.2, 0.5], device="cuda")
    assert torch.equal(enc.forward(p.expand(2, 37, 3).contiguous()), enc.forward(p.view(1, 1, 3)).expand(2, 1024))


def test_graph_replay_is_the_direct_pass(enc, golden):
    g = golden("g18_pointnet.npz")
    a, b = torch.from_numpy(g["clouds_2x1100"]).cuda(), torch.from_numpy(g["clouds_2x37"]).cuda()
    direct = enc.encode(a, use_graph=False)
    r1 = enc.encode(a)       # first call: launch by launch
    r2 = enc.encode(a)       # captures
    other = enc.encode(b)    # a second shape in between
    r3 = enc.encode(a)       # replays
    assert (2, 1100, 3) in enc._pass_graphs
    for r in (r1, r2, r3):
        assert torch.equal(r, direct)
    assert torch.equal(other, enc.encode(b, use_graph=False))


@pytest.mark.parametrize("B,n", [(3, 1024), (2, 37)])
def test_workspace_bound(enc, golden, B, n):
    pts = torch.from_numpy(golden("g18_pointnet.npz")[f"clouds_{B}x{n}"]).cuda()
    for _ in range(3):
        enc.encode(pts)
    assert (B, n, 3) in enc._pass_graphs
    used = enc.workspace_bytes(B, n)
    assert 0 < used <= B * (24 * n + 64 * 1024), used
    assert all(t.numel() <= B * 1024 for t in enc._workspace(B, n).values() if torch.is_tensor(t))  # nothing proportional to n * C


def test_fused_agent_against_the_fixture(agents, golden):
    g = golden("g18_pointnet.npz")
    sa, ea = agents
    pts = torch.from_numpy(g["clouds_3x1024"]).cuda()
    for agent, name in ((sa, "score"), (ea, "energy")):
        feat = agent.net({"pts": pts}, mode="pts_feature").cpu().numpy()
        print(f"fused {name}: max |pts_feat - ref| = {np.abs(feat - g[f'fused_feat_{name}']).max():.3e}")
        np.testing.assert_allclose(feat, g[f"fused_feat_{name}"], rtol=ENC_RTOL, atol=ENC_ATOL)
    # the grouping ticket serves the PointNet++ half only: the energy agent's features do not depend on whether it takes the grouping over
    shared = {"pts": pts}
    sa.net(shared, mode="pts_feature")
    assert "_grouping" in shared
    assert torch.equal(ea.net(shared, mode="pts_feature"), ea.net({"pts": pts}, mode="pts_feature"))
    # pred_func, PC sampler, logged draws (tolerances: tests/test_gpu_sampler.py, G7) and get_energy on its result (G8's)
    pts2 = pts[:2].contiguous()
    data = {"pts": pts2, "pts_center": pts2.mean(dim=1)}
    saved, prior = sa.net.prior_fn, torch.from_numpy(g["pc_prior_noise"])
    sa.net.prior_fn = lambda shape, T=1.0: prior * (0.01 * (50.0 / 0.01) ** T)  # the logged draw in place of ve_prior's (sde.py:26-28)
    try:
        pred, proc = sa.pred_func(data, repeat_num=4, save_path=None, return_process=True,
                                  noise=(torch.from_numpy(g["pc_z_langevin"]).cuda(), torch.from_numpy(g["pc_z_predictor"]).cuda()))
    finally:
        sa.net.prior_fn = saved
    np.testing.assert_allclose(data["pts_feat"].cpu().numpy(), g["fused_feat_score"][:2], rtol=ENC_RTOL, atol=ENC_ATOL)  # the side effect
    np.testing.assert_allclose(pred.cpu().numpy(), g["pc_pred"], rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(proc.cpu().numpy(), g["pc_proc"], rtol=1e-3, atol=5e-3)
    energy = ea.get_energy(data={"pts": pts2, "pts_center": pts2.mean(dim=1)}, pose_samples=torch.from_numpy(g["pc_pred"]).cuda(), T=1e-5)
    np.testing.assert_allclose(energy.cpu().numpy(), g["pc_energy"], rtol=5e-4, atol=5e-4 * np.abs(g["pc_energy"]).max())


def test_fused_agent_call_surface(agents, golden, tmp_path):
    """Every agent call that exists today, for both posenet_modes: the other sampler, the string-dispatched modes, load_ckpt; and the code
    that drives the PointNet++ stages itself refuses the fused agent at construction."""
    from genpose_amd.pipeline import FullPipelinePredictor, PipelinedPCPredictor
    from genpose_amd.runner import TrackingRunner
    g = golden("g18_pointnet.npz")
    sa, ea = agents
    pts = torch.from_numpy(g["clouds_3x1024"][:2]).cuda()
    feat = {a: a.net({"pts": pts}, mode="pts_feature") for a in (sa, ea)}
    for mode in ("score", "energy"):
        ode = fused_agent(mode, sampler="ode", steps=None)
        pred = ode.pred_func({"pts": pts, "pts_center": pts.mean(dim=1)}, 4, save_path=None, T0=0.55)
        assert pred.shape == (2, 4, 9) and bool(torch.isfinite(pred).all())
        pc = (sa if mode == "score" else ea).pred_func({"pts": pts, "pts_center": pts.mean(dim=1)}, 4, save_path=None)
        assert pc.shape == (2, 4, 9) and bool(torch.isfinite(pc).all())
    pose = torch.from_numpy(g["pc_pred"]).cuda().reshape(8, 9)
    for a, modes in ((sa, ("score",)), (ea, ("score", "energy"))):
        for m in modes:
            rows = {"pts_feat": feat[a], "sampled_pose": pose, "t": torch.full((8, 1), 0.3, device="cuda"), "_repeat": 4}
            out = a.net(rows, mode=m)
            assert out.shape == (8, 9 if m == "score" else 2) and bool(torch.isfinite(out).all())
    path = str(tmp_path / "fused.pth")
    torch.save({"model_state_dict": make_state_dict(0, "score", pts_encoder=FUSED)}, path)
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    loaded = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=5, pts_encoder=FUSED))
    loaded.load_ckpt(model_dir=path, model_path=True, load_model_only=True)
    assert torch.equal(loaded.net({"pts": pts}, mode="pts_feature"), feat[sa])
    for build in (lambda: PipelinedPCPredictor(sa, 2, 4, 5), lambda: FullPipelinePredictor(sa, ea, 2, 4, 5), lambda: TrackingRunner(sa, ea)):
        with pytest.raises(NotImplementedError, match=FUSED):
            build()


def test_default_agent_is_untouched(golden):
    """pts_encoder='pointnet2': the agent's features are the PointNet++ encoder's own, bit for bit, and G3's."""
    from genpose_amd.config import get_config
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from genpose_amd.posenet_agent import PoseNet
    from oracle import genpose_oracle as go
    g = golden("g3_encoder.npz")
    sd = go.make_state_dict(0, "score")
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["ode"]))
    agent.load_state_dict(sd)
    assert agent.net.fusion_layer is None and agent.net.pts_pointnet_encoder is None and isinstance(agent.net.pts_encoder, Pointnet2EncoderHIP)
    pts = torch.from_numpy(g["clouds"]).cuda()
    feat = agent.net({"pts": pts}, mode="pts_feature")
    assert torch.equal(feat, Pointnet2EncoderHIP(sd, "cuda").forward(pts))
    np.testing.assert_allclose(feat.cpu().numpy(), g["feat"], rtol=ENC_RTOL, atol=ENC_ATOL)


def test_argument_contract(enc):
    """n = 0, a null pointer and b < 0 return GP_EINVAL before any launch: the outputs keep their sentinel."""
    lib = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    xyz, trans = torch.zeros(2, 8, 3, device="cuda"), torch.eye(3, device="cuda").repeat(2, 1, 1)
    out = torch.full((2, 1024), 7.5, device="cuda")
    s = [p(t) for pair in enc.w.stn_convs for t in pair]
    c = [p(t) for pair in enc.w.convs for t in pair]
    W, b = enc.w.stn_fcs[0]
    h = torch.full((2, 512), 7.5, device="cuda")
    calls = []
    for bb, n, x, o in ((2, 0, p(xyz), p(out)), (-1, 8, p(xyz), p(out)), (2, 8, None, p(out)), (2, 8, p(xyz), None)):
        calls.append(lib.gp_pointnet_stn_pool(bb, n, x, *s, o, None))
        calls.append(lib.gp_pointnet_feat_pool(bb, n, x, p(trans), *c, o, None))
    calls.append(lib.gp_pointnet_feat_pool(2, 8, p(xyz), None, *c, p(out), None))
    calls.append(lib.gp_pointnet_stn_pool(2, 8, p(xyz), None, *s[1:], p(out), None))
    for rows, ka, xa, o in ((-1, 1024, p(out), p(h)), (2, 0, p(out), p(h)), (2, 1022, p(out), p(h)), (2, 1024, None, p(h)), (2, 1024, p(out), None)):
        calls.append(lib.gp_dense_rows(rows, ka, 0, 512, xa, None, p(W), p(b), 1, o, None))
    calls.append(lib.gp_dense_rows(2, 1024, 0, 512, p(out), None, p(W), p(b), 2, p(h), None))   # unknown activation
    calls.append(lib.gp_dense_rows(2, 512, 512, 512, p(out), None, p(W), p(b), 1, p(h), None))  # second half without its input
    torch.cuda.synchronize()
    assert calls == [-1] * len(calls)
    assert bool((out == 7.5).all()) and bool((h == 7.5).all())
    assert lib.gp_pointnet_stn_pool(0, 8, p(xyz), *s, p(out), None) == 0 and lib.gp_dense_rows(0, 1024, 0, 512, p(out), None, p(W), p(b), 1, p(h), None) == 0
    torch.cuda.synchronize()
    assert bool((out == 7.5).all()) and bool((h == 7.5).all())
