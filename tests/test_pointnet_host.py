"""Host side of the vanilla PointNet encoder (csrc/pointnet.hip, genpose_amd/pointnet_encoder.py) and of the pointnet_and_pointnet2 agent:
the fixture g18_pointnet.npz pinned without the reference, the synthetic weights, host-only loading, weight packing, the C ABI."""
import os
import re

import numpy as np
import pytest
import torch

from genpose_amd import _lib
from genpose_amd.weights_synth import make_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((3, 1024), (2, 37), (1, 1), (2, 1100))
# The fixture is the reference's fp32 CPU result.  Its distance to exact arithmetic: every layer is a dot product of K <= 1024 fp32 terms
# (relative error <= K * 2^-24 of sum |a_i b_i| in the worst case, ~sqrt(K) * 2^-24 typically) over at most 7 layers with values of order 0.1 - 1,
# i.e. a few 1e-6 typically and 7 * 1024 * 6e-8 ~ 4e-4 at the very worst.  1e-4 sits between the two; the largest difference observed
# is in DESIGN.md section 5 (1.7e-6).
F64_ATOL = F64_RTOL = 1e-4


def pointnet_f64(sd, pts, prefix="pts_encoder."):
    """PointNetfeat(num_points, out_dim=1024) (networks/pts_encoder/pointnets.py:45-118, no BatchNorm) in float64, points as rows:
    pts [B,n,3] -> (trans [B,3,3], feat [B,1024])."""
    r = torch.relu
    lin = lambda x, name: x @ sd[prefix + name + ".weight"].double().reshape(sd[prefix + name + ".weight"].shape[0], -1).T + sd[prefix + name + ".bias"].double()
    x = pts.double()
    g = r(lin(r(lin(r(lin(x, "stn.conv1")), "stn.conv2")), "stn.conv3")).max(dim=1)[0]
    trans = (lin(r(lin(r(lin(g, "stn.fc1")), "stn.fc2")), "stn.fc3") + torch.eye(3, dtype=torch.float64).reshape(9)).view(-1, 3, 3)
    y = torch.bmm(x, trans)
    feat = lin(r(lin(r(lin(r(lin(y, "conv1")), "conv2")), "conv3")), "conv4").max(dim=1)[0]
    return trans, feat


@pytest.fixture(scope="module")
def sd_pointnet():
    return make_state_dict(0, "score", pts_encoder="pointnet")


def test_fixture_is_self_consistent(golden, sd_pointnet):
    g = golden("g18_pointnet.npz")
    worst = 0.0
    for B, n in SHAPES:
        trans, feat = pointnet_f64(sd_pointnet, torch.from_numpy(g[f"clouds_{B}x{n}"]))
        for name, want in (("trans", trans), ("feat", feat)):
            got = g[f"{name}_{B}x{n}"]
            worst = max(worst, float(np.abs(got - want.numpy()).max()))
            np.testing.assert_allclose(got, want.numpy(), rtol=F64_RTOL, atol=F64_ATOL, err_msg=f"{name} at {(B, n)}")
        # what the GPU tests rely on: signed pooled values, a transform that is visibly not the identity
        assert (g[f"feat_{B}x{n}"] < 0).mean() > 0.2
        assert np.abs(g[f"trans_{B}x{n}"] - np.eye(3)).max() > 0.1
    print(f"fixture (reference, fp32) vs float64: max |diff| = {worst:.3e}")


def survey_keys():
    """The default checkpoint's key list, SURVEY.md section 5."""
    keys = []
    for k in range(4):
        for i in range(2):
            for l in range(3):
                p = f"pts_encoder.SA_modules.{k}.mlps.{i}.layer{l}."
                keys += [p + "conv.weight"] + [p + "bn.bn." + s for s in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
    q = "pose_score_net."
    keys += [q + f"pose_encoder.{j}.{s}" for j in (0, 2) for s in ("weight", "bias")] + [q + "t_encoder.0.W", q + "t_encoder.1.weight", q + "t_encoder.1.bias"]
    keys += [q + f"fusion_tail_{h}.{j}.{s}" for h in ("rot_x", "rot_y", "trans") for j in (0, 2) for s in ("weight", "bias")]
    return keys


def test_default_weights_unchanged():
    a, b = make_state_dict(0, "score"), make_state_dict(0, "score", pts_encoder="pointnet2")
    assert list(a) == list(b) and sorted(a) == sorted(survey_keys())
    assert not any("stn" in k or "fusion_layer" in k for k in a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].numpy().tobytes() == b[k].numpy().tobytes(), k
    # the fused layout: the same PointNet++ / score-net bytes under the reference's second prefix, plus the new keys
    f = make_state_dict(0, "score", pts_encoder="pointnet_and_pointnet2")
    for k in a:
        kk = "pts_pointnet2_encoder." + k[len("pts_encoder."):] if k.startswith("pts_encoder.") else k
        assert f[kk].numpy().tobytes() == a[k].numpy().tobytes(), k
    extra = sorted(set(f) - {("pts_pointnet2_encoder." + k[len("pts_encoder."):] if k.startswith("pts_encoder.") else k) for k in a})
    want = [f"pts_pointnet_encoder.{m}.{s}" for m in ["stn.conv1", "stn.conv2", "stn.conv3", "stn.fc1", "stn.fc2", "stn.fc3", "conv1", "conv2", "conv3", "conv4"]
            for s in ("weight", "bias")] + ["fusion_layer.weight", "fusion_layer.bias"]
    assert extra == sorted(want)
    assert tuple(f["pts_pointnet_encoder.conv4.weight"].shape) == (1024, 512, 1) and tuple(f["fusion_layer.weight"].shape) == (1024, 2048)
    assert all(float(f[k].abs().min()) > 0 for k in extra if k.endswith(".bias"))  # non-zero biases


def test_fused_agent_loads_on_the_host():
    from genpose_amd.config import get_config
    from genpose_amd.pointnet_encoder import PointNetEncoderHIP
    from genpose_amd.posenet_agent import PoseNet
    for mode in ("score", "energy"):
        agent = PoseNet(get_config(device="cpu", posenet_mode=mode, pts_encoder="pointnet_and_pointnet2"))
        agent.load_state_dict(make_state_dict(0, mode, pts_encoder="pointnet_and_pointnet2"))
        net = agent.net
        assert net.pts_encoder is None and isinstance(net.pts_pointnet_encoder, PointNetEncoderHIP)
        assert net.pts_pointnet_encoder.out_dim == 1024 and net.pts_pointnet2_encoder.out_dim == 1024
        assert tuple(net.fusion_layer[0].shape) == (1024, 2048)
        # packed on the host: four trunk convolutions in gp_pack_weight's size, fc3's bias carries the identity
        w = net.pts_pointnet_encoder.w
        assert [p.numel() for p, _ in w.convs] == [64 * 16, 128 * 64, 512 * 128, 1024 * 512]
        sd = make_state_dict(0, mode, pts_encoder="pointnet_and_pointnet2")
        torch.testing.assert_close(w.stn_fcs[2][1], sd["pts_pointnet_encoder.stn.fc3.bias"] + torch.eye(3).reshape(9), rtol=0, atol=0)
    # without a device the encoder raises like everything else; code that drives the PointNet++ stages itself gets a refusal that names the option
    if not torch.cuda.is_available():
        with pytest.raises(_lib.GenposeHipError):
            net.pts_pointnet_encoder.encode(torch.zeros(1, 4, 3))
    with pytest.raises(NotImplementedError, match="pointnet_and_pointnet2"):
        net.pointnet2_encoder("test")  # (what the pipeline predictors and the frame-graph runner call first)
    with pytest.raises(NotImplementedError, match="PointNetEncoderHIP"):
        PoseNet(get_config(device="cpu", pts_encoder="pointnet"))


def test_conv4_packing_round_trips(sd_pointnet):
    from genpose_amd.weights import PointNetWeights
    W = sd_pointnet["pts_encoder.conv4.weight"][:, :, 0]
    packed = PointNetWeights(sd_pointnet, "cpu").convs[3][0]
    NC = 1024 // 16
    assert packed.numel() == 1024 * 512
    # gp_common.h: Wp[((kg * NC + nc) * 64 + lane) * 4 + jj] = W[nc * 16 + (lane & 15)][kg * 16 + 4 * (lane >> 4) + jj]
    for nc, kg, lane, jj in ((0, 0, 0, 0), (63, 31, 63, 3), (17, 5, 38, 2), (40, 30, 15, 1), (1, 0, 16, 0)):
        assert float(packed[((kg * NC + nc) * 64 + lane) * 4 + jj]) == float(W[nc * 16 + (lane & 15), kg * 16 + 4 * (lane >> 4) + jj])


def test_new_entry_points_in_the_abi():
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    for name in ("gp_pointnet_stn_pool", "gp_pointnet_feat_pool", "gp_dense_rows"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, name
        assert len(_lib.SIGNATURES[name]) == len(m.group(1).split(",")), name
        assert hasattr(_lib.lib(), name)
