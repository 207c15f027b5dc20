"""Seeded random weights under the reference's state-dict key names and shapes - stands in for
`ckpt_genpose.pth`, which is not reachable offline.  Output layers (zero-initialised by the reference,
scorenet.py:156-170) are drawn N(0, 0.05) so the score is not identically zero, and BatchNorm statistics are
randomised so BN folding is exercised.  Pure torch-CPU; shared by bench.py, the smoke test, the oracle and the golden
generator so that every party sees identical bytes."""
import math

import torch

# networks/pts_encoder/pointnet2.py:57-66 (ClsMSG_CFG_Light), input_channels = 0
LIGHT_MLPS = [[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]],
              [[256, 256, 512], [256, 384, 512]]]


def mlp_specs(mlps=LIGHT_MLPS, input_channels=0):
    """[(level, scale, [Cin+3, c1, c2, c3])] as built by pointnet2.py:173-190 + pointnet2_modules.py:88-90."""
    out = []
    cin = input_channels
    for k, level in enumerate(mlps):
        cout = 0
        for i, m in enumerate(level):
            out.append((k, i, [cin + 3] + list(m)))
            cout += m[-1]
        cin = cout
    return out


def make_state_dict(seed=0, mode="score", params="light", pts_encoder="pointnet2"):
    """Random weights with the reference's shapes and key names; output layers (zero-initialised by the
    reference, scorenet.py:156-170) re-drawn N(0,0.05), BN statistics randomised so BN folding is exercised.
    params: the encoder configuration (--pointnet2_params: 'light' | 'dense' | 'lighter', pointnet2.py:47-78).
    pts_encoder (--pts_encoder, networks/posenet.py:36-46): 'pointnet' puts PointNetfeat's keys under `pts_encoder.` in place of the
    PointNet++ ones; 'pointnet_and_pointnet2' the reference's fused layout - PointNet++ under
    `pts_pointnet2_encoder.`, PointNetfeat under `pts_pointnet_encoder.`, and `fusion_layer.{weight,bias}` [1024, 2048]."""
    g = torch.Generator().manual_seed(seed + (0 if mode == "score" else 7919))
    sd = {}

    def rn(*shape, std=1.0):
        return torch.randn(*shape, generator=g) * std

    if params == "light":
        mlps = LIGHT_MLPS
    else:
        from .weights import ENCODER_CFGS
        mlps = ENCODER_CFGS[params]["mlps"]
    for (k, i, spec) in mlp_specs(mlps):
        for l in range(3):
            cin, cout = spec[l], spec[l + 1]
            p = f"pts_encoder.SA_modules.{k}.mlps.{i}.layer{l}."
            sd[p + "conv.weight"] = rn(cout, cin, 1, 1, std=math.sqrt(2.0 / cin))
            sd[p + "bn.bn.weight"] = 1.0 + 0.1 * rn(cout)
            sd[p + "bn.bn.bias"] = 0.1 * rn(cout)
            sd[p + "bn.bn.running_mean"] = 0.1 * rn(cout)
            sd[p + "bn.bn.running_var"] = (1.0 + 0.1 * rn(cout)).abs() + 0.05
            sd[p + "bn.bn.num_batches_tracked"] = torch.tensor(100)
    q = "pose_score_net."

    def lin(name, cin, cout, std=None):
        std = 1.0 / math.sqrt(cin) if std is None else std
        sd[q + name + ".weight"] = rn(cout, cin, std=std)
        sd[q + name + ".bias"] = rn(cout, std=std)

    lin("pose_encoder.0", 9, 256)
    lin("pose_encoder.2", 256, 256)
    sd[q + "t_encoder.0.W"] = rn(64, std=30.0)
    lin("t_encoder.1", 128, 128)
    for h in ("rot_x", "rot_y", "trans"):
        lin(f"fusion_tail_{h}.0", 1408, 256)
        lin(f"fusion_tail_{h}.2", 256, 3, std=0.05)
    if pts_encoder == "pointnet2":
        return sd
    if pts_encoder not in ("pointnet", "pointnet_and_pointnet2"):
        raise ValueError(f"pts_encoder {pts_encoder!r}: 'pointnet2', 'pointnet' or 'pointnet_and_pointnet2'")
    # the extra tensors come from a SECOND generator, after every draw above: the default call returns the bytes it always returned
    g2 = torch.Generator().manual_seed(104729 + seed + (0 if mode == "score" else 7919))

    def rn2(*shape, std=1.0):
        return torch.randn(*shape, generator=g2) * std

    fused = pts_encoder == "pointnet_and_pointnet2"
    if fused:  # networks/posenet.py:40-43: the PointNet++ encoder under its second name
        sd = {("pts_pointnet2_encoder." + k[len("pts_encoder."):] if k.startswith("pts_encoder.") else k): v for k, v in sd.items()}
    else:  # PointNetfeat alone owns `pts_encoder.`
        sd = {k: v for k, v in sd.items() if not k.startswith("pts_encoder.")}
    p = "pts_pointnet_encoder." if fused else "pts_encoder."
    # PointNetfeat (networks/pts_encoder/pointnets.py:45-56, 83-94): non-zero biases throughout
    for name, cin, cout in (("stn.conv1", 3, 64), ("stn.conv2", 64, 128), ("stn.conv3", 128, 1024), ("conv1", 3, 64), ("conv2", 64, 128),
                            ("conv3", 128, 512), ("conv4", 512, 1024)):
        sd[p + name + ".weight"] = rn2(cout, cin, 1, std=math.sqrt(2.0 / cin))
        sd[p + name + ".bias"] = 0.1 * rn2(cout)
    for name, cin, cout in (("stn.fc1", 1024, 512), ("stn.fc2", 512, 256)):
        sd[p + name + ".weight"] = rn2(cout, cin, std=math.sqrt(2.0 / cin))
        sd[p + name + ".bias"] = 0.1 * rn2(cout)
    # fc3 wide enough that trans is visibly NOT the identity (entries of order 0.3): an almost-identity transform hides a transposed bmm
    sd[p + "stn.fc3.weight"] = rn2(9, 256, std=0.02)
    sd[p + "stn.fc3.bias"] = 0.3 * rn2(9)
    if fused:
        sd["fusion_layer.weight"] = rn2(1024, 2048, std=math.sqrt(2.0 / 2048))
        sd["fusion_layer.bias"] = 0.1 * rn2(1024)
    return sd
