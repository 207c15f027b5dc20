"""Plain-torch reference of the vanilla PointNet encoder (csrc/pointnet.hip: gp_pointnet_stn_pool, gp_pointnet_feat_pool, gp_dense_rows) and
of the pointnet_and_pointnet2 agent's fused feature (helper of test_pointnet_reference_cpu.py and test_gpu_f64_pointnet.py; CPU only,
nothing here touches a device).

Every function runs in the dtype of the state dict it is given: the float64-cast state dict gives the TRUTH, the float32 one the
YARDSTICK (the reference's own rounding, f64_reference.py's rule: a device result passes at <= MARGIN x E_oracle).  The yardstick never
sees the code under test.  Points are rows ([B,n,3]); PointNetfeat without BatchNorm (networks/pts_encoder/pointnets.py:45-123).

    stn_pool(sd, pts)            relu(conv3(relu(conv2(relu(conv1(x)))))) of the transform net, max over the cloud     -> g [B,1024]
    stn_head(sd, g)              fc3(relu(fc2(relu(fc1(g))))) + identity                                                -> trans [B,3,3]
    feat_pool(sd, pts, trans)    conv4(relu(conv3(relu(conv2(relu(conv1(x . trans))))))), max over the cloud (signed)   -> [B,1024]
    pointnet(sd, pts)            -> (feat, trans)
    dense_rows(xa, W, bias, act, xb=None)   act([xa | xb] . W^T + bias)
    fused_feature(sd, pts)       relu(fusion_layer([pointnet | PointNet++])), the PointNet++ half on the fp32 oracle's grouping
                                 (f64_reference.encoder64 in float64, the oracle's own pass in float32)
    state_dict(which, mode)      'seed0' | 'seed1' | 'stress', the fused agent's layout;  integer_state_dict()  weights in {-1, 0, 1}

The case set, its clouds and the dense-rows cases are here too, with e_oracle(quantity): the yardstick of each quantity, computed once and
called by both test files."""
import functools
import math
import os

import numpy as np
import torch

import f64_reference as fr
from genpose_amd.weights_synth import make_state_dict
from oracle import genpose_oracle as go

PN = "pts_pointnet_encoder."
PN2 = "pts_pointnet2_encoder."
ACT_NONE, ACT_RELU = 0, 1
RELU_LAYERS = ("stn.conv1", "stn.conv2", "stn.conv3", "stn.fc1", "stn.fc2", "conv1", "conv2", "conv3")
LAYERS = RELU_LAYERS + ("stn.fc3", "conv4")

WEIGHTS = ("seed0", "seed1", "stress")
# one point; one below, at and above one and two tile boundaries (48 points per tile); 17 clouds = three row tiles of gp_dense_rows, the
# last ragged; 9 clouds of four tiles with one valid row in the last (and two row tiles of gp_dense_rows)
SHAPES = ((1, 1), (2, 47), (2, 48), (3, 49), (2, 96), (2, 97), (17, 49), (9, 145))
OFFSETS = (0.0, 0.5)
MASK_OFFSET = 0.5          # the clouds declared mask-exercising: a zero padding row beats the real points in MASK_SHARE of the channels
MASK_SHARE, NEGATIVE_SHARE = 0.20, 0.10
INTEGER_SHAPES = ((2, 47), (3, 49), (2, 97))
EXACT = float(2 ** 24)     # integers below this are fp32 numbers

# gp_dense_rows: (rows, k_a, k_b, n_out, act)
DENSE_CASES = ((1, 1024, 0, 512, ACT_RELU), (9, 512, 0, 256, ACT_RELU), (17, 256, 0, 9, ACT_NONE), (8, 4, 0, 1, ACT_NONE), (7, 260, 0, 5, ACT_RELU),
               (16, 256, 4, 18, ACT_RELU), (3, 1024, 1024, 1024, ACT_RELU), (25, 8, 8, 33, ACT_NONE))


# ----------------------------------------------------------------------------- the network, in the state dict's dtype
def _dtype(sd, prefix=PN):
    return sd[prefix + "conv1.weight"].dtype


def _lin(sd, name, x, prefix=PN):
    W = sd[prefix + name + ".weight"]
    return x @ W.reshape(W.shape[0], -1).T + sd[prefix + name + ".bias"]


def stn_rows(sd, pts, prefix=PN):
    """the transform net's per-point chain -> [B,n,1024] (after conv3's ReLU)"""
    x = pts.to(_dtype(sd, prefix))
    for name in ("stn.conv1", "stn.conv2", "stn.conv3"):
        x = torch.relu(_lin(sd, name, x, prefix))
    return x


def stn_pool(sd, pts, prefix=PN):
    return stn_rows(sd, pts, prefix).max(dim=1)[0]


def stn_head(sd, g, prefix=PN):
    h = torch.relu(_lin(sd, "stn.fc2", torch.relu(_lin(sd, "stn.fc1", g.to(_dtype(sd, prefix)), prefix)), prefix))
    return (_lin(sd, "stn.fc3", h, prefix) + torch.eye(3, dtype=h.dtype).reshape(9)).view(-1, 3, 3)


def trunk_rows(sd, pts, trans, prefix=PN):
    """the trunk's per-point chain on x . trans -> [B,n,1024] (conv4 has no ReLU: signed)"""
    dt = _dtype(sd, prefix)
    x = torch.bmm(pts.to(dt), trans.to(dt))
    for name in ("conv1", "conv2", "conv3"):
        x = torch.relu(_lin(sd, name, x, prefix))
    return _lin(sd, "conv4", x, prefix)


def feat_pool(sd, pts, trans, prefix=PN):
    return trunk_rows(sd, pts, trans, prefix).max(dim=1)[0]


def pointnet(sd, pts, prefix=PN):
    trans = stn_head(sd, stn_pool(sd, pts, prefix), prefix)
    return feat_pool(sd, pts, trans, prefix), trans


def dense_rows(xa, W, bias, act, xb=None):
    x = xa if xb is None else torch.cat([xa, xb], dim=1)
    y = x.to(W.dtype) @ W.T + bias
    return torch.relu(y) if act == ACT_RELU else y


def fused_feature(sd, pts):
    """posenet.py:85-88 of the pointnet_and_pointnet2 agent: relu(fusion_layer(cat(pointnet, pointnet2))).  The PointNet++ half: the fp32
    oracle's pass in float32; in float64 encoder64 on that pass's (integer) grouping - the float64 state dict is a cast of a float32 one,
    so casting it back is exact."""
    f1 = pointnet(sd, pts)[0]
    sd32 = {k: (v.float() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    f2, inter = go.encoder_forward(sd32, pts, prefix=PN2, return_intermediates=True)
    if f1.dtype == torch.float64:
        f2 = fr.encoder64(sd, pts, inter, prefix=PN2)[0]
    return dense_rows(f1, sd["fusion_layer.weight"], sd["fusion_layer.bias"], ACT_RELU, xb=f2)


# ----------------------------------------------------------------------------- weights
@functools.lru_cache(maxsize=None)
def state_dict(which, mode="score"):
    """float32 state dict of the fused agent (PointNet under PN, PointNet++ under PN2, fusion_layer): 'seed0' / 'seed1' seeded; 'stress' =
    seed 0 with 20 % of the ReLU layers' biases at -50 (dead channels), conv4.weight x 4 and stn.fc3.weight x 4.  Read-only."""
    if which != "stress":
        return make_state_dict(int(which[4:]), mode, pts_encoder="pointnet_and_pointnet2")
    g = torch.Generator().manual_seed(21 if mode == "score" else 22)
    sd = {k: v.clone() for k, v in state_dict("seed0", mode).items()}
    for name in RELU_LAYERS:
        b = sd[PN + name + ".bias"]
        sd[PN + name + ".bias"] = torch.where(torch.rand(b.shape, generator=g) < 0.2, torch.full_like(b, -50.0), b)
    for name in ("conv4", "stn.fc3"):
        sd[PN + name + ".weight"] = sd[PN + name + ".weight"] * 4.0
    return sd


@functools.lru_cache(maxsize=None)
def state_dict64(which, mode="score"):
    return fr.f64_state_dict(state_dict(which, mode))


@functools.lru_cache(maxsize=None)
def integer_state_dict():
    """float32, PointNet keys only: weights in {-1, 0, 1} with about 8 non-zeros per output channel (all three inputs for the 3-wide
    layers), integer biases in [-2, 2], stn.fc3 zero with bias zero (trans is the identity).  The density keeps the network small: on
    integer points in [-4, 4] no layer's sum of |w| |x| + |b| passes 1000 (integer_bound), so every partial sum, in any order, is an
    integer far below 2^24 - asserted in test_pointnet_reference_cpu.py."""
    g = torch.Generator().manual_seed(1848)
    sd = {}
    for name in LAYERS:
        shape = state_dict("seed0")[PN + name + ".weight"].shape
        cin = shape[1]
        W = torch.randint(-1, 2, shape, generator=g).float()
        if cin > 8:
            sign = torch.randint(0, 2, shape, generator=g).float() * 2 - 1
            W = torch.where(torch.rand(shape, generator=g) < 8.0 / cin, sign, torch.zeros_like(sign))
        sd[PN + name + ".weight"] = W
        sd[PN + name + ".bias"] = torch.randint(-2, 3, (shape[0],), generator=g).float()
    sd[PN + "stn.fc3.weight"].zero_()
    sd[PN + "stn.fc3.bias"].zero_()
    return sd


def integer_bound(sd, pts, prefix=PN):
    """max over the layers, rows and channels of sum_k |w_k| |x_k| + |b| (float64): below 2^24 every partial sum of every layer is exact
    in fp32 whatever the order of summation"""
    sd64 = fr.f64_state_dict(sd)
    worst = 0.0

    def chain(x, names, relu_last):
        nonlocal worst
        for i, name in enumerate(names):
            W = sd64[prefix + name + ".weight"]
            W = W.reshape(W.shape[0], -1)
            worst = max(worst, float((x.abs() @ W.abs().T + sd64[prefix + name + ".bias"].abs()).max()))
            x = x @ W.T + sd64[prefix + name + ".bias"]
            if relu_last or i + 1 < len(names):
                x = torch.relu(x)
        return x

    x = pts.double()
    g = chain(x, ("stn.conv1", "stn.conv2", "stn.conv3"), True).max(dim=1)[0]
    t = chain(g, ("stn.fc1", "stn.fc2", "stn.fc3"), False).view(-1, 3, 3) + torch.eye(3, dtype=torch.float64)
    chain(torch.bmm(x, t), ("conv1", "conv2", "conv3", "conv4"), False)
    return worst


# ----------------------------------------------------------------------------- inputs
@functools.lru_cache(maxsize=None)
def clouds(B, n, offset):
    """[B,n,3] float32, randn * 0.1 + offset (the encoder's input is in the camera frame: not centred).  Read-only."""
    g = torch.Generator().manual_seed(900000 + 1000 * B + n + (500000 if offset else 0))
    return torch.randn(B, n, 3, generator=g) * 0.1 + offset


@functools.lru_cache(maxsize=None)
def integer_clouds(B, n):
    g = torch.Generator().manual_seed(770000 + 1000 * B + n)
    return torch.randint(-4, 5, (B, n, 3), generator=g).float()


@functools.lru_cache(maxsize=None)
def dense_inputs(i, integer=False):
    """case i of DENSE_CASES -> (xa, xb or None, W, bias) float32: randn inputs, weights randn * sqrt(2 / K); or integers in [-4, 4]
    (K <= 2048: every partial sum is an integer below 2048 * 16 + 4)"""
    rows, ka, kb, n_out, _ = DENSE_CASES[i]
    g = torch.Generator().manual_seed(310000 + i + (1000 if integer else 0))
    if integer:
        draw = lambda *s: torch.randint(-4, 5, s, generator=g).float()
        xa, xb, W, b = draw(rows, ka), (draw(rows, kb) if kb else None), draw(n_out, ka + kb), draw(n_out)
    else:
        draw = lambda *s: torch.randn(*s, generator=g)
        xa, xb, W, b = draw(rows, ka), (draw(rows, kb) if kb else None), draw(n_out, ka + kb) * math.sqrt(2.0 / (ka + kb)), 0.1 * draw(n_out)
    return xa, xb, W, b


def dense_reference(i, dtype, integer=False):
    xa, xb, W, b = dense_inputs(i, integer)
    return dense_rows(xa.to(dtype), W.to(dtype), b.to(dtype), DENSE_CASES[i][4], None if xb is None else xb.to(dtype))


# ----------------------------------------------------------------------------- cases and the yardstick
def cloud_error(got, ref64):
    """fr.block_error of the whole vector, per cloud (row), the worst cloud: a cloud of small features does not hide behind a large one"""
    return max(fr.block_error(got[b:b + 1].reshape(1, -1), ref64[b:b + 1].reshape(1, -1), None)[0] for b in range(ref64.shape[0]))


@functools.lru_cache(maxsize=None)
def case(which, B, n, offset):
    """One case on the host, computed once and read-only: pts; g / trans / feat in float32 (the yardstick) and float64 (the truth), end to
    end; feat_gt64 = the float64 trunk GIVEN the float32 reference's trans (what gp_pointnet_feat_pool is fed in the direct test - the
    float32 trunk on that trans is feat32 itself)."""
    sd32, sd64, pts = state_dict(which), state_dict64(which), clouds(B, n, offset)
    g32, g64 = stn_pool(sd32, pts), stn_pool(sd64, pts)
    trans32, trans64 = stn_head(sd32, g32), stn_head(sd64, g64)
    return dict(pts=pts, g32=g32, g64=g64, trans32=trans32, trans64=trans64, feat32=feat_pool(sd32, pts, trans32),
                feat_gt64=feat_pool(sd64, pts, trans32), feat64=feat_pool(sd64, pts, trans64))


def oracle_errors(which, B, n, offset):
    c = case(which, B, n, offset)
    return {"g": cloud_error(c["g32"], c["g64"]), "trans": cloud_error(c["trans32"], c["trans64"]),
            "feat_given_trans": cloud_error(c["feat32"], c["feat_gt64"]), "feat": cloud_error(c["feat32"], c["feat64"])}


def case_set():
    return [(w, B, n, o) for w in WEIGHTS for B, n in SHAPES for o in OFFSETS]


@functools.lru_cache(maxsize=None)
def fused_case(mode):
    """the fixture's clouds_3x1024 through the fused agent's feature, seed-0 weights of `mode`: float32 and float64"""
    pts = torch.from_numpy(np.load(os.path.join(fr.HERE, "golden", "g18_pointnet.npz"))["clouds_3x1024"])
    return dict(pts=pts, f32=fused_feature(state_dict("seed0", mode), pts), f64=fused_feature(state_dict64("seed0", mode), pts))


@functools.lru_cache(maxsize=None)
def e_oracle(quantity):
    """THE yardstick of a quantity: the fp32 reference's own error against float64, maximised over the whole case set ('g', 'trans',
    'feat_given_trans', 'feat'), over DENSE_CASES ('dense') or over the two agents ('fused')."""
    if quantity == "dense":
        return max(dense_oracle_errors())
    if quantity == "fused":
        return max(cloud_error(fused_case(m)["f32"], fused_case(m)["f64"]) for m in ("score", "energy"))
    return max(oracle_errors(*c)[quantity] for c in case_set())


@functools.lru_cache(maxsize=None)
def dense_oracle_errors():
    return tuple(fr.block_error(dense_reference(i, torch.float32), dense_reference(i, torch.float64), None)[0] for i in range(len(DENSE_CASES)))
