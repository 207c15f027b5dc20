"""float64 ground truth for the fp32 score, energy and encoder kernels (helper of test_f64_reference_cpu.py, test_gpu_f64_score.py and
test_gpu_f64_encoder.py; CPU only, nothing here touches a device).

    f64_state_dict      the state dict cast to float64
    score64 / energy64 / energy_score64 / divergence64 / embed64
                        oracle.genpose_oracle's own functions on the float64 state dict and float64 inputs
    evaluate(sd, q, ...)  one of those quantities in the state dict's own dtype - float64 for the truth, float32 for the yardstick
    block_error         max |got - ref| / max |ref| per block (the three heads of a 9-column output, each column of the 2-column energy,
                        the whole vector otherwise): a small head does not hide behind a large one
    oracle_error        block_error of the fp32 CPU oracle on the same inputs - the reference's OWN rounding, the yardstick of the GPU
                        tests.  It never sees the code under test.
    kink_free           rows whose derivative quantity is stable under a 1e-6 relative move of x (test_gpu_exact_likelihood.py's criterion)
    encoder64           the PointNet++ encoder in float64 on the fp32 oracle's (integer, feature-independent) FPS and ball-query indices,
                        every SharedMLP from the UNFOLDED state dict - so a fold of BatchNorm into the weights is part of what is tested

The GPU rule (tests/test_gpu_f64_score.py): per (model, quantity, block, t) E_oracle = max of oracle_error over the shape set, the pose
scales and the weight sets (e_oracle_cell); a device result passes when its block_error <= MARGIN * E_oracle.  MARGIN = 3 is the allowance for two fp32 evaluations that
round only in their accumulations but in different orders (MFMA k-blocks of 4 in a fixed chain against oneDNN's blocked sums); it was
fixed before any kernel was measured against it.  ORACLE_CEILING is a condition on the reference alone."""
import functools
import os

import numpy as np
import torch

from oracle import genpose_oracle as go

HERE = os.path.dirname(os.path.abspath(__file__))
P = "pose_score_net."
HEADS = ("rot_x", "rot_y", "trans")

MARGIN = 3.0             # device error <= MARGIN x the fp32 oracle's own error
MARGIN_CAP = 8.0         # a named per-plan exception is gated at the next power of two and never above this: beyond, the split-bf16 class
ORACLE_CEILING = 5e-6    # the fp32 oracle's own error stays under this in every cell (measured on the host: worst 2.1e-6)
AGREE = 1e-5             # float64 functions against the fp32 oracle, of the scale
KINK_MOVE, KINK_TOL, KINK_SHARE = 1e-6, 1e-3, 0.05
CANCEL_LIMIT = 2.5       # the energies' inner products cancel by at most this on every case (the multi-row cases reach 2.4 by themselves)

SHAPES = [(1, 1), (3, 7), (2, 43), (3, 50)]  # one row; a tile spanning clouds; 86 rows; 150 rows = a full 128-row workgroup + a ragged one
POSE_SCALES = (1.0, 50.0)
TIMES = (1e-5, 1e-3, 0.15, 0.55, 1.0)
WEIGHTS = ("seed0", "seed1", "stress", "trained")
BLOCKS9 = ((0, 3), (3, 6), (6, 9))
# The draw of each (B, K, pose scale): the FIRST seed 0, 1, 2, ... whose inputs meet three conditions on the REFERENCE alone, all asserted in
# test_f64_reference_cpu.py: (a) cancellation <= CANCEL_LIMIT in every energy block, (b) at most KINK_SHARE of a case's rows near a kink,
# (c) the fp32 oracle's own error under SEED_HEADROOM x ORACLE_CEILING in every cell (the headroom is for another host's fp32 rounding).
# They bind on the small shapes only: the metric of a one-row case is the relative error of ONE energy, an inner product that cancels by
# 12x to 500x on the first draws (the oracle itself is then off by up to 1e-4), and one or two kink rows of 21 are over the cap.  No
# kernel entered this choice; a draw chosen by (c) alone would be one on which the oracle was lucky, which is why (a) is there.
SEED_HEADROOM = 0.8
INPUT_SEEDS = {(1, 1, 1.0): 120, (1, 1, 50.0): 68, (3, 7, 1.0): 1, (3, 7, 50.0): 0, (2, 43, 1.0): 0, (2, 43, 50.0): 0, (3, 50, 1.0): 0, (3, 50, 50.0): 0}
MODEL_OF = {"score": "score", "sdiv": "score", "embed": "score", "energy": "energy", "escore": "energy"}  # quantity -> whose weights it runs on


def f64_state_dict(sd):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def state_dict(which, model):
    """float32 state dict: 'seed0' / 'seed1' (seeded), 'stress' (test_gpu_weight_seeds._stress of seed 0), 'trained' (tests/golden/trained)"""
    if which == "trained":
        sd = torch.load(os.path.join(HERE, "golden", "trained", f"ckpt_{model}.pth"), map_location="cpu")["model_state_dict"]
        return {k: (v.float() if torch.is_floating_point(v) else v) for k, v in sd.items()}
    if which == "stress":
        from test_gpu_weight_seeds import _stress
        return _stress(go.make_state_dict(0, model), 11 if model == "score" else 12)
    return go.make_state_dict(int(which[4:]), model)


@functools.lru_cache(maxsize=None)
def state_dict64(which, model):
    return f64_state_dict(state_dict(which, model))


@functools.lru_cache(maxsize=None)
def inputs(B, K, scale):
    """features [B,1024], poses [B K,9] at the pose scale, probe [B K,9], centres [B,3]: float32, read-only"""
    g = torch.Generator().manual_seed(100000 * INPUT_SEEDS[B, K, scale] + 1000 * B + 10 * K + int(scale))
    feat = torch.randn(B, 1024, generator=g).abs()
    pose = torch.randn(B * K, 9, generator=g) * scale
    probe = torch.randn(B * K, 9, generator=g)
    centre = torch.randn(B, 3, generator=g) * 0.3
    return feat, pose, probe, centre


# ----------------------------------------------------------------------------- the network's quantities, in the state dict's dtype
def _t(R, t, dtype):
    # (the time is the fp32 value the kernels are given, in either precision)
    return torch.full((R, 1), float(np.float32(t)), dtype=dtype)


def embed_time(sd, t):
    """relu(t_encoder.1([sin, cos](2 pi W t))) -> [1,128]"""
    tt = _t(1, t, sd[P + "t_encoder.0.W"].dtype)[:, 0]
    xp = tt[:, None] * sd[P + "t_encoder.0.W"][None, :] * 2 * np.pi
    return torch.relu(go._lin(sd, P + "t_encoder.1", torch.cat([torch.sin(xp), torch.cos(xp)], dim=-1)))


def embed(sd, feat, t):
    """What the rows consume of the heads' first layer besides the pose: W[:, :1152] . [pts_feat; relu(t_encoder.1(sin, cos))] + b of the
    three stacked head layers -> [B,768] (the device's cvec[cloud] + tvec, wherever it keeps the biases)."""
    dtype = sd[P + "t_encoder.0.W"].dtype
    tf = embed_time(sd, t)
    W = torch.cat([sd[f"{P}fusion_tail_{h}.0.weight"] for h in HEADS], 0)
    b = torch.cat([sd[f"{P}fusion_tail_{h}.0.bias"] for h in HEADS], 0)
    return torch.cat([feat.to(dtype), tf.expand(feat.shape[0], -1)], dim=-1) @ W[:, :1152].T + b


def evaluate(sd, quantity, feat, K, pose, t, probe=None):
    """-> tensor or tuple of tensors in sd's dtype.  quantity: 'score' [R,9] | 'energy' [R,2] | 'escore' ([R,9], [R]) the energy model's
    score and energy | 'sdiv' ([R,9], [R]) score and e^T J e | 'embed' [B,768]"""
    dtype = sd[P + "t_encoder.0.W"].dtype
    if quantity == "embed":
        return embed(sd, feat, t)
    fr, x, tt = feat.repeat_interleave(K, 0).to(dtype), pose.to(dtype), _t(pose.shape[0], t, dtype)
    if quantity == "score":
        return go.score_forward(sd, fr, x, tt)
    if quantity == "energy":
        return go.energy_forward(sd, fr, x, tt)
    if quantity == "escore":
        return go.energy_score(sd, fr, x, tt)
    if quantity == "sdiv":
        return go.score_and_divergence(sd, fr, x, tt, probe.to(dtype))
    raise ValueError(quantity)


def score64(sd64, feat, K, pose, t):
    return evaluate(sd64, "score", feat, K, pose, t)


def energy64(sd64, feat, K, pose, t):
    return evaluate(sd64, "energy", feat, K, pose, t)


def energy_score64(sd64, feat, K, pose, t):
    return evaluate(sd64, "escore", feat, K, pose, t)


def divergence64(sd64, feat, K, pose, t, probe):
    return evaluate(sd64, "sdiv", feat, K, pose, t, probe)


def embed64(sd64, feat, t):
    return embed(sd64, feat, t)


def blocks_of(ref):
    if ref.ndim == 2 and ref.shape[1] == 9:
        return BLOCKS9
    if ref.ndim == 2 and ref.shape[1] == 2:
        return ((0, 1), (1, 2))
    if ref.ndim == 2 and ref.shape[1] == 768:
        return ((0, 256), (256, 512), (512, 768))
    return None


def block_error(got, ref64, blocks="auto", rows=None):
    """max |got - ref| / max |ref| per block -> list of floats.  blocks: column ranges, None (the whole array) or 'auto' (blocks_of)."""
    got, ref = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref64).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    if ref.shape[0] == 0:  # (every row left out: nothing to compare - the caller's cap on the share of such rows is what fails)
        return [0.0] * (1 if blocks is None or (isinstance(blocks, str) and blocks_of(ref) is None) else len(blocks_of(ref) if isinstance(blocks, str) else blocks))
    if isinstance(blocks, str):
        blocks = blocks_of(ref)
    if blocks is None:
        return [float((got - ref).abs().max()) / float(ref.abs().max())]
    return [float((got[..., a:b] - ref[..., a:b]).abs().max()) / float(ref[..., a:b].abs().max()) for a, b in blocks]


def near_kink(sd64, feat, K, pose, t):
    """Rows [R] bool with a ReLU on the path from x (pose_encoder.0, pose_encoder.2, the heads' first layers) whose float64 pre-activation
    z = w . a + b lies within KINK_MOVE of zero relative to |w| . |a| + |b|, the scale at which an fp32 dot product rounds (1e-6 is ~17
    units in the last place): an fp32 evaluation, the CPU oracle's as much as a kernel's, may take the other side of that kink, which
    moves a derivative by the unit's whole share (1/256 of a head) while the forward value does not notice."""
    g = lambda k: sd64[P + k]
    x, fr = pose.double(), feat.repeat_interleave(K, 0).double()
    tf = embed_time(sd64, t).expand(x.shape[0], -1)
    Wa = torch.cat([g(f"fusion_tail_{h}.0.weight") for h in HEADS], 0)
    ba = torch.cat([g(f"fusion_tail_{h}.0.bias") for h in HEADS], 0)
    near = torch.zeros(x.shape[0], dtype=torch.bool)
    a = x
    for W, b in ((g("pose_encoder.0.weight"), g("pose_encoder.0.bias")), (g("pose_encoder.2.weight"), g("pose_encoder.2.bias")), (Wa, ba)):
        if W is Wa:
            a = torch.cat([fr, tf, a], dim=-1)
        z, s = a @ W.T + b, a.abs() @ W.abs().T + b.abs()
        near |= (z.abs() <= KINK_MOVE * s).any(dim=1)
        a = torch.relu(z)
    return near


def kink_free(sd64, quantity, feat, K, pose, t, probe=None):
    """Rows [R] bool kept for a derivative quantity (the divergence of 'sdiv', the score of 'escore'): it moves by at most KINK_TOL relative
    under a KINK_MOVE relative move of x (test_gpu_exact_likelihood.py's criterion), and no pre-activation is near_kink.  The second
    condition is needed because the first moves only the pose's share of a head's pre-activation, which at pose scale 1 is a small part of
    it: without it the fp32 CPU ORACLE is off by 4e-3 to 1e-2 of the scale on single rows of these draws."""
    a = evaluate(sd64, quantity, feat, K, pose, t, probe)
    b = evaluate(sd64, quantity, feat, K, pose.double() * (1 + KINK_MOVE), t, probe)
    a, b = (a[1], b[1]) if quantity == "sdiv" else (a[0], b[0])
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    return ((b - a).abs().max(dim=1)[0] <= KINK_TOL * a.abs().max(dim=1)[0]) & ~near_kink(sd64, feat, K, pose, t)


def cancellation(which, B, K, scale, t):
    """How much the energy model's inner products <x, s> cancel on a case's rows, per energy block (rotation, translation, all nine):
    max_rows sum |x_i s_i| / max_rows |sum x_i s_i| in float64.  The block metric divides by the second, an error of s enters with the
    first: a one-row case whose inner product cancels measures that cancellation, not an evaluation."""
    sd, (feat, pose, _, _) = state_dict64(which, "energy"), inputs(B, K, scale)
    x = pose.double()
    s = go._trunk(sd, feat.repeat_interleave(K, 0).double(), x, _t(x.shape[0], t, torch.float64))
    return [float((x[:, a:b] * s[:, a:b]).abs().sum(1).max() / (x[:, a:b] * s[:, a:b]).sum(1).abs().max()) for a, b in ((0, 6), (6, 9), (0, 9))]


@functools.lru_cache(maxsize=None)
def case(which, quantity, B, K, scale, t):
    """One cell's inputs on the host, computed once and read-only: -> dict(ref: float64 truth (tuple for 'escore' / 'sdiv'), f32: the fp32
    oracle's result, keep: kink-free rows or None)."""
    model = MODEL_OF[quantity]
    feat, pose, probe, _ = inputs(B, K, scale)
    sd32, sd64 = state_dict(which, model), state_dict64(which, model)
    ref = evaluate(sd64, quantity, feat, K, pose, t, probe)
    f32 = evaluate(sd32, quantity, feat, K, pose, t, probe)
    keep = kink_free(sd64, quantity, feat, K, pose, t, probe) if quantity in ("escore", "sdiv") else None
    return dict(ref=ref, f32=f32, keep=keep)


def errors(got, c, quantity):
    """{name: [block errors]} of `got` (same structure as the case's reference; a None member is left out) against the case's float64
    truth, kink rows left out"""
    if quantity in ("escore", "sdiv"):
        names = ("escore", "eenergy") if quantity == "escore" else ("sdiv_score", "sdiv_div")
        # (the kink criterion covers the derivative; the plain forward outputs - sdiv's score, escore's energy - keep every row)
        rows = (c["keep"], None) if quantity == "escore" else (None, c["keep"])
        return {n: block_error(g, r, rows=rw) for n, g, r, rw in zip(names, got, c["ref"], rows) if g is not None}
    return {quantity: block_error(got, c["ref"])}


def oracle_error(which, quantity, B, K, scale, t):
    """the fp32 CPU oracle's own block errors on the case's inputs"""
    c = case(which, quantity, B, K, scale, t)
    return errors(c["f32"], c, quantity)


@functools.lru_cache(maxsize=None)
def e_oracle(which, quantity, t, shapes=tuple(SHAPES), scales=POSE_SCALES):
    """{name: [per block: max of oracle_error over the shapes and pose scales]} - the yardstick of one (weights, quantity, t)"""
    out = {}
    for B, K in shapes:
        for sc in (scales if quantity != "embed" else scales[:1]):
            for n, e in oracle_error(which, quantity, B, K, sc, t).items():
                out[n] = [max(a, b) for a, b in zip(out.get(n, [0.0] * len(e)), e)]
    return out


@functools.lru_cache(maxsize=None)
def e_oracle_cell(quantity, t):
    """THE yardstick of a (model, quantity, block, t) cell: {name: [per block: max of oracle_error over the shape set, the pose scales and
    the weights]} (a quantity runs on one model's weights: MODEL_OF)"""
    out = {}
    for which in WEIGHTS:
        for n, e in e_oracle(which, quantity, t).items():
            out[n] = [max(a, b) for a, b in zip(out.get(n, [0.0] * len(e)), e)]
    return out


# ----------------------------------------------------------------------------- encoder
def encoder64(sd64, pts, inter, cfg=go.LIGHT_CFG, prefix="pts_encoder."):
    """The encoder in float64 on the grouping the fp32 oracle made: pts [B,N,3] fp32 clouds, inter = encoder_forward(...,
    return_intermediates=True)[1] (fps_idx, bq_idx*: integer results that no feature enters).  Conv, eval-mode BatchNorm, ReLU and max of
    every SharedMLP from the unfolded float64 state dict.  -> (out [B,C] float64, [level features [B,C,n] float64])"""
    xyz = pts[..., 0:3].double()
    B = xyz.shape[0]
    bi = torch.arange(B)[:, None, None]
    feats, levels = None, []
    for k, npoint in enumerate(cfg["npoints"]):
        outs = []
        if npoint is not None:
            new_xyz = xyz[bi[:, :, 0], torch.from_numpy(inter[k]["fps_idx"]).long()]  # [B,np,3]
            assert np.array_equal(new_xyz.float().numpy(), inter[k]["new_xyz"])
        for i in range(len(cfg["radii"][k])):
            if npoint is not None:
                idx = torch.from_numpy(inter[k][f"bq_idx{i}"]).long()                # [B,np,ns]
                g = (xyz[bi, idx] - new_xyz[:, :, None, :]).permute(0, 3, 1, 2)       # [B,3,np,ns]
                if feats is not None:
                    g = torch.cat([g, feats.transpose(1, 2)[bi, idx].permute(0, 3, 1, 2)], dim=1)
            else:
                g = xyz.transpose(1, 2).unsqueeze(2)
                if feats is not None:
                    g = torch.cat([g, feats.unsqueeze(2)], dim=1)
            outs.append(go._shared_mlp(sd64, f"{prefix}SA_modules.{k}.mlps.{i}.", g).max(dim=3)[0])
        feats = torch.cat(outs, dim=1)
        if npoint is not None:
            xyz = new_xyz
        levels.append(feats)
    return feats.squeeze(-1), levels


def level_blocks(cfg, k):
    """column blocks of level k's features: level 0 per scale (16-16-32 | 32-32-64: the narrow scale must not hide), later levels whole"""
    if k > 0:
        return None
    edges = np.cumsum([0] + [m[-1] for m in cfg["mlps"][k]])
    return tuple((int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]))


def encoder_errors(levels_got, levels_ref, cfg=go.LIGHT_CFG):
    """[level][cloud] -> block errors; levels_* are lists of [B,C,n] arrays"""
    out = []
    for k, (g, r) in enumerate(zip(levels_got, levels_ref)):
        g, r = torch.as_tensor(g).double(), torch.as_tensor(r).double()
        out.append([block_error(g[b].T, r[b].T, level_blocks(cfg, k)) for b in range(r.shape[0])])
    return out


ENCODER_WEIGHTS = ("seed0", "stress", "trained")


@functools.lru_cache(maxsize=None)
def encoder_clouds():
    """[4,1024,3] fp32: synth.make_batch(3, start=4321) and the tiled-duplicates cloud of the split-bf16 level tests (cloud 4 of
    make_batch(5, start=4321), its first 64 points repeated: every neighbourhood is full of repeated points)"""
    from genpose_amd import synth
    five = torch.from_numpy(synth.make_batch(5, start=4321)).float()
    tiled = five[4, :64].repeat(five.shape[1] // 64, 1)
    return torch.cat([five[:3], tiled[None]], dim=0).contiguous()


@functools.lru_cache(maxsize=None)
def encoder_case(which, params="light", nclouds=4):
    """The encoder's host side, computed once and read-only: the fp32 oracle's pass (out, inter), the float64 encoder on its grouping
    (out64, levels64) and the yardstick - e_levels[k] = per block the max over the clouds of the oracle's own error at level k, e_out the
    same for the 1024 features."""
    from genpose_amd.weights import ENCODER_CFGS
    cfg = ENCODER_CFGS[params]
    sd = state_dict(which, "score") if params == "light" else go.make_state_dict(int(which[4:]), "score", params)
    pts = encoder_clouds()[:nclouds]
    out, inter = go.encoder_forward(sd, pts, cfg=cfg, return_intermediates=True)
    out64, levels64 = encoder64(f64_state_dict(sd), pts, inter, cfg=cfg)
    per_cloud = encoder_errors([r["features"] for r in inter], levels64, cfg)
    e_levels = [[max(c[j] for c in lv) for j in range(len(lv[0]))] for lv in per_cloud]
    e_out = max(block_error(out[b:b + 1], out64[b:b + 1], None)[0] for b in range(pts.shape[0]))
    return dict(sd=sd, cfg=cfg, pts=pts, out=out, inter=inter, out64=out64, levels64=levels64, e_levels=e_levels, e_out=e_out)
