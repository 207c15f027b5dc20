"""State-dict -> device weight blocks for the HIP kernels.

Accepts exactly the reference's `model_state_dict` key schema (posenet_agent.py:143-173):
  pts_encoder.SA_modules.{k}.mlps.{i}.layer{l}.conv.weight [Cout,Cin,1,1], ....bn.bn.{weight,bias,running_mean,running_var}
  pose_score_net.{pose_encoder.{0,2}, t_encoder.0.W, t_encoder.1, fusion_tail_{rot_x,rot_y,trans}.{0,2}}.{weight,bias}
so a real `ckpt_genpose.pth` drops in; for cfg.pts_encoder = 'pointnet_and_pointnet2' (posenet.py:40-44) the same PointNet++ keys under
`pts_pointnet2_encoder.`, PointNetfeat's under `pts_pointnet_encoder.` (PointNetWeights) and `fusion_layer.{weight,bias}`.  Host-side work here is layout only: BatchNorm (eval) folding into the
1x1 conv, input-channel permutation [dx,dy,dz,feat] -> [feat,dx,dy,dz], and the MFMA
fragment packing of gp_pack_weight (include/genpose_hip.h).
"""
import ctypes

import torch

from . import _lib

# networks/pts_encoder/pointnet2.py:24-78 (input_channels = 0, use_xyz=True)
ENCODER_CFGS = {
    "light": dict(npoints=[512, 256, 128, None], radii=[[0.02, 0.04], [0.04, 0.08], [0.08, 0.16], [None, None]],
                  nsamples=[[16, 32], [16, 32], [16, 32], [None, None]],
                  mlps=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]],
                        [[256, 256, 512], [256, 384, 512]]]),
    "dense": dict(npoints=[512, 256, 128, None], radii=[[0.02, 0.04], [0.04, 0.08], [0.08, 0.16], [None, None]],
                  nsamples=[[32, 64], [16, 32], [8, 16], [None, None]],
                  mlps=[[[16, 16, 32], [32, 32, 64]], [[64, 64, 128], [64, 96, 128]], [[128, 196, 256], [128, 196, 256]],
                        [[256, 256, 512], [256, 384, 512]]]),
    "lighter": dict(npoints=[512, 256, 128, 64, None], radii=[[0.01], [0.02], [0.04], [0.08], [None]],
                    nsamples=[[64], [32], [16], [8], [None]],
                    mlps=[[[32, 32, 64]], [[64, 64, 128]], [[128, 196, 256]], [[256, 256, 512]], [[512, 512, 1024]]]),
}
BN_EPS = 1e-5


def _round16(v):
    return (v + 15) // 16 * 16


def pack_weight(W):
    """W [n_out, k_in] (CPU f32) -> packed MFMA A-operand stream (CPU f32), see gp_common.h."""
    W = W.detach().to(torch.float32).contiguous().cpu()
    n, k = W.shape
    size = _lib.lib().gp_pack_weight_size(n, k)
    out = torch.empty(size, dtype=torch.float32)
    _lib.call("gp_pack_weight", n, k, ctypes.c_void_p(W.data_ptr()), k, ctypes.c_void_p(out.data_ptr()))
    return out


def pad_bias(b):
    b = b.detach().to(torch.float32).cpu()
    out = torch.zeros(_round16(b.numel()), dtype=torch.float32)
    out[: b.numel()] = b
    return out


class SAScale:
    """One (level, scale) of the encoder: three folded layers."""

    def __init__(self, sd, prefix, cin_feat, device):
        self.cin = cin_feat
        self.layers = []
        self.couts = []
        self.hidden_layout = 0  # GP_SA_TAIL_PLAIN
        folded = []
        l = 0
        while f"{prefix}layer{l}.conv.weight" in sd:
            p = f"{prefix}layer{l}."
            W = sd[p + "conv.weight"].detach().double().cpu().reshape(sd[p + "conv.weight"].shape[0], -1)
            gamma, beta = sd[p + "bn.bn.weight"].double().cpu(), sd[p + "bn.bn.bias"].double().cpu()
            mean, var = sd[p + "bn.bn.running_mean"].double().cpu(), sd[p + "bn.bn.running_var"].double().cpu()
            scale = gamma / torch.sqrt(var + BN_EPS)
            Wf = W * scale[:, None]
            bf = beta - mean * scale
            if l == 0:
                if Wf.shape[1] != cin_feat + 3:
                    raise ValueError(f"{p}conv.weight has {Wf.shape[1]} input channels, expected {cin_feat + 3}")
                # hoisted form (csrc/sa_mlp.hip): feature half applied once per source point, xyz half while gathering
                self.w1_feat = Wf[:, 3:].float().contiguous()  # [c1, cin]
                c1p = _round16(Wf.shape[0])
                wxyz = torch.zeros(c1p, 4)
                wxyz[: Wf.shape[0], :3] = Wf[:, :3].float()
                self.wxyz = wxyz.to(device)
                Wf = torch.cat([Wf[:, 3:], Wf[:, :3]], dim=1)  # [dx,dy,dz,feat] -> [feat,dx,dy,dz]
            folded.append((Wf.float(), bf.float()))
            self.couts.append(Wf.shape[0])
            l += 1
        if l != 3:
            raise ValueError(f"{prefix}: the fused SA kernel expects 3-layer shared MLPs, found {l}")
        self._folded_plain = [(W.clone(), b.clone()) for W, b in folded]  # channel order as trained (the fp32 packs below may permute it)
        self._device = device
        self._bf16x3 = None
        self._bf16x9 = None
        self._bf16x9_lds = None
        c2 = self.couts[1]
        if c2 % 16:
            # hidden width not a multiple of 16 (light level 2: 196): the channels of the last, partly filled 16-channel block go to
            # positions 4 (c % 4) + c / 4 of it (GP_SA_TAIL_SPREAD, genpose_hip.h) - as rows of layer 2 and columns of layer 3 alike, so
            # the network is unchanged - and the chain kernels skip the k-steps of that block that only multiply padding
            self.hidden_layout = 1
            pos = torch.tensor([_lib.lib().gp_sa_tail_position(c2, c) for c in range(c2)], dtype=torch.long)
            (W2, b2), (W3, b3) = folded[1], folded[2]
            W2s, b2s = torch.zeros(_round16(c2), W2.shape[1]), torch.zeros(_round16(c2))
            W2s[pos], b2s[pos] = W2, b2
            W3s = torch.zeros(W3.shape[0], _round16(c2))
            W3s[:, pos] = W3
            folded[1], folded[2] = (W2s, b2s), (W3s, b3)
        self.layers = [(pack_weight(W).to(device), pad_bias(b).to(device)) for W, b in folded]


    def bf16x3_packs(self):
        """Operands of the opt-in split-bf16 kernel (csrc/sa_bf16x3.hip) for layers 2 and 3: every weight as hi = bf16(w) and
        lo = bf16(w - hi), in the fragment order of v_mfma_f32_16x16x32_bf16 with the k order the register chain produces -
        k-block m = channels 32 m .. 32 m + 31, lane group g holds [32m + 4g .. +3] and [32m + 16 + 4g .. +3].
        -> (w2 [KB1][NC2][2][64][8], b2 [32 KB2], w3 [c3/128][KB2][8][2][64][8], b3) as int16 / float32 device tensors."""
        if self._bf16x3 is None:
            (_, _), (W2, b2), (W3, b3) = self._folded_plain
            c1, c2, c3 = self.couts
            nc2 = (c2 + 15) // 16
            kb2 = (nc2 + 1) // 2
            w2 = pack_bf16x3(W2, nc2, c1 // 32)                                   # [KB1][NC2][2][64][8]
            w3 = pack_bf16x3(W3, c3 // 16, kb2)                                   # [KB2][16][2][64][8]
            w3 = torch.stack([w3[:, 8 * h:8 * h + 8] for h in range(c3 // 128)], dim=0).contiguous()  # [half][KB2][8][2][64][8]: slice = (half, k-block)
            b2p = torch.zeros(32 * kb2)
            b2p[:c2] = b2
            dev = self._device
            self._bf16x3 = (w2.to(dev), b2p.to(dev), w3.to(dev), b3.float().contiguous().to(dev))
        return self._bf16x3


    def bf16x9_packs(self):
        """Operands of the exact-product split-bf16 level-2 kernel (csrc/sa_bf16x9.hip) for layers 2 and 3 (128 -> 196 -> 256):
        -> (w [22][8][3][64][8] int16 (pack_sa_bf16x9), b2 [224] zero padded, b3 [256]) as device tensors, channel order as trained; or None
        where a BN-folded weight does not split exactly into three normal bf16 terms (split_bf16x9) - the caller keeps the fp32 kernel."""
        if self._bf16x9 is None:
            (_, _), (W2, b2), (W3, b3) = self._folded_plain
            try:
                w = pack_sa_bf16x9(W2, W3)
            except ValueError:
                self._bf16x9 = False
                return None
            b2p = torch.zeros(224)
            b2p[:b2.numel()] = b2
            dev = self._device
            self._bf16x9 = (w.to(dev), b2p.to(dev), b3.float().contiguous().to(dev))
        return self._bf16x9 or None

    def bf16x9_lds_packs(self):
        """Operands of the exact-product split-bf16 kernel with LDS-resident weights (csrc/sa_lds_bf16x9.hip: grouping level 1, hidden widths
        that are whole 32-wide k-blocks) for layers 2 and 3: -> (w2 [c1/32][c2/16][3][64][8] int16, b2 [c2], w3 [c2/32][c3/16][3][64][8], b3 [c3])
        as device tensors (pack_bf16x9, channel order as trained); or None where the widths are not whole k-blocks / chunks or a BN-folded
        weight does not split exactly into three normal bf16 terms (split_bf16x9) - the caller keeps the fp32 kernel for this scale."""
        if self._bf16x9_lds is None:
            (_, _), (W2, b2), (W3, b3) = self._folded_plain
            c1, c2, c3 = self.couts
            self._bf16x9_lds = False
            if c1 % 32 == 0 and c2 % 32 == 0 and c3 % 16 == 0:
                try:
                    w2, w3 = pack_bf16x9(W2, c2 // 16, c1 // 32), pack_bf16x9(W3, c3 // 16, c2 // 32)
                except ValueError:
                    return None
                dev = self._device
                self._bf16x9_lds = (w2.to(dev), b2.float().contiguous().to(dev), w3.to(dev), b3.float().contiguous().to(dev))
        return self._bf16x9_lds or None


def pack_bf16x3(W, n_chunks, k_blocks, chain=True):
    """W [n_out, k_in] f32 -> int16 [k_blocks][n_chunks][2 = hi, lo][64 lanes][8]: the A / B operand fragments of
    v_mfma_f32_16x16x32_bf16 for output chunk nc (16 outputs) and k-block kb (32 inputs), lane l = (n = l % 16, g = l // 16), element e:
    input channel 32 kb + (4 g + e if e < 4 else 16 + 4 g + e - 4) - two consecutive D fragments of the previous layer, as the register
    chain of csrc/sa_bf16x3.hip holds them (chain=False: the natural order 32 kb + 8 g + e, for a layer whose input is not a D fragment).
    Out-of-range outputs / inputs are zero."""
    Wp = _pad_for_fragments(W, n_chunks, k_blocks)
    hi = Wp.to(torch.bfloat16)
    lo = (Wp - hi.float()).to(torch.bfloat16)
    return _gather_fragments((hi, lo), n_chunks, k_blocks, chain)


def _pad_for_fragments(W, n_chunks, k_blocks):
    W = W.detach().float().cpu()
    Wp = torch.zeros(16 * n_chunks, 32 * k_blocks)
    Wp[:W.shape[0], :W.shape[1]] = W
    return Wp


def _gather_fragments(terms, n_chunks, k_blocks, chain):
    """bf16 terms, each [16 n_chunks, 32 k_blocks] -> int16 [k_blocks][n_chunks][len(terms)][64][8] in pack_bf16x3's fragment order."""
    terms = torch.stack([t.view(torch.int16) for t in terms], dim=0)
    lanes = torch.arange(64)
    n, g = lanes % 16, lanes // 16
    e = torch.arange(8)
    if chain:
        koff = torch.where(e < 4, 4 * g[:, None] + e[None, :], 16 + 4 * g[:, None] + (e[None, :] - 4))  # [64, 8]
    else:
        koff = 8 * g[:, None] + e[None, :]
    rows = (16 * torch.arange(n_chunks)[None, :, None, None] + n[None, None, :, None]).expand(k_blocks, n_chunks, 64, 8)
    cols = (32 * torch.arange(k_blocks)[:, None, None, None] + koff[None, None]).expand(k_blocks, n_chunks, 64, 8)
    return terms[:, rows, cols].permute(1, 2, 0, 3, 4).contiguous()  # [terms][kb][nc][64][8] -> [kb][nc][terms][64][8]


def split_bf16x9(W):
    """W f32 -> (hi, mid, lo) bf16 with hi + mid + lo == W exactly: hi = bf16(W), mid = bf16(W - hi), lo = bf16((W - hi) - mid), each
    rounded to nearest even; both differences are exact in fp32.  Raises ValueError where the three terms do not give W back bit for bit
    or a nonzero term lies below the normal range (the matrix pipe may flush it), and for non-finite weights."""
    W = W.detach().float().cpu()
    hi = W.to(torch.bfloat16)
    r = W - hi.float()
    mid = r.to(torch.bfloat16)
    lo = (r - mid.float()).to(torch.bfloat16)
    back = (hi.double() + mid.double()) + lo.double()
    tiny = torch.finfo(torch.float32).tiny
    bad = ~torch.isfinite(W) | (back != W.double())
    for t in (hi, mid, lo):
        bad |= (t.float() != 0) & (t.float().abs() < tiny)
    if bool(bad.any()):
        raise ValueError(f"{int(bad.sum())} weight(s) do not split exactly into three normal bf16 terms "
                         f"(first at index {tuple(bad.nonzero()[0].tolist())})")
    return hi, mid, lo


def pack_bf16x9(W, n_chunks, k_blocks, chain=True):
    """W [n_out, k_in] f32 -> int16 [k_blocks][n_chunks][3 = hi, mid, lo][64 lanes][8]: pack_bf16x3's fragment order and k order with the
    three exact terms of split_bf16x9 (checked there: hi + mid + lo == W for every weight).  Out-of-range outputs / inputs are zero."""
    return _gather_fragments(split_bf16x9(_pad_for_fragments(W, n_chunks, k_blocks)), n_chunks, k_blocks, chain)


def pack_heads_bf16x9(W):
    """The three stacked 256-wide heads [768, 256] -> int16 [head 3][chunk pair 8][chunk 2][k-block 8][3][64][8]: the stream of
    csrc/trunk_bf16x9.h's chunk-major head slices in the order they are consumed - a slice is (two output chunks 2 j, 2 j + 1 of a head) x
    (all eight k-blocks) x (hi, mid, lo).  A permutation of pack_bf16x9(W, 48, 8): fragments, k order and the exactness check are its."""
    if tuple(W.shape) != (768, 256):
        raise ValueError(f"stacked heads [768, 256] expected, got {tuple(W.shape)}")
    return pack_bf16x9(W, 48, 8).view(8, 3, 8, 2, 3, 64, 8).permute(1, 2, 3, 0, 4, 5, 6).contiguous()  # [kb][h][j][c] -> [h][j][c][kb]


def pack_sa_bf16x9(W2, W3):
    """Level 2's layer-2 [196, 128] and layer-3 [256, 196 (or zero padded up to 224)] weights -> int16 [22 slices][8 chunks][3][64][8]: the
    stream of csrc/sa_bf16x9.hip's ring in the order it is consumed.  Slices 0-7: layer 2 as (k-block kb, chunk half h) = 2 kb + h, output
    chunks 8 h .. 8 h + 7 (13 chunks padded to 16); slices 8-21: layer 3 as (half h, k-block kb) = 8 + 7 h + kb, output chunks 8 h .. 8 h + 7.
    Fragments, k order and the exactness check are pack_bf16x9's; out-of-range outputs / inputs are zero."""
    if tuple(W2.shape) != (196, 128) or W3.shape[0] != 256 or not 196 <= W3.shape[1] <= 224:
        raise ValueError(f"level-2 shapes [196, 128] and [256, 196..224] expected, got {tuple(W2.shape)} and {tuple(W3.shape)}")
    w2 = pack_bf16x9(W2, 16, 4).reshape(8, 8, 3, 64, 8)                      # [kb][16] -> [(kb, h)][8]
    w3 = pack_bf16x9(W3, 16, 7)                                              # [kb][16][3][64][8]
    w3 = torch.stack([w3[:, 8 * h:8 * h + 8] for h in range(2)], dim=0).reshape(14, 8, 3, 64, 8)  # [(h, kb)][8]
    return torch.cat([w2, w3], dim=0).contiguous()


def pack_groupall_bf16x9(W1, W2, W3):
    """One scale of the GroupAll level - layer 1's feature half [256, 512], layer 2 [C2, 256] and layer 3 [512, C2], C2 = 256 | 384 - ->
    int16 [80 | 104 slices][8 chunks][3][64][8]: the stream of csrc/sa_groupall_bf16x9.hip's ring in the order it is consumed.  For half
    h = 0, 1: layer 1's output chunks 8 h .. 8 h + 7 over its 16 k-blocks (16 slices), then layer 2's k-blocks 4 h .. 4 h + 3, each as C2 / 128
    slices of 8 output chunks (8 | 12 slices); then layer 3 as (group q of 8 output chunks, k-block) = 4 x C2 / 32 slices.  Fragments, k
    order and the exactness check are pack_bf16x9's."""
    c2 = W2.shape[0]
    if tuple(W1.shape) != (256, 512) or c2 not in (256, 384) or W2.shape[1] != 256 or tuple(W3.shape) != (512, c2):
        raise ValueError(f"GroupAll shapes [256, 512], [256 | 384, 256], [512, C2] expected, got {tuple(W1.shape)}, {tuple(W2.shape)}, {tuple(W3.shape)}")
    nh2, kb3 = c2 // 128, c2 // 32
    w1 = pack_bf16x9(W1, 16, 16)                                             # [kb 16][chunk 16][3][64][8]
    w2 = pack_bf16x9(W2, 8 * nh2, 8).reshape(8, nh2, 8, 3, 64, 8)            # [kb 8][chunk third / half][8]
    w3 = pack_bf16x9(W3, 32, kb3)                                            # [kb][chunk 32]
    parts = []
    for h in range(2):
        parts.append(w1[:, 8 * h:8 * h + 8])                                 # 16 slices
        parts.append(w2[4 * h:4 * h + 4].reshape(4 * nh2, 8, 3, 64, 8))
    parts += [w3[:, 8 * q:8 * q + 8] for q in range(4)]
    return torch.cat(parts, dim=0).contiguous()


class EncoderWeights:
    def __init__(self, sd, device, params="light", prefix="pts_encoder."):
        self._device = device
        self._groupall_x9 = None
        if params not in ENCODER_CFGS:
            raise NotImplementedError(params)
        self.cfg = ENCODER_CFGS[params]
        self.levels = []
        self.z_weights = []
        cin = 0
        for k, level in enumerate(self.cfg["mlps"]):
            scales = [SAScale(sd, f"{prefix}SA_modules.{k}.mlps.{i}.", cin, device) for i in range(len(level))]
            for sc, spec in zip(scales, level):
                if sc.couts != list(spec):
                    raise ValueError(f"SA level {k}: checkpoint layer widths {sc.couts} != config {spec}")
            self.levels.append(scales)
            # combined per-point first-layer weights of the level's scales: z = feat . [W1f_0 ; W1f_1]^T
            self.z_weights.append(pack_weight(torch.cat([sc.w1_feat for sc in scales], dim=0)).to(device) if cin > 0 else None)
            cin = sum(s.couts[-1] for s in scales)
        self.out_dim = cin

    def groupall_bf16x9_packs(self):
        """Operands of the exact-product split-bf16 GroupAll kernel (csrc/sa_groupall_bf16x9.hip): -> (w, slice offset of every scale) - the
        six matrices of the level's two scales as ONE int16 device tensor [80 + 104 slices][8][3][64][8] in the order the ring consumes them
        (pack_groupall_bf16x9 per scale) - or None where the level is not the light encoder's (128 points x 512 -> (256, 256 | 384, 512), two
        scales) or ANY of the six does not split exactly into three normal bf16 terms (split_bf16x9): the whole level then keeps the fp32
        kernels."""
        if self._groupall_x9 is None:
            self._groupall_x9 = False
            k = len(self.levels) - 1
            scales = self.levels[k]
            if self.cfg["npoints"][k] is None and k >= 1 and self.cfg["npoints"][k - 1] == 128 and len(scales) == 2:
                try:
                    packs = [pack_groupall_bf16x9(sc.w1_feat, sc._folded_plain[1][0], sc._folded_plain[2][0]) for sc in scales]
                except ValueError:
                    packs = None
                if packs is not None:
                    offs = [0, packs[0].shape[0]]
                    self._groupall_x9 = (torch.cat(packs, dim=0).contiguous().to(self._device), offs)
        return self._groupall_x9 or None


class PointNetWeights:
    """Device blocks of the vanilla PointNet encoder, PointNetfeat(num_points, out_dim=1024) (networks/pts_encoder/pointnets.py:83-123), from the
    reference's keys {prefix}stn.conv{1,2,3}, {prefix}stn.fc{1,2,3}, {prefix}conv{1..4} (.weight / .bias; Conv1d weights [Cout, Cin, 1]).
    Host-side work is layout only: the convolutions in the MFMA fragment order of gp_pack_weight, the fully connected layers of the transform
    net's head as trained ([out, in] row-major, gp_dense_rows), and the `+ iden` of STNkd.forward (pointnets.py:70-77) folded into fc3's bias."""
    STN_CONVS = ((3, 64), (64, 128), (128, 1024))
    STN_FCS = ((1024, 512), (512, 256), (256, 9))
    CONVS = ((3, 64), (64, 128), (128, 512), (512, 1024))

    def __init__(self, sd, device, prefix="pts_encoder."):
        def conv(name, cin, cout):
            W = sd[f"{prefix}{name}.weight"].detach().float().cpu()
            W = W.reshape(W.shape[0], -1)
            b = sd[f"{prefix}{name}.bias"].detach().float().cpu()
            if tuple(W.shape) != (cout, cin) or b.numel() != cout:
                raise ValueError(f"{prefix}{name}.weight is {tuple(W.shape)}, expected {(cout, cin)} (PointNetfeat with in_dim=3, out_dim=1024)")
            return W, b

        self.stn_convs = [(pack_weight(W).to(device), pad_bias(b).to(device)) for W, b in (conv(f"stn.conv{i + 1}", *s) for i, s in enumerate(self.STN_CONVS))]
        fcs = [conv(f"stn.fc{i + 1}", *s) for i, s in enumerate(self.STN_FCS)]
        W3, b3 = fcs[2]
        fcs[2] = (W3, b3 + torch.eye(3).reshape(9))
        self.stn_fcs = [(W.contiguous().to(device), b.contiguous().to(device)) for W, b in fcs]
        self.convs = [(pack_weight(W).to(device), pad_bias(b).to(device)) for W, b in (conv(f"conv{i + 1}", *s) for i, s in enumerate(self.CONVS))]
        self.out_dim = self.CONVS[-1][1]


class ScoreNetWeights:
    """Device block behind `struct gp_scorenet` (score and energy nets share the layout, posenet.py:58-67)."""

    def __init__(self, sd, device, prefix="pose_score_net."):
        g = lambda k: sd[prefix + k].detach().to(torch.float32).cpu()
        heads = ("rot_x", "rot_y", "trans")
        W1 = torch.cat([g(f"fusion_tail_{h}.0.weight") for h in heads], dim=0)  # [768, 1408] = [pts 1024 | t 128 | pose 256]
        if W1.shape != (768, 1408):
            raise ValueError(f"unexpected fusion_tail first-layer shape {tuple(W1.shape)} (need Rx_Ry_and_T heads, 1024-d pts feature)")
        b1 = torch.cat([g(f"fusion_tail_{h}.0.bias") for h in heads], dim=0)
        W2 = torch.cat([g(f"fusion_tail_{h}.2.weight") for h in heads], dim=0)  # [9, 256]
        b2 = torch.cat([g(f"fusion_tail_{h}.2.bias") for h in heads], dim=0)
        t = {}
        t["w_pose0"] = pack_weight(g("pose_encoder.0.weight"))
        t["b_pose0"] = pad_bias(g("pose_encoder.0.bias"))
        t["w_pose2"] = pack_weight(g("pose_encoder.2.weight"))
        t["b_pose2"] = pad_bias(g("pose_encoder.2.bias"))
        t["w_headx"] = pack_weight(W1[:, 1152:1408].contiguous())
        t["w_out"] = W2.contiguous()
        t["b_out"] = torch.cat([b2, torch.zeros(7)])
        t["fourier_w"] = g("t_encoder.0.W")
        t["w_t1"] = g("t_encoder.1.weight").t().contiguous()  # [in][out]
        t["b_t1"] = g("t_encoder.1.bias")
        t["w_headt"] = W1[:, 1024:1152].t().contiguous()  # [128][768]
        t["w_headp"] = pack_weight(W1[:, :1024].contiguous())
        t["b_head"] = b1.contiguous()
        # transposed packs: backward pass of gp_score_div
        t["w_headx_t"] = pack_weight(W1[:, 1152:1408].t().contiguous())
        t["w_pose2_t"] = pack_weight(g("pose_encoder.2.weight").t().contiguous())
        t["w_pose0_t"] = pack_weight(g("pose_encoder.0.weight").t().contiguous())
        self.tensors = {k: v.to(device) for k, v in t.items()}
        self.struct = _lib.GpScoreNet(**{k: v.data_ptr() for k, v in self.tensors.items()})
        self._raw = {"pose0": g("pose_encoder.0.weight"), "pose2": g("pose_encoder.2.weight"), "headx": W1[:, 1152:1408].contiguous()}
        self._device = device
        self._bf16x3 = None
        self._bf16x9 = None

    def bf16x3_packs(self):
        """Operands of the opt-in split-bf16 PC step (csrc/trunk_bf16x3.hip): the three dense layers of the trunk as hi / lo bf16 pairs in
        the fragment order of v_mfma_f32_16x16x32_bf16 (pack_bf16x3) -> (w_pose0 [1][16][2][64][8], w_pose2 [8][16]..., w_headx [8][48]...)."""
        if self._bf16x3 is None:
            r = self._raw
            self._bf16x3 = (pack_bf16x3(r["pose0"], 16, 1, chain=False).to(self._device), pack_bf16x3(r["pose2"], 16, 8).to(self._device),
                            pack_bf16x3(r["headx"], 48, 8).to(self._device))
        return self._bf16x3

    def bf16x9_packs(self):
        """Operands of the bf16x9 chain kernels (csrc/trunk_bf16x9.h: PC step, Heun step, RK45 stage): the three dense layers of the trunk as
        exact hi / mid / lo bf16 triples in the fragment order of v_mfma_f32_16x16x32_bf16 (pack_bf16x9), the heads in the order the ring
        consumes them (pack_heads_bf16x9)
        -> (w_pose0 [1][16][3][64][8], w_pose2 [8][16][3][64][8], w_headx [3][8][2][8][3][64][8]) as int16 device tensors."""
        if self._bf16x9 is None:
            r = self._raw
            self._bf16x9 = (pack_bf16x9(r["pose0"], 16, 1, chain=False).to(self._device), pack_bf16x9(r["pose2"], 16, 8).to(self._device),
                            pack_heads_bf16x9(r["headx"]).to(self._device))
        return self._bf16x9

    def ref(self):
        return ctypes.byref(self.struct)
