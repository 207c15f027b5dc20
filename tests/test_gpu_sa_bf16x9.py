"""GPU: grouping level 2 (256 source points x 128 hoisted channels -> 196 -> 256, 128 centres, ns = 16 | 32) as exact-product split bf16
(csrc/sa_bf16x9.hip, encoder precision 'bf16x9' - the default of a PC-sampler agent) against a float64 evaluation of the same indices and weights, against the
fp32 MFMA kernel it replaces, and for its padding, fallback, position independence and opt-out.

Tolerance: both kernels round only in their fp32 accumulations (every bf16 cross product is exact), in different orders.  The fp32 kernel's
own max error over the feature scale against float64 is MEASURED here on the same inputs; the split kernel gets twice that.
Measured (MI355X, profiles/r10_sa_bf16x9.txt): see that file; the fp32 figure recorded before this kernel existed is 5.8e-7."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

NB = 5            # clouds of the shared batch; the last one consists of tiled duplicate points
BATCHES = (1, 2, 3, 5)


@functools.lru_cache(maxsize=None)
def _setup():
    """Encoders, one five-cloud pass of the fp32 encoder (its grouping, hoisted features and level-2 output) and the float64 reference of
    level 2 on those inputs - computed once, read-only afterwards."""
    from genpose_amd import synth
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd = go.make_state_dict(0, "score")
    e32 = Pointnet2EncoderHIP(sd, "cuda", precision="f32")
    e9 = Pointnet2EncoderHIP(sd, "cuda", precision="bf16x9")
    pts = torch.from_numpy(synth.make_batch(NB, start=4321)).cuda().float()
    pts[NB - 1] = pts[NB - 1, :64].repeat(pts.shape[1] // 64, 1)  # tiled duplicates: every neighbourhood is full of repeated points
    _, ws = e32.forward(pts, return_intermediates=True)
    ins = {"xyz": ws["new_xyz"][1].clone(), "new_xyz": ws["new_xyz"][2].clone(), "z": ws["z"][2].clone(),
           "idx": [t.clone() for t in ws["bq"][2]], "feat32": ws["feat"][2].clone()}
    assert ins["xyz"].shape == (NB, 256, 3) and ins["z"].shape == (NB, 256, 256) and ins["new_xyz"].shape == (NB, 128, 3)
    ref = _level2_fp64(ins, [sc._folded_plain for sc in e32.w.levels[2]])
    return sd, e32, e9, pts, ins, ref


def _level2_fp64(ins, folded):
    """float64 on the host from the hoisted fp32 features z, the coordinates, the indices and the folded weights:
    h1 = relu(z_j + Wxyz (x_j - c) + b1) -> relu(W2 h1 + b2) -> max_j relu(W3 h2 + b3); -> [B, 128, 512]."""
    xyz, centres, z = ins["xyz"].double().cpu(), ins["new_xyz"].double().cpu(), ins["z"].double().cpu()
    B = xyz.shape[0]
    bi = torch.arange(B)[:, None, None]
    outs = []
    for i, ((W1, b1), (W2, b2), (W3, b3)) in enumerate(folded):
        W1, b1, W2, b2, W3, b3 = (t.double() for t in (W1, b1, W2, b2, W3, b3))  # W1 columns: [feat..., dx, dy, dz]
        idx = ins["idx"][i].long().cpu()
        d = xyz[bi, idx] - centres[:, :, None, :]
        h1 = torch.relu(z[bi, idx][..., 128 * i:128 * i + 128] + d @ W1[:, -3:].t() + b1)
        h2 = torch.relu(h1 @ W2.t() + b2)
        outs.append(torch.relu(h2 @ W3.t() + b3).max(dim=2)[0])
    return torch.cat(outs, dim=-1)


def _run(kind, sc, i, ins, B, packs=None):
    """Scale i of level 2 for the first B clouds through the C entry point: kind 'f32' (gp_sa_pre_mlp_max_layout) | 'x9'; -> [B, 128, 256]."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    ns = ins["idx"][i].shape[-1]
    out = torch.full((B, 128, 512), float("nan"), device="cuda")
    (_, b1), (w2, b2), (w3, b3) = sc.layers
    head = (B, 256, 128, ns, 128, 196, 256, ptr(ins["xyz"]), ptr(ins["new_xyz"]), ptr(ins["idx"][i]), ptr(ins["z"]), 256, 128 * i, ptr(sc.wxyz), ptr(b1))
    if kind == "f32":
        _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, *head, ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 512, 256 * i, stream_ptr())
    else:
        w, b2p, b3p = packs if packs is not None else sc.bf16x9_packs()
        _lib.call("gp_sa_pre_mlp_max_bf16x9", *head, ptr(w), ptr(b2p), ptr(b3p), ptr(out), 512, 256 * i, stream_ptr())
    torch.cuda.synchronize()
    other = out[..., 256 * (1 - i):256 * (1 - i) + 256]
    assert bool(torch.isnan(other).all())  # the other scale's columns are not touched
    return out[..., 256 * i:256 * i + 256].clone()


def test_against_float64_within_twice_the_fp32_kernels_error():
    sd, e32, e9, pts, ins, ref = _setup()
    scale = float(ref.abs().max())
    rows = []
    for B in BATCHES:
        for i, sc in enumerate(e32.w.levels[2]):
            r = ref[:B, :, 256 * i:256 * i + 256]
            o32, o9 = _run("f32", sc, i, ins, B), _run("x9", e9.w.levels[2][i], i, ins, B)
            assert torch.equal(o32, ins["feat32"][:B, :, 256 * i:256 * i + 256])  # the direct call is what the 'f32' encoder ran
            rows.append((B, ins["idx"][i].shape[-1], float((o32.double().cpu() - r).abs().max()) / scale, float((o9.double().cpu() - r).abs().max()) / scale))
    e32_max = max(r[2] for r in rows)
    for B, ns, a, b in rows:
        print(f"level 2, {B} cloud(s), ns = {ns}: max error / feature scale vs float64: fp32 MFMA {a:.3e}, bf16x9 {b:.3e}")
    print(f"fp32 MFMA kernel, max over the cases: {e32_max:.3e}; bound for bf16x9: {2 * e32_max:.3e}; bf16x9 max: {max(r[3] for r in rows):.3e}")
    assert 0 < e32_max < 3e-6  # the fp32 kernel is in its recorded class (5.8e-7), so the bound means something
    for B, ns, a, b in rows:  # every case
        assert b <= 2 * e32_max, (B, ns, a, b, e32_max)


def test_padding_lanes_never_reach_the_output():
    from genpose_amd.weights import pack_sa_bf16x9
    sd, e32, e9, pts, ins, ref = _setup()
    g = torch.Generator().manual_seed(5)
    for i, sc in enumerate(e9.w.levels[2]):
        (W1, b1), (W2, b2), (W3, b3) = sc._folded_plain
        b2big = b2.clone()
        b2big[190:196] = 40.0  # the last real channels of the partly filled chunk 12 carry a large bias; its padding channels must not
        b2p = torch.zeros(224)
        b2p[:196] = b2big
        W3poison = torch.cat([W3, 1e3 * torch.randn(256, 28, generator=g)], dim=1)  # columns 196-223 meet only the zero k-padding
        clean = (pack_sa_bf16x9(W2, W3).cuda(), b2p.cuda(), b3.cuda())
        poisoned = (pack_sa_bf16x9(W2, W3poison).cuda(), b2p.cuda(), b3.cuda())
        assert not torch.equal(clean[0], poisoned[0])
        for B in (1, 3):
            a, b = _run("x9", sc, i, ins, B, clean), _run("x9", sc, i, ins, B, poisoned)
            assert torch.equal(a, b), (i, B)
            r = _level2_fp64({k: (v[:B] if k != "idx" else [t[:B] for t in v]) for k, v in ins.items()}, [((W1, b1), (W2, b2big), (W3, b3))] * (i + 1))
            r = r[..., 256 * i:256 * i + 256]
            assert float((a.double().cpu() - r).abs().max()) <= 3e-6 * float(r.abs().max()), (i, B)  # channels 190-195 DID get their bias
            assert not torch.equal(a, _run("x9", sc, i, ins, B))


def test_unsplittable_weight_keeps_the_fp32_kernel_for_that_scale():
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd, e32, e9, pts, ins, ref = _setup()
    bad = dict(sd)
    key = "pts_encoder.SA_modules.2.mlps.0.layer1.conv.weight"
    W = bad[key].clone()
    W[7, 11] = 1e-40  # subnormal: its bf16 terms lie below the normal range, the matrix pipe may flush them
    bad[key] = W
    eb, ef = Pointnet2EncoderHIP(bad, "cuda", precision="bf16x9"), Pointnet2EncoderHIP(bad, "cuda", precision="f32")
    assert eb.sa_kernels[(2, 0)] == "f32mfma" and eb.sa_kernels[(2, 1)] == "bf16x9"
    assert set(ef.sa_kernels.values()) == {"f32mfma"}
    (_, wb), (_, wf) = eb.forward(pts, return_intermediates=True), ef.forward(pts, return_intermediates=True)
    assert torch.equal(wb["feat"][2][..., :256], wf["feat"][2][..., :256])
    assert not torch.equal(wb["feat"][2][..., 256:], wf["feat"][2][..., 256:])


def test_a_clouds_features_do_not_depend_on_its_position_or_the_replay():
    sd, e32, e9, pts, ins, ref = _setup()
    for c in (0, NB - 1):
        X = pts[c]
        five = torch.stack([X, pts[1], X, pts[2], X]).contiguous()
        f1, w1 = e9.forward(X[None].contiguous(), return_intermediates=True)
        f1, l1 = f1.clone(), w1["feat"][2].clone()
        f5, w5 = e9.forward(five, return_intermediates=True)
        for pos in (0, 2, 4):
            assert torch.equal(w5["feat"][2][pos], l1[0]) and torch.equal(f5[pos], f1[0]), (c, pos)
    feats = [e9.encode(pts)[0].clone() for _ in range(4)]  # launch by launch, capture + replay, replay, replay
    assert all(torch.equal(feats[0], f) for f in feats[1:])
    assert torch.equal(feats[0], e9.forward(pts))


def test_default_selects_the_split_kernel_and_f32_opts_out():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    sd, e32, e9, pts, ins, ref = _setup()
    assert e9.precision == "bf16x9" and e9.sa_kernels[(2, 0)] == e9.sa_kernels[(2, 1)] == "bf16x9"
    assert all(v == "f32mfma" for k, v in e9.sa_kernels.items() if k[0] != 2) and set(e32.sa_kernels.values()) == {"f32mfma"}
    f9, w9 = e9.forward(pts, return_intermediates=True)
    for k in (0, 1):
        assert torch.equal(w9["feat"][k], e32.forward(pts, return_intermediates=True)[1]["feat"][k])  # levels 0 and 1: the same kernels
    for i, sc in enumerate(e9.w.levels[2]):
        x9, f32 = _run("x9", sc, i, ins, NB), _run("f32", e32.w.levels[2][i], i, ins, NB)
        assert torch.equal(w9["feat"][2][..., 256 * i:256 * i + 256], x9)                     # the default ran the split kernel ...
        assert torch.equal(ins["feat32"][..., 256 * i:256 * i + 256], f32)                    # ... 'f32' the fp32 MFMA kernel, as before
        assert not torch.equal(x9, f32)
    for cfg, want in ((get_config(sampler_mode=["pc"]), "bf16x9"), (get_config(sampler_mode=["pc"], encoder_level2="f32mfma"), "f32"),
                      (get_config(sampler_mode=["ode"]), "f32"), (get_config(encoder_precision="bf16x9"), "bf16x9")):
        a = PoseNet(cfg)
        a.load_state_dict(sd)
        assert a.net.pts_encoder.precision == want
