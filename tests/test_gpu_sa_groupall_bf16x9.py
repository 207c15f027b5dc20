"""GPU: the GroupAll level (128 points x [512 features + xyz] -> 256 -> 256 | 384 -> 512, max over the cloud, two scales) as exact-product
split bf16 in one launch (csrc/sa_groupall_bf16x9.hip, Pointnet2EncoderHIP(level3='bf16x9') - the default of a PC-sampler agent) against a
float64 evaluation of the same features, coordinates and folded weights, against the fp32 path it replaces (gp_point_linear + the fp32
GroupAll kernels), and for its independence of placement, its output range, its fallback, its selection and its argument checks.

Tolerance: both paths round only in their fp32 accumulations (every bf16 cross product is exact), in different orders.  The fp32 path's own
max error over the feature scale against float64 is MEASURED here on the same inputs; the split kernel gets twice that (the rule of
test_gpu_sa_bf16x9.py).  Measured figures: profiles/sa_groupall_bf16x9.txt."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

NB = 5            # clouds of the shared batch; the last one consists of tiled duplicate points
BATCHES = (1, 2, 3, 5)
C2 = (256, 384)


@functools.lru_cache(maxsize=None)
def _setup():
    """One five-cloud pass of the fp32 encoder (its level-2 features and centres, its GroupAll output) and the float64 reference of the
    GroupAll level on those inputs - computed once, read-only afterwards."""
    from genpose_amd import synth
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd = go.make_state_dict(0, "score")
    e32 = Pointnet2EncoderHIP(sd, "cuda")
    pts = torch.from_numpy(synth.make_batch(NB, start=4321)).cuda().float()
    pts[NB - 1] = pts[NB - 1, :64].repeat(pts.shape[1] // 64, 1)  # tiled duplicates
    f32, ws = e32.forward(pts, return_intermediates=True)
    ins = {"xyz": ws["new_xyz"][2].clone(), "feat": ws["feat"][2].clone(), "out32": ws["feat"][3].reshape(NB, 1024).clone()}
    assert ins["xyz"].shape == (NB, 128, 3) and ins["feat"].shape == (NB, 128, 512) and torch.equal(ins["out32"], f32)
    ref = _groupall_fp64(ins, [sc._folded_plain for sc in e32.w.levels[3]])
    return sd, e32, pts, ins, ref


def _groupall_fp64(ins, folded):
    """float64 on the host: h1 = relu(W1 [feat, x] + b1) -> relu(W2 h1 + b2) -> max over the points of relu(W3 h2 + b3); -> [B, 1024]."""
    x = torch.cat([ins["feat"].double().cpu(), ins["xyz"].double().cpu()], dim=-1)  # W1 columns: [feat..., x, y, z]
    outs = []
    for (W1, b1), (W2, b2), (W3, b3) in folded:
        W1, b1, W2, b2, W3, b3 = (t.double() for t in (W1, b1, W2, b2, W3, b3))
        h2 = torch.relu(torch.relu(x @ W1.t() + b1) @ W2.t() + b2)
        outs.append(torch.relu(h2 @ W3.t() + b3).max(dim=1)[0])
    return torch.cat(outs, dim=-1)


def _run_f32(e, xyz, feat):
    """The fp32 path through the C entry points, as the encoder issues it; -> [B, 1024]."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    B = feat.shape[0]
    out = torch.zeros(B, 1024, device="cuda")
    z = torch.empty(B, 128, 512, device="cuda")
    _lib.call("gp_point_linear", B * 128, 512, 512, ptr(feat), ptr(e.w.z_weights[3]), ptr(z), stream_ptr())
    for i, sc in enumerate(e.w.levels[3]):
        (_, b1), (w2, b2), (w3, b3) = sc.layers
        _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, B, 128, 1, 128, 256, C2[i], 512, ptr(xyz), None, None, ptr(z), 512, 256 * i, ptr(sc.wxyz),
                  ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 1024, 512 * i, stream_ptr())
    torch.cuda.synchronize()
    return out


def _x9_args(e, xyz, feat, out, scales):
    from genpose_amd._lib import ptr, stream_ptr
    wx9, offs = e.w.groupall_bf16x9_packs()
    sargs = []
    for i in scales:
        sc = e.w.levels[3][i]
        (_, b1), (_, b2), (_, b3) = sc.layers
        sargs += [C2[i], ptr(wx9[offs[i]:]), ptr(sc.wxyz), ptr(b1), ptr(b2), ptr(b3), 512 * i]
    if len(scales) == 1:
        sargs += [0, None, None, None, None, None, 0]
    return [feat.shape[0], 128, 512, 256, 512, ptr(xyz), ptr(feat), *sargs, ptr(out), 1024, stream_ptr()]


def _run_x9(e, xyz, feat, scales=(0, 1), out=None, sync=True):
    """The split-bf16 kernel through its C entry point, both scales in one launch or one of them; -> [B, 1024], NaN where nothing was written."""
    from genpose_amd import _lib
    if out is None:
        out = torch.full((feat.shape[0], 1024), float("nan"), device="cuda")
    _lib.call("gp_sa_groupall_bf16x9", *_x9_args(e, xyz, feat, out, scales))
    if sync:
        torch.cuda.synchronize()
    return out


def test_against_float64_within_twice_the_fp32_paths_error():
    sd, e32, pts, ins, ref = _setup()
    scale = float(ref.abs().max())
    rows = []
    for B in BATCHES:
        xyz, feat = ins["xyz"][:B].contiguous(), ins["feat"][:B].contiguous()
        o32, o9 = _run_f32(e32, xyz, feat), _run_x9(e32, xyz, feat)
        assert torch.equal(o32, ins["out32"][:B])  # the direct calls are what the fp32 encoder ran
        for i in range(2):
            alone = _run_x9(e32, xyz, feat, scales=(i,))  # one scale alone: the same bits as in the two-scale launch
            assert torch.equal(alone[:, 512 * i:512 * i + 512], o9[:, 512 * i:512 * i + 512])
            r = ref[:B, 512 * i:512 * i + 512]
            rows.append((B, C2[i], float((o32[:, 512 * i:512 * i + 512].double().cpu() - r).abs().max()) / scale,
                         float((o9[:, 512 * i:512 * i + 512].double().cpu() - r).abs().max()) / scale))
    e32_max = max(r[2] for r in rows)
    for B, c2, a, b in rows:
        print(f"GroupAll, {B} cloud(s), C2 = {c2}: max error / feature scale vs float64: fp32 path {a:.3e}, bf16x9 {b:.3e}")
    print(f"fp32 path, max over the cases: {e32_max:.3e}; bound for bf16x9: {2 * e32_max:.3e}; bf16x9 max: {max(r[3] for r in rows):.3e}")
    assert 0 < e32_max < 3e-6  # the fp32 path is in its class, so the bound means something
    for B, c2, a, b in rows:  # every case
        assert b <= 2 * e32_max, (B, c2, a, b, e32_max)


def test_a_clouds_bits_do_not_depend_on_its_position_or_the_batch():
    sd, e32, pts, ins, ref = _setup()
    for c in (0, NB - 1):
        X, F = ins["xyz"][c], ins["feat"][c]
        one = _run_x9(e32, X[None].contiguous(), F[None].contiguous())
        five = _run_x9(e32, torch.stack([X, ins["xyz"][1], X, ins["xyz"][2], X]).contiguous(), torch.stack([F, ins["feat"][1], F, ins["feat"][2], F]).contiguous())
        for pos in (0, 2, 4):
            assert torch.equal(five[pos], one[0]), (c, pos)
    # more clouds than compute units: the persistent loop wraps and the weight stream runs on from item to item, on every workgroup
    n = torch.cuda.get_device_properties(0).multi_processor_count + 1
    sel = torch.arange(n, device="cuda") % 3
    many = _run_x9(e32, ins["xyz"][sel].contiguous(), ins["feat"][sel].contiguous())
    singles = torch.cat([_run_x9(e32, ins["xyz"][c:c + 1].contiguous(), ins["feat"][c:c + 1].contiguous()) for c in range(3)])
    assert not bool(torch.isnan(many).any())
    assert torch.equal(many, singles[sel])


def test_capture_and_replay_give_the_launched_bits():
    sd, e32, pts, ins, ref = _setup()
    xyz, feat = ins["xyz"], ins["feat"]
    direct = _run_x9(e32, xyz, feat).clone()
    out = torch.full((NB, 1024), float("nan"), device="cuda")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run_x9(e32, xyz, feat, out=out, sync=False)
    for _ in range(2):  # capture + replay, then a second replay
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, direct)


def test_only_the_scales_columns_are_written():
    sd, e32, pts, ins, ref = _setup()
    both = _run_x9(e32, ins["xyz"], ins["feat"])
    assert not bool(torch.isnan(both).any())
    for i in range(2):
        o = _run_x9(e32, ins["xyz"], ins["feat"], scales=(i,))
        assert not bool(torch.isnan(o[:, 512 * i:512 * i + 512]).any())
        assert bool(torch.isnan(o[:, 512 * (1 - i):512 * (1 - i) + 512]).all())
    # a wider row: nothing outside [off, off + 512) of either scale
    from genpose_amd import _lib
    wide = torch.full((NB, 1040), float("nan"), device="cuda")
    args = _x9_args(e32, ins["xyz"], ins["feat"], wide, (0, 1))
    args[13], args[20], args[22] = 4, 520, 1040  # cout_off_a, cout_off_b, cout_total
    _lib.call("gp_sa_groupall_bf16x9", *args)
    torch.cuda.synchronize()
    assert torch.equal(wide[:, 4:516], both[:, :512]) and torch.equal(wide[:, 520:1032], both[:, 512:])
    assert bool(torch.isnan(wide[:, :4]).all()) and bool(torch.isnan(wide[:, 516:520]).all()) and bool(torch.isnan(wide[:, 1032:]).all())


def test_unsplittable_weight_keeps_the_fp32_kernels_for_the_whole_level():
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd, e32, pts, ins, ref = _setup()
    bad = dict(sd)
    key = "pts_encoder.SA_modules.3.mlps.1.layer1.conv.weight"
    W = bad[key].clone()
    W[7, 11] = 1e-40  # subnormal: its bf16 terms lie below the normal range, the matrix pipe may flush them
    bad[key] = W
    eb, ef = Pointnet2EncoderHIP(bad, "cuda", level3="bf16x9"), Pointnet2EncoderHIP(bad, "cuda")
    eb.LEVEL3_BF16X9_MIN_CLOUDS = 1
    assert eb.level3 == "bf16x9" and eb.level3_kernel == "f32mfma" and eb.w.groupall_bf16x9_packs() is None
    assert torch.equal(eb.forward(pts), ef.forward(pts))


def test_selection_by_agent_kind_and_direct_construction():
    from genpose_amd.config import get_config
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from genpose_amd.posenet_agent import PoseNet
    sd, e32, pts, ins, ref = _setup()
    assert e32.level3 == "f32mfma" and e32.level3_kernel == "f32mfma" and get_config().encoder_level3 == "auto"
    for cfg, want in ((get_config(sampler_mode=["pc"]), "bf16x9"), (get_config(sampler_mode=["ode"]), "f32mfma"),
                      (get_config(sampler_mode=["heun"], sampling_steps=8), "f32mfma"), (get_config(sampler_mode=["dpm2m"], sampling_steps=8), "f32mfma"),
                      (get_config(sampler_mode=["pc"], encoder_level3="f32mfma"), "f32mfma"), (get_config(sampler_mode=["ode"], encoder_level3="bf16x9"), "bf16x9")):
        a = PoseNet(cfg)
        a.load_state_dict(sd)
        assert a.net.pts_encoder.level3 == want and a.net.pts_encoder.level3_kernel == want, (cfg.sampler_mode, want)
    with pytest.raises(ValueError):
        Pointnet2EncoderHIP(sd, "cuda", level3="fp8")
    # the encoder runs what the entry point computes, from its threshold upward; below it, and by default, the fp32 kernels' bits
    e9 = Pointnet2EncoderHIP(sd, "cuda", level3="bf16x9")
    assert e9.level3_kernel == "bf16x9" and e9.precision == "f32" and set(e9.sa_kernels.values()) == {"f32mfma"}
    assert NB < e9.LEVEL3_BF16X9_MIN_CLOUDS and torch.equal(e9.forward(pts), ins["out32"])
    e9.LEVEL3_BF16X9_MIN_CLOUDS = 1
    x9 = _run_x9(e32, ins["xyz"], ins["feat"])
    f9, w9 = e9.forward(pts, return_intermediates=True)
    assert torch.equal(w9["feat"][2], ins["feat"]) and torch.equal(f9, x9) and not torch.equal(f9, ins["out32"])


def test_bad_arguments_are_refused():
    from genpose_amd import _lib
    sd, e32, pts, ins, ref = _setup()
    fn = _lib.lib().gp_sa_groupall_bf16x9
    out = torch.full((NB, 1024), float("nan"), device="cuda")
    good = _x9_args(e32, ins["xyz"], ins["feat"], out, (0, 1))
    EINVAL = -1

    def changed(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)

    assert changed(a0=0) == 0                                  # b = 0: nothing to do
    assert changed(a0=-1) == EINVAL
    assert changed(a1=64) == EINVAL and changed(a2=256) == EINVAL and changed(a3=128) == EINVAL and changed(a4=256) == EINVAL  # n, cin, c1, c3
    assert changed(a7=196) == EINVAL and changed(a14=512) == EINVAL   # c2 of either scale
    assert changed(a6=ctypes.c_void_p(ins["feat"].data_ptr() + 4)) == EINVAL     # feat: 16 bytes
    assert changed(a8=ctypes.c_void_p(good[8].value + 8)) == EINVAL              # weight stream: 16 bytes
    assert changed(a9=ctypes.c_void_p(good[9].value + 4)) == EINVAL              # wxyz rows: 16 bytes
    assert changed(a21=ctypes.c_void_p(out.data_ptr() + 2)) == EINVAL            # out: 4 bytes
    assert changed(a5=None) == EINVAL and changed(a15=None) == EINVAL
    assert changed(a13=516) == EINVAL and changed(a20=256) == EINVAL and changed(a22=1022) == EINVAL  # columns out of range / overlapping / odd
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())  # none of them launched
