"""GPU: grouping level 1 (512 source points x 64 hoisted channels -> 64 | 96 -> 128, 256 centres, ns = 16 | 32) as exact-product split bf16
with LDS-resident weights (csrc/sa_lds_bf16x9.hip, Pointnet2EncoderHIP(level1='bf16x9') - the default of a PC-sampler agent) against a
float64 evaluation of the same indices, hoisted features and folded weights, against the fp32 MFMA kernel it replaces, and for its
independence of placement (persistent loop wrapped), its output range, graph capture, its fallback, its selection and its argument checks.

Tolerance: both kernels round only in their fp32 accumulations (every bf16 cross product is exact), in different orders.  The fp32 kernel's
own max error over the feature scale against float64 is MEASURED here on the same inputs; the split kernel gets twice that (the rule of
test_gpu_sa_bf16x9.py and test_gpu_sa_groupall_bf16x9.py).  Measured figures: profiles/sa_lds_bf16x9.txt."""
import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import genpose_oracle as go

NB = 5            # clouds of the shared batch; the last one consists of tiled duplicate points
BATCHES = (1, 2, 3, 5)
C2 = (64, 96)
NSS = (16, 32)
# no geometry of the kernel holds more waves per compute unit: at most two workgroups fit the LDS (>= 75 KB each), of at most 12 waves
MAX_WAVES_PER_CU = 24


@functools.lru_cache(maxsize=None)
def _setup():
    """One five-cloud pass of the fp32 encoder (its grouping, hoisted features and level-1 output) and the float64 reference of level 1 on
    those inputs - computed once, read-only afterwards."""
    from genpose_amd import synth
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd = go.make_state_dict(0, "score")
    e32 = Pointnet2EncoderHIP(sd, "cuda")
    pts = torch.from_numpy(synth.make_batch(NB, start=4321)).cuda().float()
    pts[NB - 1] = pts[NB - 1, :64].repeat(pts.shape[1] // 64, 1)  # tiled duplicates: every neighbourhood is full of repeated points
    f32, ws = e32.forward(pts, return_intermediates=True)
    ins = {"xyz": ws["new_xyz"][0].clone(), "new_xyz": ws["new_xyz"][1].clone(), "z": ws["z"][1].clone(),
           "idx": [t.clone() for t in ws["bq"][1]], "feat32": ws["feat"][1].clone(), "out32": f32.clone()}
    assert ins["xyz"].shape == (NB, 512, 3) and ins["z"].shape == (NB, 512, 128) and ins["new_xyz"].shape == (NB, 256, 3)
    assert [tuple(t.shape) for t in ins["idx"]] == [(NB, 256, 16), (NB, 256, 32)] and ins["feat32"].shape == (NB, 256, 256)
    assert [tuple(sc.couts) for sc in e32.w.levels[1]] == [(64, 64, 128), (64, 96, 128)]
    ref = _level1_fp64(ins, [sc._folded_plain for sc in e32.w.levels[1]])
    return sd, e32, pts, ins, ref


def _level1_fp64(ins, folded):
    """float64 on the host from the hoisted fp32 features z, the coordinates, the indices and the folded weights, layer 1 in the kernel's
    order: h1 = relu(z_j + (Wxyz (x_j - c) + b1)) -> relu(W2 h1 + b2) -> relu(max_j (W3 h2) + b3); -> [B, 256, 256]."""
    xyz, centres, z = ins["xyz"].double().cpu(), ins["new_xyz"].double().cpu(), ins["z"].double().cpu()
    B = xyz.shape[0]
    bi = torch.arange(B)[:, None, None]
    outs = []
    for i, ((W1, b1), (W2, b2), (W3, b3)) in enumerate(folded):
        W1, b1, W2, b2, W3, b3 = (t.double() for t in (W1, b1, W2, b2, W3, b3))  # W1 columns: [feat..., dx, dy, dz]
        idx = ins["idx"][i].long().cpu()
        d = xyz[bi, idx] - centres[:, :, None, :]
        h1 = torch.relu(z[bi, idx][..., 64 * i:64 * i + 64] + (d @ W1[:, -3:].t() + b1))
        h2 = torch.relu(h1 @ W2.t() + b2)
        outs.append(torch.relu((h2 @ W3.t()).max(dim=2)[0] + b3))
    return torch.cat(outs, dim=-1)


def _x9_args(sc, i, xyz, new_xyz, idx, z, out, packs=None):
    from genpose_amd._lib import ptr, stream_ptr
    (_, b1), _, _ = sc.layers
    w2, b2, w3, b3 = packs if packs is not None else sc.bf16x9_lds_packs()
    return [xyz.shape[0], 512, 256, NSS[i], 64, C2[i], 128, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(z), 128, 64 * i, ptr(sc.wxyz), ptr(b1), ptr(w2), ptr(b2),
            ptr(w3), ptr(b3), ptr(out), 256, 128 * i, stream_ptr()]


def _run(kind, sc, i, xyz, new_xyz, idx, z, out=None, sync=True):
    """Scale i of level 1 through the C entry point: kind 'f32' (gp_sa_pre_mlp_max_layout) | 'x9' (gp_sa_lds_bf16x9); -> the scale's
    [B, 256, 128] columns of a NaN-prefilled [B, 256, 256] output whose other half must stay NaN."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    B = xyz.shape[0]
    if out is None:
        out = torch.full((B, 256, 256), float("nan"), device="cuda")
    if kind == "f32":
        (_, b1), (w2, b2), (w3, b3) = sc.layers
        _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, B, 512, 256, NSS[i], 64, C2[i], 128, ptr(xyz), ptr(new_xyz), ptr(idx), ptr(z), 128, 64 * i,
                  ptr(sc.wxyz), ptr(b1), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 256, 128 * i, stream_ptr())
    else:
        _lib.call("gp_sa_lds_bf16x9", *_x9_args(sc, i, xyz, new_xyz, idx, z, out))
    if not sync:
        return out
    torch.cuda.synchronize()
    mine, other = out[..., 128 * i:128 * i + 128], out[..., 128 * (1 - i):128 * (1 - i) + 128]
    assert bool(torch.isfinite(mine).all())  # the scale's 128 columns are written whole ...
    assert bool(torch.isnan(other).all())    # ... and the other scale's are not touched
    return mine.clone()


def _first(ins, i, B):
    return [ins["xyz"][:B].contiguous(), ins["new_xyz"][:B].contiguous(), ins["idx"][i][:B].contiguous(), ins["z"][:B].contiguous()]


def test_against_float64_within_twice_the_fp32_kernels_error():
    sd, e32, pts, ins, ref = _setup()
    scale = float(ref.abs().max())
    rows = []
    for i, sc in enumerate(e32.w.levels[1]):
        for B in BATCHES:
            r = ref[:B, :, 128 * i:128 * i + 128]
            o32, o9 = _run("f32", sc, i, *_first(ins, i, B)), _run("x9", sc, i, *_first(ins, i, B))
            assert torch.equal(o32, ins["feat32"][:B, :, 128 * i:128 * i + 128])  # the anchor: the direct call is what the fp32 encoder ran
            rows.append((B, C2[i], NSS[i], float((o32.double().cpu() - r).abs().max()) / scale, float((o9.double().cpu() - r).abs().max()) / scale))
    e32_max = max(r[3] for r in rows)
    for B, c2, ns, a, b in rows:
        print(f"level 1, {B} cloud(s), 64-{c2}-128, ns = {ns}: max error / feature scale vs float64: fp32 MFMA {a:.3e}, bf16x9 {b:.3e}")
    print(f"fp32 MFMA kernel, max over the cases: {e32_max:.3e}; bound for bf16x9: {2 * e32_max:.3e}; bf16x9 max: {max(r[4] for r in rows):.3e}")
    assert 0 < e32_max < 3e-6  # the fp32 kernel is in its class, so the bound means something
    for B, c2, ns, a, b in rows:  # every case
        assert b <= 2 * e32_max, (B, c2, ns, a, b, e32_max)


@pytest.mark.parametrize("i", [0, 1])
def test_a_clouds_bits_do_not_depend_on_its_position_when_the_persistent_loop_wraps(i):
    sd, e32, pts, ins, ref = _setup()
    sc = e32.w.levels[1][i]
    units_per_cloud = 256 * NSS[i] // 32
    waves = torch.cuda.get_device_properties(0).multi_processor_count * MAX_WAVES_PER_CU
    n = -(-(waves + 1) // units_per_cloud)  # more 32-row units than the launched grid has waves: some wave takes a second unit
    assert n * units_per_cloud > waves
    sel = torch.arange(n, device="cuda") % 3
    singles = torch.cat([_run("x9", sc, i, *(t[c:c + 1].contiguous() for t in (ins["xyz"], ins["new_xyz"], ins["idx"][i], ins["z"]))) for c in range(3)])
    many = _run("x9", sc, i, *(t[sel].contiguous() for t in (ins["xyz"], ins["new_xyz"], ins["idx"][i], ins["z"])))
    for pos in (0, 1, 2, n // 2, n - 2, n - 1):  # first, middle, last - named, for the message
        assert torch.equal(many[pos], singles[int(sel[pos])]), (i, pos)
    assert torch.equal(many, singles[sel])   # and every copy
    # the tiled-duplicates cloud, in the middle of others
    c = NB - 1
    one = _run("x9", sc, i, *(t[c:c + 1].contiguous() for t in (ins["xyz"], ins["new_xyz"], ins["idx"][i], ins["z"])))
    order = torch.tensor([c, 1, c, 2, c], device="cuda")
    five = _run("x9", sc, i, *(t[order].contiguous() for t in (ins["xyz"], ins["new_xyz"], ins["idx"][i], ins["z"])))
    for pos in (0, 2, 4):
        assert torch.equal(five[pos], one[0]), (i, pos)


def test_capture_and_replay_give_the_launched_bits():
    sd, e32, pts, ins, ref = _setup()
    for i, sc in enumerate(e32.w.levels[1]):
        args = _first(ins, i, NB)
        direct = _run("x9", sc, i, *args)
        out = torch.full((NB, 256, 256), float("nan"), device="cuda")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            _run("x9", sc, i, *args, out=out, sync=False)
        for _ in range(2):  # capture + replay, then a second replay
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[..., 128 * i:128 * i + 128], direct) and bool(torch.isnan(out[..., 128 * (1 - i):128 * (1 - i) + 128]).all())


def test_unsplittable_weight_keeps_the_fp32_kernel_for_that_scale():
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd, e32, pts, ins, ref = _setup()
    bad = dict(sd)
    key = "pts_encoder.SA_modules.1.mlps.0.layer1.conv.weight"
    W = bad[key].clone()
    W[7, 11] = 1e-40  # subnormal: its bf16 terms lie below the normal range, the matrix pipe may flush them
    bad[key] = W
    eb, ef = Pointnet2EncoderHIP(bad, "cuda", level1="bf16x9"), Pointnet2EncoderHIP(bad, "cuda")
    eb.LEVEL1_BF16X9_MIN_CLOUDS = 1
    assert eb.sa_kernels[(1, 0)] == "f32mfma" and eb.sa_kernels[(1, 1)] == "bf16x9"
    assert set(ef.sa_kernels.values()) == {"f32mfma"}
    (_, wb), (_, wf) = eb.forward(pts, return_intermediates=True), ef.forward(pts, return_intermediates=True)
    assert torch.equal(wb["feat"][1][..., :128], wf["feat"][1][..., :128])
    assert not torch.equal(wb["feat"][1][..., 128:], wf["feat"][1][..., 128:])


def test_selection_by_agent_kind_direct_construction_and_threshold():
    from genpose_amd.config import get_config
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from genpose_amd.posenet_agent import PoseNet
    sd, e32, pts, ins, ref = _setup()
    assert e32.level1 == "f32mfma" and set(e32.sa_kernels.values()) == {"f32mfma"} and get_config().encoder_level1 == "auto"
    for cfg, want in ((get_config(sampler_mode=["pc"]), "bf16x9"), (get_config(sampler_mode=["ode"]), "f32mfma"),
                      (get_config(sampler_mode=["heun"], sampling_steps=8), "f32mfma"), (get_config(sampler_mode=["dpm2m"], sampling_steps=8), "f32mfma"),
                      (get_config(sampler_mode=["pc"], encoder_level1="f32mfma"), "f32mfma"), (get_config(sampler_mode=["ode"], encoder_level1="bf16x9"), "bf16x9")):
        a = PoseNet(cfg)
        a.load_state_dict(sd)
        e = a.net.pts_encoder
        assert e.level1 == want and e.sa_kernels[(1, 0)] == e.sa_kernels[(1, 1)] == want, (cfg.sampler_mode, want)
        assert e.sa_kernels[(0, 0)] == e.sa_kernels[(0, 1)] == "f32mfma"
    with pytest.raises(ValueError):
        Pointnet2EncoderHIP(sd, "cuda", level1="fp8")
    # unchanged: the class default and precision = 'bf16x9' (level 2 only)
    e9 = Pointnet2EncoderHIP(sd, "cuda", precision="bf16x9")
    assert e9.level1 == "f32mfma" and all(v == ("bf16x9" if k[0] == 2 else "f32mfma") for k, v in e9.sa_kernels.items())
    assert torch.equal(e9.forward(pts, return_intermediates=True)[1]["feat"][1], ins["feat32"])
    # level1 = 'bf16x9': the encoder runs what the entry point computes, from its threshold upward; below it the fp32 kernels' bits
    e1 = Pointnet2EncoderHIP(sd, "cuda", level1="bf16x9")
    assert e1.precision == "f32" and e1.level3_kernel == "f32mfma"
    assert {k: v for k, v in e1.sa_kernels.items() if v != "f32mfma"} == {(1, 0): "bf16x9", (1, 1): "bf16x9"}
    e1.LEVEL1_BF16X9_MIN_CLOUDS = 1
    f1, w1 = e1.forward(pts, return_intermediates=True)
    assert torch.equal(w1["feat"][0], e32.forward(pts, return_intermediates=True)[1]["feat"][0])
    for i, sc in enumerate(e32.w.levels[1]):
        x9 = _run("x9", sc, i, *_first(ins, i, NB))
        assert torch.equal(w1["feat"][1][..., 128 * i:128 * i + 128], x9) and not torch.equal(x9, ins["feat32"][..., 128 * i:128 * i + 128])
    assert not torch.equal(f1, ins["out32"])
    e1.LEVEL1_BF16X9_MIN_CLOUDS = NB + 1
    fb, wb = e1.forward(pts, return_intermediates=True)
    assert torch.equal(wb["feat"][1], ins["feat32"]) and torch.equal(fb, ins["out32"])


def test_bad_arguments_are_refused():
    from genpose_amd import _lib
    sd, e32, pts, ins, ref = _setup()
    fn = _lib.lib().gp_sa_lds_bf16x9
    EINVAL = -1
    for i, sc in enumerate(e32.w.levels[1]):
        out = torch.full((NB, 256, 256), float("nan"), device="cuda")
        good = _x9_args(sc, i, *_first(ins, i, NB), out)

        def changed(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return fn(*a)

        assert changed(a0=0) == 0                                   # b = 0: nothing to do
        assert changed(a0=-1) == EINVAL and changed(a1=0) == EINVAL and changed(a2=0) == EINVAL
        assert changed(a3=NSS[1 - i]) == EINVAL                     # the other scale's neighbourhood size: not instantiated
        assert changed(a4=128) == EINVAL and changed(a5=C2[i] + 32) == EINVAL and changed(a6=256) == EINVAL  # c1, c2, c3
        assert changed(a0=1, a2=1, a3=16 if i == 0 else 8) == EINVAL  # not whole 32-row units
        for k in (7, 8, 9, 10, 13, 14, 15, 16, 17, 18, 19):           # every pointer
            assert changed(**{f"a{k}": None}) == EINVAL, k
        assert changed(a11=130) == EINVAL and changed(a11=32) == EINVAL and changed(a12=2) == EINVAL and changed(a12=-4) == EINVAL and changed(a12=68) == EINVAL  # zstride, zoff
        assert changed(a20=254) == EINVAL and changed(a21=2) == EINVAL and changed(a21=-4) == EINVAL and changed(a21=132) == EINVAL  # cout_total, cout_off
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all())  # none of them launched
