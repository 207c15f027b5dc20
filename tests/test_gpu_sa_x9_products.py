"""GPU: the three encoder kernels of the bf16x9 family form EIGHT of the nine products of the split (csrc/bf16x9.h, NPROD = 8: lo.lo, at
most 2^-32 |a b| per multiply, is not issued) - gp_sa_lds_bf16x9 (level 1), gp_sa_pre_mlp_max_bf16x9 (level 2), gp_sa_groupall_bf16x9
(level 3).  Held here, on the inputs, references and helpers of their own test files (an fp32 encoder pass over
synth.make_batch(5, start=4321); 1, 2, 3 and 5 clouds):
  - the error against float64 stays within the project's rule for these kernels, twice the fp32 kernel's own maximum on the same inputs
    (what is not formed is 1 / 256 of an fp32 roundoff of one product: the figures are expected to be those of nine products,
    profiles/sa_x9_products.txt);
  - a cloud's features depend neither on the batch nor on its position, also where the persistent loops wrap;
  - capture + two replays give the launched bits;
  - nothing else moved: the fp32 kernels' bits, and the PC / Heun / RK45 chain kernels' recorded bits (all nine products)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_sa_bf16x9 as l2
import test_gpu_sa_groupall_bf16x9 as l3
import test_gpu_sa_lds_bf16x9 as l1

NB, BATCHES = 5, (1, 2, 3, 5)
assert (l1.NB, l2.NB, l3.NB) == (NB, NB, NB) and l1.BATCHES == l2.BATCHES == l3.BATCHES == BATCHES
L2_WAVES_PER_CU = 8  # sa_bf16x9.hip: one persistent 8-wave workgroup per compute unit


def _l1_runs(kind, B):
    sd, e32, pts, ins, ref = l1._setup()
    return torch.cat([l1._run(kind, sc, i, *l1._first(ins, i, B)) for i, sc in enumerate(e32.w.levels[1])], dim=-1)


def _l2_runs(kind, B, ins=None):
    sd, e32, e9, pts, ins0, ref = l2._setup()
    enc = e32 if kind == "f32" else e9
    return torch.cat([l2._run(kind, sc, i, ins0 if ins is None else ins, B) for i, sc in enumerate(enc.w.levels[2])], dim=-1)


def _l3_runs(kind, B):
    sd, e32, pts, ins, ref = l3._setup()
    xyz, feat = ins["xyz"][:B].contiguous(), ins["feat"][:B].contiguous()
    return l3._run_f32(e32, xyz, feat) if kind == "f32" else l3._run_x9(e32, xyz, feat)


LEVELS = {1: (_l1_runs, lambda: l1._setup()[4], 128), 2: (_l2_runs, lambda: l2._setup()[5], 256), 3: (_l3_runs, lambda: l3._setup()[4], 512)}


@pytest.mark.parametrize("level", [1, 2, 3])
def test_error_against_float64_within_twice_the_fp32_kernels(level):
    runs, get_ref, width = LEVELS[level]
    ref = get_ref()
    scale = float(ref.abs().max())
    rows = []
    for B in BATCHES:
        o32, o9 = runs("f32", B).double().cpu(), runs("x9", B).double().cpu()
        assert o32.shape == o9.shape == ref[:B].shape and not torch.equal(o32, o9)
        for i in range(2):  # per scale: the columns of one launch (level 3: of one scale's items)
            cols = slice(width * i, width * (i + 1))
            rows.append((B, i, float((o32[..., cols] - ref[:B][..., cols]).abs().max()) / scale, float((o9[..., cols] - ref[:B][..., cols]).abs().max()) / scale))
    e32_max = max(r[2] for r in rows)
    for B, i, a, b in rows:
        print(f"level {level}, {B} cloud(s), scale {i}: max error / feature scale vs float64: fp32 kernel {a:.3e}, bf16x9 with eight products {b:.3e}")
    print(f"level {level}: fp32 max over the cases {e32_max:.3e}; bound {2 * e32_max:.3e}; eight products, max {max(r[3] for r in rows):.3e}")
    assert 0 < e32_max < 3e-6  # the fp32 kernel is in its class, so the bound means something
    for B, i, a, b in rows:  # every case
        assert b <= 2 * e32_max, (level, B, i, a, b, e32_max)


@pytest.mark.parametrize("level", [1, 2, 3])
def test_a_clouds_features_do_not_depend_on_the_batch(level):
    runs = LEVELS[level][0]
    five = runs("x9", NB)
    for B in BATCHES[:-1]:  # 1, 2 and 3 clouds alone against the same clouds inside 5 (level 3: another split of the items over workgroups)
        assert torch.equal(runs("x9", B), five[:B]), (level, B)


def test_level3_position_inside_the_batch():
    sd, e32, pts, ins, ref = l3._setup()
    three = l3._run_x9(e32, ins["xyz"][:3].contiguous(), ins["feat"][:3].contiguous())
    order = torch.tensor([3, 0, 4, 1, 2], device="cuda")  # the three clouds at other positions, other clouds between them
    five = l3._run_x9(e32, ins["xyz"][order].contiguous(), ins["feat"][order].contiguous())
    assert torch.equal(five[[1, 3, 4]], three)


@pytest.mark.parametrize("i", [0, 1])
def test_level2_position_when_the_persistent_loop_wraps(i):
    sd, e32, e9, pts, ins, ref = l2._setup()
    sc = e9.w.levels[2][i]
    ns = ins["idx"][i].shape[-1]
    units_per_cloud = 128 * ns // 32
    waves = torch.cuda.get_device_properties(0).multi_processor_count * L2_WAVES_PER_CU
    n = -(-(waves + 1) // units_per_cloud)  # more 32-row units than the launched grid has waves: some wave takes a second unit
    assert n * units_per_cloud > waves
    sel = torch.arange(n, device="cuda") % 3

    def pick(s):
        return {k: ([t[s].contiguous() for t in v] if k == "idx" else v[s].contiguous()) for k, v in ins.items()}

    singles = torch.cat([l2._run("x9", sc, i, pick(slice(c, c + 1)), 1) for c in range(3)])
    many = l2._run("x9", sc, i, pick(sel), n)
    for pos in (0, 1, 2, n // 2, n - 2, n - 1):  # first, middle, last - named, for the message
        assert torch.equal(many[pos], singles[int(sel[pos])]), (i, pos)
    assert torch.equal(many, singles[sel])
    # the tiled-duplicates cloud between others
    c = NB - 1
    order = torch.tensor([c, 1, c, 2, c], device="cuda")
    one, five = l2._run("x9", sc, i, pick(slice(c, c + 1)), 1), l2._run("x9", sc, i, pick(order), 5)
    for pos in (0, 2, 4):
        assert torch.equal(five[pos], one[0]), (i, pos)


def _replays(launch, out, direct):
    """launch(out) captured; capture + replay, then a second replay, each into a NaN-filled `out`: the bits of `direct` where it is finite,
    NaN (untouched) elsewhere."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(out)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(out), torch.isnan(direct)) and torch.equal(torch.nan_to_num(out), torch.nan_to_num(direct))


def test_capture_and_two_replays_give_the_launched_bits():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    # level 1, scale by scale
    sd, e32, pts, ins, ref = l1._setup()
    for i, sc in enumerate(e32.w.levels[1]):
        args = l1._first(ins, i, NB)
        direct = torch.full((NB, 256, 256), float("nan"), device="cuda")
        direct[..., 128 * i:128 * i + 128] = l1._run("x9", sc, i, *args)
        _replays(lambda out: l1._run("x9", sc, i, *args, out=out, sync=False), torch.full((NB, 256, 256), float("nan"), device="cuda"), direct)
    # level 2, scale by scale (the entry point as test_gpu_sa_bf16x9._run calls it, without its synchronisation)
    sd, e32, e9, pts, ins, ref = l2._setup()
    for i, sc in enumerate(e9.w.levels[2]):
        (_, b1), _, _ = sc.layers
        w, b2p, b3p = sc.bf16x9_packs()
        direct = torch.full((NB, 128, 512), float("nan"), device="cuda")
        direct[..., 256 * i:256 * i + 256] = l2._run("x9", sc, i, ins, NB)

        def launch(out):
            _lib.call("gp_sa_pre_mlp_max_bf16x9", NB, 256, 128, ins["idx"][i].shape[-1], 128, 196, 256, ptr(ins["xyz"]), ptr(ins["new_xyz"]), ptr(ins["idx"][i]),
                      ptr(ins["z"]), 256, 128 * i, ptr(sc.wxyz), ptr(b1), ptr(w), ptr(b2p), ptr(b3p), ptr(out), 512, 256 * i, stream_ptr())

        _replays(launch, torch.full((NB, 128, 512), float("nan"), device="cuda"), direct)
    # level 3, both scales in one launch
    sd, e32, pts, ins, ref = l3._setup()
    direct = l3._run_x9(e32, ins["xyz"], ins["feat"]).clone()
    _replays(lambda out: l3._run_x9(e32, ins["xyz"], ins["feat"], out=out, sync=False), torch.full((NB, 1024), float("nan"), device="cuda"), direct)


def test_fp32_kernels_bits_are_unchanged():
    from genpose_amd.encoder import Pointnet2EncoderHIP
    sd, e32, pts, ins, ref = l1._setup()
    f32, w32 = e32.forward(pts, return_intermediates=True)
    want = [t.clone() for t in w32["feat"]]
    assert torch.equal(f32, ins["out32"])
    # asked for by name: the class defaults
    ef = Pointnet2EncoderHIP(sd, "cuda", precision="f32", level1="f32mfma", level3="f32mfma")
    assert set(ef.sa_kernels.values()) == {"f32mfma"} and ef.level3_kernel == "f32mfma"
    ff, wf = ef.forward(pts, return_intermediates=True)
    assert torch.equal(ff, f32) and all(torch.equal(a, b) for a, b in zip(wf["feat"], want))
    # all three split kernels, thresholds set to 1 on the instance: every level from 1 up runs eight products ...
    e9 = Pointnet2EncoderHIP(sd, "cuda", precision="bf16x9", level1="bf16x9", level3="bf16x9")
    e9.LEVEL1_BF16X9_MIN_CLOUDS = e9.LEVEL3_BF16X9_MIN_CLOUDS = 1
    assert {k[0] for k, v in e9.sa_kernels.items() if v == "bf16x9"} == {1, 2} and e9.level3_kernel == "bf16x9"
    f9, w9 = e9.forward(pts, return_intermediates=True)
    got = [t.clone() for t in w9["feat"]]
    assert torch.equal(got[0], want[0])                              # ... level 0 (fp32 kernels) has the fp32 encoder's bits,
    assert torch.equal(got[1], _l1_runs("x9", NB)) and not torch.equal(got[1], want[1])   # level 1 is the entry point's output on them,
    assert not torch.equal(got[2], want[2]) and not torch.equal(f9, f32)
    # ... and with the thresholds above the batch the same instance runs the fp32 kernels at levels 1 and 3, bit for bit
    e9.LEVEL1_BF16X9_MIN_CLOUDS = e9.LEVEL3_BF16X9_MIN_CLOUDS = NB + 1
    fb, wb = e9.forward(pts, return_intermediates=True)
    assert torch.equal(wb["feat"][0], want[0]) and torch.equal(wb["feat"][1], want[1])
    # the fp32 entry points, called directly on the fp32 encoder's intermediates
    assert torch.equal(_l1_runs("f32", NB), want[1]) and torch.equal(_l2_runs("f32", NB), want[2]) and torch.equal(_l3_runs("f32", NB), f32)


def test_chain_kernels_still_give_their_recorded_bits(golden):
    """The score trunks keep all nine products: the PC / seeded PC / Heun / RK45 chain kernels reproduce tests/golden/x9_chain_bits.npz
    (the replay is test_gpu_x9_chain_bits.py's, the goldens stay where they are)."""
    import test_gpu_x9_chain_bits as bits
    rec = golden("x9_chain_bits.npz")
    new = bits._generator().compute({k: v for k, v in rec.items() if ".out." not in k})
    names = sorted(k for k in rec if ".out." in k)
    assert names and {k.split(".out.")[0] for k in names} == set(bits.CASES)
    for k in names:
        assert rec[k].dtype == new[k].dtype and rec[k].shape == new[k].shape and np.array_equal(rec[k], new[k]), k
