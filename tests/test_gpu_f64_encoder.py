"""GPU: the PointNet++ encoder against a FLOAT64 encoder (tests/f64_reference.py: encoder64), level 0 included and end to end.

Levels 1-3 of the fp32 encoder have float64 checks on their own inputs (the split-bf16 test files); level 0 (sa0_chain: a three-channel
input padded into an MFMA k-block) had none, nor had the pass as a whole, from state dict to the 1024 features.  Here the float64 encoder
runs from the UNFOLDED state dict (conv, eval-mode BatchNorm, ReLU, max) on the fp32 oracle's FPS and ball-query indices, so the fold of
BatchNorm into the weights, the hoisted first layers and the error carried from level to level are all part of what is tested.

The rule is test_gpu_f64_score.py's: E_oracle = the fp32 CPU oracle's (encoder_forward) own error against the float64 encoder, per level
and block, maximised over the clouds; a device result passes at <= MARGIN x E_oracle (MARGIN = 3, fixed before any measurement).  Blocks:
the two scales of level 0 (the 32-column scale must not hide behind the 64-column one), each later level whole, the 1024 features whole.
The split-bf16 configurations get the SAME bound as fp32: that is the project's claim for them.

Clouds: synth.make_batch(3, start=4321) and the tiled-duplicates cloud of the split-bf16 level tests.  Weights: seed 0, the stress state
dict of test_gpu_weight_seeds.py, the encoder inside tests/golden/trained/ckpt_score.pth.  Every cell is printed (pytest -s);
profiles/f64_gate.txt keeps a run."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import f64_reference as fr


def _configs(sd):
    """name -> (encoder, the kernels it must report)"""
    from genpose_amd.encoder import Pointnet2EncoderHIP
    named = Pointnet2EncoderHIP(sd, "cuda", precision="f32", level1="f32mfma", level3="f32mfma")
    default = Pointnet2EncoderHIP(sd, "cuda")
    split = Pointnet2EncoderHIP(sd, "cuda", precision="bf16x9", level1="bf16x9", level3="bf16x9")
    split.LEVEL1_BF16X9_MIN_CLOUDS = split.LEVEL3_BF16X9_MIN_CLOUDS = 1
    return {"f32 by name": named, "class defaults": default, "all split-bf16": split}


def _gate(tag, which, what, block, eo, ed, bad):
    print(f"f64gate | {tag:22s} | {which:7s} | {what:14s} b{block} | oracle {eo:.2e} | device {ed:.2e} | ratio {ed / eo:6.3f}")
    assert 0 < eo < fr.ORACLE_CEILING
    if not ed <= fr.MARGIN * eo:
        bad.append((tag, which, what, block, eo, ed, round(ed / eo, 3)))


def _check_pass(tag, which, enc, c, bad):
    """one device pass over the case's clouds: grouping equal to the oracle's, every level and the features under the rule"""
    cfg, inter = c["cfg"], c["inter"]
    feat, ws = enc.forward(c["pts"].cuda(), return_intermediates=True)
    torch.cuda.synchronize()
    nlev = sum(1 for n in cfg["npoints"] if n is not None)
    for k in range(nlev):  # a feature error cannot be blamed on grouping
        assert np.array_equal(ws["fps_idx"][k].cpu().numpy(), inter[k]["fps_idx"]), (tag, which, k)
        assert np.array_equal(ws["new_xyz"][k].cpu().numpy(), inter[k]["new_xyz"]), (tag, which, k)
        for i in range(len(cfg["radii"][k])):
            assert np.array_equal(ws["bq"][k][i].cpu().numpy(), inter[k][f"bq_idx{i}"]), (tag, which, k, i)
    levels = [ws["feat"][k].cpu().transpose(1, 2) for k in range(len(cfg["npoints"]))]  # point-major [B,n,C] -> [B,C,n]
    per_cloud = fr.encoder_errors(levels, c["levels64"], cfg)
    for k, lv in enumerate(per_cloud):
        for j in range(len(lv[0])):
            _gate(tag, which, f"level {k}", j, c["e_levels"][k][j], max(cl[j] for cl in lv), bad)
    out = feat.cpu()
    e_dev = max(fr.block_error(out[b:b + 1], c["out64"][b:b + 1], None)[0] for b in range(out.shape[0]))
    _gate(tag, which, "1024 features", 0, c["e_out"], e_dev, bad)


@pytest.mark.parametrize("which", fr.ENCODER_WEIGHTS)
def test_encoder_levels_and_features(which):
    """four clouds through the fp32 kernels asked for by name, the class defaults and the all-split configuration (both *_MIN_CLOUDS
    thresholds set to 1 on the instance): centres and indices equal the oracle's, level 0's two scales, levels 1-3 and the 1024 features
    within MARGIN x the oracle's own error"""
    c = fr.encoder_case(which)
    bad = []
    for tag, enc in _configs(c["sd"]).items():
        if tag == "all split-bf16":
            # (a scale whose folded weights do not split into three normal bf16 terms keeps its fp32 kernel: the seeded weights all
            # split; for the others the levels that did are part of the printed name)
            split = sorted({k[0] for k, v in enc.sa_kernels.items() if v == "bf16x9"}) + ([3] if enc.level3_kernel == "bf16x9" else [])
            assert which != "seed0" or split == [1, 2, 3]
            assert enc.launch_plan(4)[-1] == ("gp_sa_groupall_bf16x9" if 3 in split else "gp_sa_pre_mlp_max_layout")
            tag = f"split-bf16 L{''.join(map(str, split))}"
        else:
            assert set(enc.sa_kernels.values()) == {"f32mfma"} and enc.level3_kernel == "f32mfma"
        _check_pass(tag, which, enc, c, bad)
    assert not bad, bad


def test_dense_encoder_on_one_cloud():
    """params='dense' (neighbourhoods of 8 to 64 samples) on one cloud, seed-0 weights"""
    from genpose_amd.encoder import Pointnet2EncoderHIP
    c = fr.encoder_case("seed0", "dense", 1)
    bad = []
    _check_pass("dense", "seed0", Pointnet2EncoderHIP(c["sd"], "cuda", "dense"), c, bad)
    assert not bad, bad
