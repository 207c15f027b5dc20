"""Generator of tests/golden/x9_chain_bits_more.npz: inputs and outputs of the library's own bf16x9 chain kernels (128-row workgroups) on
seeded random weights, on the shapes x9_chain_bits.npz does not have - a workgroup whose rows span all NCL = 4 staged clouds, and
workgroups with fewer than 128 live rows - recorded BEFORE the staged fp32 operands were requested ahead of the sampler update and the
k-major layers' splits and tails went between the MFMAs.  tests/test_gpu_x9_chain_bits_more.py replays compute() on the recorded inputs
and asserts equal bits on every array.

    python tests/golden/make_x9_chain_bits_more.py        (on an MI355X; rewrites the fixture from the tree it runs in)

Cases (clouds, candidates, batches):
  pc_w    PCSampler (6, 43, 1), 4 steps: 258 rows - workgroup 1 (rows 128-255) spans clouds 2, 3, 4, 5, all four staged rows of
          cvec + tvec (43 is the smallest k the chain plan admits); workgroup 2 has two live rows and a clamped last cloud
  pc_one  PCSampler (1, 50, 1), 4 steps: 50 rows - one workgroup, 78 clamped duplicate rows, two waves with no live row
  pc_s    PCSampler (6, 43, 1) with seed=, 2 steps: the noise drawn inside the step kernel
  heun    HeunSampler (6, 43), 2 steps
pc_w, pc_s and heun share one set of inputs (`w.*`).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "x9_chain_bits_more.npz")
PC_STEPS, SEEDED_STEPS, HEUN_STEPS, SEED = 4, 2, 2, 20241019
CASES = {"pc_w": (6, 43, 1), "pc_one": (1, 50, 1), "pc_s": (6, 43, 1), "heun": (6, 43, 1)}
INPUTS = {"pc_w": "w", "pc_one": "one", "pc_s": "w", "heun": "w"}  # case -> its input set
MAX_BYTES = 300 * 1000


def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    return ScoreNetHIP(make_state_dict(0, "score"), "cuda")


def make_inputs():
    """As tests/golden/make_x9_chain_bits.py, per input set; cvec comes from the library's cloud embedding and is recorded as an input."""
    net = _net()
    inp = {}
    for i, (name, case) in enumerate((("w", "pc_w"), ("one", "pc_one"))):
        B, K, _ = CASES[case]
        g = torch.Generator().manual_seed(1000 + B + K + i)
        feat = torch.randn(B, 1024, generator=g).abs()
        centre = torch.randn(B, 3, generator=g) * 0.3
        x0 = torch.randn(B * K, 9, generator=g) * 50.0
        z1, z2 = torch.randn(PC_STEPS, B * K, 9, generator=g), torch.randn(PC_STEPS, B * K, 9, generator=g)
        inp[f"{name}.cvec"] = net.cloud_embed(feat.cuda()).cpu().numpy()
        inp[f"{name}.centre"], inp[f"{name}.x0"] = centre.numpy(), x0.numpy()
        inp[f"{name}.z1"], inp[f"{name}.z2"] = z1.numpy(), z2.numpy()
    return inp


def compute(inp):
    """The recorded outputs, from the recorded inputs, on the tree this runs in."""
    from genpose_amd.samplers import HeunSampler, PCSampler
    net = _net()
    dev = lambda case, name: torch.from_numpy(inp[f"{INPUTS[case]}.{name}"]).cuda()
    out = {}
    for case in ("pc_w", "pc_one", "pc_s"):
        B, K, groups = CASES[case]
        kw, steps = ({"seed": SEED}, SEEDED_STEPS) if case == "pc_s" else ({}, PC_STEPS)
        smp = PCSampler(net, B, K, steps, "cuda", groups=groups, tile=128, trunk="bf16x9", record_traj=True, use_graph=False, **kw)
        assert smp.tile == 128 and smp.kernel_name == "pc_step_chain_kernel<bf16x9>"
        if case == "pc_s":
            smp.run(dev(case, "cvec"), dev(case, "centre"), dev(case, "x0"), run_index=0)
        else:
            smp.run(dev(case, "cvec"), dev(case, "centre"), dev(case, "x0"), dev(case, "z1"), dev(case, "z2"))
        torch.cuda.synchronize()
        for name in ("x", "mean_x", "score", "partials", "traj"):
            out[f"{case}.out.{name}"] = getattr(smp, name).cpu().numpy()
    B, K, _ = CASES["heun"]
    smp = HeunSampler(net, B, K, HEUN_STEPS, "cuda", tile=128, use_graph=False)
    assert smp.kernel_name == "heun_step_chain_kernel<bf16x9>"
    smp.run(dev("heun", "cvec"), dev("heun", "centre"), dev("heun", "x0"))
    torch.cuda.synchronize()
    for name in ("x", "score", "out"):
        out[f"heun.out.{name}"] = getattr(smp, name).cpu().numpy()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    dest = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    inputs = make_inputs()
    outputs = compute(inputs)
    again = compute(inputs)
    for k in outputs:
        assert np.array_equal(outputs[k], again[k]), f"{k}: not reproducible on one tree"
        assert np.isfinite(outputs[k]).all(), k
    np.savez_compressed(dest, **inputs, **outputs)
    size = os.path.getsize(dest)
    assert size < MAX_BYTES, f"{dest}: {size} bytes"
    print(f"{dest}: {len(inputs)} inputs, {len(outputs)} outputs, {size} bytes")
