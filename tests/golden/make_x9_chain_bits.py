"""Generator of tests/golden/x9_chain_bits.npz: inputs and outputs of the library's own bf16x9 chain kernels (128-row workgroups) on
seeded random weights, recorded BEFORE the trunk's heads went chunk-major.  tests/test_gpu_x9_chain_bits.py replays compute() on the
recorded inputs and asserts equal bits on every array.

    python tests/golden/make_x9_chain_bits.py        (on an MI355X; rewrites the fixture from the tree it runs in)

Cases (clouds, candidates, batches):
  pc_a    PCSampler (3, 43, 1): 129 rows - a second workgroup with one real row, workgroups spanning several clouds
  pc_b    PCSampler (4, 64, 2): two batches of one 128-row workgroup each, two clouds per workgroup (with several batches per launch
          the chain plan admits whole workgroups only, gp_pc_layout: a ragged one exists with one batch alone, pc_a)
  pc_s    PCSampler (3, 43, 1) with sampler_seed: the noise drawn inside the step kernel
  heun    HeunSampler (3, 43), 2 steps
  ode     ODESampler(trunk='bf16x9') (3, 43), one solve from T0 = 0.2
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "x9_chain_bits.npz")
PC_STEPS, HEUN_STEPS, ODE_T0, SEED = 3, 2, 0.2, 20240917
CASES = {"pc_a": (3, 43, 1), "pc_b": (4, 64, 2), "pc_s": (3, 43, 1), "heun": (3, 43, 1), "ode": (3, 43, 1)}


def _net():
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    return ScoreNetHIP(make_state_dict(0, "score"), "cuda")


def make_inputs():
    """As tests/test_gpu_bf16x9.py::_inputs, per case; cvec comes from the library's cloud embedding and is recorded as an input."""
    net = _net()
    inp = {}
    for i, (case, (B, K, _)) in enumerate(CASES.items()):
        g = torch.Generator().manual_seed(B + K + i)
        feat = torch.randn(B, 1024, generator=g).abs()
        centre = torch.randn(B, 3, generator=g) * 0.3
        x0 = torch.randn(B * K, 9, generator=g) * 50.0
        z1, z2 = torch.randn(PC_STEPS, B * K, 9, generator=g), torch.randn(PC_STEPS, B * K, 9, generator=g)
        if case == "ode":
            x0 = x0 * 1e-3  # a state at T0 = 0.2, where sigma is 0.055
        inp[f"{case}.cvec"] = net.cloud_embed(feat.cuda()).cpu().numpy()
        inp[f"{case}.centre"], inp[f"{case}.x0"] = centre.numpy(), x0.numpy()
        if case in ("pc_a", "pc_b"):
            inp[f"{case}.z1"], inp[f"{case}.z2"] = z1.numpy(), z2.numpy()
    return inp


def compute(inp):
    """The recorded outputs, from the recorded inputs, on the tree this runs in."""
    from genpose_amd.samplers import HeunSampler, ODESampler, PCSampler
    net = _net()
    dev = lambda case, name: torch.from_numpy(inp[f"{case}.{name}"]).cuda()
    out = {}
    for case in ("pc_a", "pc_b", "pc_s"):
        B, K, groups = CASES[case]
        kw = {"seed": SEED} if case == "pc_s" else {}
        smp = PCSampler(net, B, K, PC_STEPS, "cuda", groups=groups, tile=128, trunk="bf16x9", record_traj=True, use_graph=False, **kw)
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
    B, K, _ = CASES["ode"]
    smp = ODESampler(net, B, K, "cuda", tile=128, trunk="bf16x9")
    assert smp.trunk == "bf16x9"
    _, poses = smp.run(dev("ode", "cvec"), dev("ode", "centre"), dev("ode", "x0"), ODE_T0)
    torch.cuda.synchronize()
    out["ode.out.poses"] = poses.cpu().numpy()
    out["ode.out.nfev"] = np.array([int(smp.last_stats["nfev"])], dtype=np.int64)
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
    print(f"{dest}: {len(inputs)} inputs, {len(outputs)} outputs, {os.path.getsize(dest)} bytes; nfev {outputs['ode.out.nfev'][0]}")
