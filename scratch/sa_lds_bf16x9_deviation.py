"""Deviation record (not a gate) for encoder level 1 as exact-product split bf16: PC-100 on one 64 x 50 batch with injected prior and noise
(the draws of bench.py's split-bf16 leg, seed 5), config.encoder_level1 'f32mfma' against 'bf16x9', everything else equal.

    python scratch/sa_lds_bf16x9_deviation.py"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    from genpose_amd import synth
    from genpose_amd.config import get_config
    from genpose_amd.pipeline import PipelinedPCPredictor
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.weights_synth import make_state_dict
    B, K, n, dev = 64, 50, 100, "cuda"
    pts = torch.from_numpy(synth.make_batch(B, start=0)).to(dev)
    gen = torch.Generator().manual_seed(5)
    R1 = B * K
    priors = [torch.randn(R1, 9, generator=gen).to(dev)]
    noises = [(torch.randn(n, R1, 9, generator=gen).to(dev), torch.randn(n, R1, 9, generator=gen).to(dev))]
    outs, feats = {}, {}
    for lvl1 in ("f32mfma", "bf16x9"):
        agent = PoseNet(get_config(device=dev, posenet_mode="score", sampler_mode=["pc"], sampling_steps=n, encoder_level1=lvl1))
        agent.load_state_dict(make_state_dict(0, "score"))
        enc = agent.net.pts_encoder
        assert B >= enc.LEVEL1_BF16X9_MIN_CLOUDS and enc.sa_kernels[(1, 0)] == enc.sa_kernels[(1, 1)] == lvl1
        feats[lvl1] = enc.forward(pts).clone()
        pipe = PipelinedPCPredictor(agent, B, K, n, batches_per_launch=1, overlap=False)
        outs[lvl1] = torch.stack([o.clone() for o in pipe.run([pts], prior_noise=priors, noise=noises)])
        torch.cuda.synchronize()
    f32, f9 = feats["f32mfma"], feats["bf16x9"]
    print(f"encoder features, {B} clouds: max |diff| / scale {float((f9 - f32).abs().max()) / float(f32.abs().max()):.2e}")
    ref, got = outs["f32mfma"], outs["bf16x9"]
    rot = (got[..., :6] - ref[..., :6]).abs().reshape(-1)
    tr = (got[..., 6:] - ref[..., 6:]).abs().max() / ref[..., 6:].abs().max()
    rq = torch.quantile(rot.float(), torch.tensor([0.5, 0.99, 0.999], device=rot.device))
    print(f"rotation |diff|: median {float(rq[0]):.1e}, p99 {float(rq[1]):.1e}, p99.9 {float(rq[2]):.1e}, max {float(rot.max()):.1e}; "
          f"translation max / scale {float(tr):.1e}")
    print("Beside it: two fp32 launch plans of one batch differ by p99.9 2.6e-5 / max 7e-3 (tests/test_gpu_fullsize.py).")


if __name__ == "__main__":
    main()
