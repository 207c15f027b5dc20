"""One full PC pass (100 steps) at the benched shape - 64 clouds x 50 candidates per batch, ten batches per launch, 32 000 rows - with the
two normal_() launches of the default path inside the timed region, against the seeded path (noise drawn in the step kernels).
HIP events, warm-up, median [min, max] over --reps repeats, the two paths interleaved in one session.

    python scratch/seeded_noise_time.py [--reps 9] [--out FILE]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from genpose_amd.samplers import PCSampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    G, B1, K, n = 10, 64, 50, 100
    gen = torch.Generator().manual_seed(0)
    cvec = net.cloud_embed(torch.randn(G * B1, 1024, generator=gen).abs().cuda())
    centre = (torch.randn(G * B1, 3, generator=gen) * 0.3).cuda()
    x0 = (torch.randn(G * B1 * K, 9, generator=gen) * 50.0).cuda()
    smps = {"default (normal_ x 2 + graph)": PCSampler(net, G * B1, K, n, "cuda", groups=G),
            "seeded  (graph only)": PCSampler(net, G * B1, K, n, "cuda", groups=G, seed=1)}
    times = {k: [] for k in smps}
    for it in range(args.warmup + args.reps):
        for name, smp in smps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            smp.run(cvec, centre, x0)
            e1.record()
            e1.synchronize()
            if it >= args.warmup:
                times[name].append(e0.elapsed_time(e1))
    lines = []
    for name, smp in smps.items():
        t = sorted(times[name])
        lines.append(f"{name:32s} {smp.kernel_name:30s} PC-{n} pass, {G} x {B1} clouds x {K}: median {t[len(t) // 2]:.3f} ms "
                     f"[min {t[0]:.3f}, max {t[-1]:.3f}] over {len(t)} repeats")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
