"""Stand-alone timing of the bf16x9 chain kernels at the benched launch shape - 640 clouds x 50 candidates = 32 000 rows, ten batches per
launch - for profiles/x9_kmajor_under_mfma.txt.  One process times ONE build of the library (GENPOSE_HIP_LIB=<path> selects a variant
built with GP_BUILD_TAG, genpose_amd/build.py); arms are compared by running this script once per arm, alternating, in one session.

  PC-100   HIP events around single replays of the sampler graph (101 launches), noise pre-filled, x restored before each replay;
           the finish launch (launch 100: no network) timed in a graph of 50 of them; us per full launch = (chain - finish) / 100
  Heun-18  the same around the HeunSampler graph (18 steps, 38 launches)
  RK45     wall clock around ODESampler(trunk='bf16x9').run() from T0 = 0.15 (host polling included)
  --pmc N  instead of all that: N full PC launches at this shape, one by one, no graph (for a rocprofv3 --pmc pass)

  --products 6   the PC arms on the six-product kernel (PCSampler(products=6)); --only-pc skips the Heun and RK45 arms

    python scratch/x9_kmajor_measure.py [--reps 11] [--warmup 2] [--pmc N] [--label NAME] [--products 9|6] [--only-pc]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
G, B1, K, N_PC, N_HEUN, T0_ODE = 10, 64, 50, 100, 18, 0.15


def _events(fn, before, reps, warmup):
    ts = []
    for it in range(warmup + reps):
        before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if it >= warmup:
            ts.append(e0.elapsed_time(e1))
    return ts


def _fmt(ts, scale=1.0, unit="ms"):
    return f"{statistics.median(ts) * scale:.3f} [{min(ts) * scale:.3f}, {max(ts) * scale:.3f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pmc", type=int, default=0)
    ap.add_argument("--label", default=os.path.basename(os.environ.get("GENPOSE_HIP_LIB", "libgenpose_hip.so")))
    ap.add_argument("--products", type=int, default=9, choices=(9, 6))
    ap.add_argument("--only-pc", action="store_true")
    args = ap.parse_args()
    from genpose_amd.samplers import HeunSampler, ODESampler, PCSampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    gen = torch.Generator().manual_seed(0)
    B = G * B1
    cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
    centre = (torch.randn(B, 3, generator=gen) * 0.3).cuda()
    x0 = (torch.randn(B * K, 9, generator=gen) * 50.0).cuda()
    z1, z2 = torch.randn(N_PC, B * K, 9, generator=gen).cuda(), torch.randn(N_PC, B * K, 9, generator=gen).cuda()
    tag = f"[{args.label}]"

    if args.pmc:
        pc = PCSampler(net, B, K, N_PC, "cuda", groups=G, tile=128, trunk="bf16x9", use_graph=False, products=args.products)
        pc.cvec.copy_(cvec), pc.centre.copy_(centre), pc.x.copy_(x0), pc.z1.copy_(z1), pc.z2.copy_(z2)
        for i in range(args.pmc):
            pc.launch_step(i)
            torch.cuda.synchronize()
        print(f"{tag} {args.pmc} full launches of {pc.kernel_name}, sum |x| {pc.x.double().abs().sum().item()!r}")
        return

    # ---- PC-100
    pc = PCSampler(net, B, K, N_PC, "cuda", groups=G, tile=128, trunk="bf16x9", products=args.products)
    assert pc.kernel_name == ("pc_step_chain_kernel<bf16x9,6>" if args.products == 6 else "pc_step_chain_kernel<bf16x9>")
    pc.run(cvec, centre, x0, z1, z2)  # captures
    torch.cuda.synchronize()
    chk = pc.mean_x.double().abs().sum().item()
    chain = _events(pc.graph.replay, lambda: pc.x.copy_(x0), args.reps, args.warmup)
    NF = 50  # the finish launch (no network) on its own: a graph of NF of them, per launch
    pc.launch_step(N_PC)
    torch.cuda.synchronize()
    gfin = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gfin):
        for _ in range(NF):
            pc.launch_step(N_PC)
    fin = [t / NF for t in _events(gfin.replay, lambda: None, args.reps, args.warmup)]
    f = statistics.median(fin)
    print(f"{tag} PC-{N_PC} chain ({N_PC + 1} launches) {_fmt(chain)}   finish launch {_fmt(fin, 1e3, 'us')}")
    print(f"{tag}   per full launch (chain - finish) / {N_PC}: {_fmt([(t - f) / N_PC for t in chain], 1e3, 'us')}   sum |mean_x| {chk!r}")
    if args.only_pc:
        return
    # ---- Heun, 18 steps
    hs = HeunSampler(net, B, K, N_HEUN, "cuda", groups=G, tile=128)
    assert hs.kernel_name == "heun_step_chain_kernel<bf16x9>"
    hs.run(cvec, centre, x0)
    torch.cuda.synchronize()
    chk = hs.out.double().abs().sum().item()
    heun = _events(hs.graph.replay, lambda: hs.x.copy_(x0), args.reps, args.warmup)
    print(f"{tag} Heun-{N_HEUN} pass ({hs.nlaunch} launches) {_fmt(heun)}   sum |out| {chk!r}")
    # ---- one RK45 solve
    ode = ODESampler(net, B, K, "cuda", groups=G, tile=128, trunk="bf16x9")
    xo = x0 * 1e-3
    ts = []
    for it in range(2 + 7):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, poses = ode.run(cvec, centre, xo, T0_ODE)
        torch.cuda.synchronize()
        if it >= 2:
            ts.append((time.perf_counter() - t0) * 1e3)
    print(f"{tag} RK45 solve from T0 = {T0_ODE} (wall clock) {_fmt(ts)}   sum |poses| {poses.double().abs().sum().item()!r}")


if __name__ == "__main__":
    main()
