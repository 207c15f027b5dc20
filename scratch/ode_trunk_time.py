"""ODESampler(trunk=): the chain plan's stage kernels as exact-product split bf16 (rk45_stage_chain_kernel_bf16x9) against the fp32 MFMA chain
stage (rk45_stage_chain_kernel<2, STAGE, 0>), both in ONE session, alternating, 9 repeats each: one ODE solve from T0 = 1 timed by HIP events,
median [min, max].  The time per stage launch comes from a run of its own under `rocprofv3 --kernel-trace --stats` (same script).
    python scratch/ode_trunk_time.py [clouds] [K] [groups] [repeats]        (default 640 50 10 9 = 32 000 rows, ten 64-cloud batches)"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose_amd.samplers import ODESampler  # noqa: E402
from genpose_amd.scorenet import ScoreNetHIP  # noqa: E402
from genpose_amd.weights_synth import make_state_dict  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 640
K = int(sys.argv[2]) if len(sys.argv) > 2 else 50
G = int(sys.argv[3]) if len(sys.argv) > 3 else 10
REP = int(sys.argv[4]) if len(sys.argv) > 4 else 9
T0 = 1.0
net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
gen = torch.Generator().manual_seed(1)
cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
centre = torch.randn(B, 3, generator=gen).cuda() * 0.3
x0 = torch.randn(B * K, 9, generator=gen).cuda() * 50.0  # the prior's scale at T0 = 1
print(f"{B} clouds x {K} candidates = {B * K} rows in {G} groups, T0 = {T0}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
smps = {t: ODESampler(net, B, K, "cuda", groups=G, tile=128, trunk=t) for t in ("f32mfma", "bf16x9")}
assert smps["bf16x9"].trunk == "bf16x9"
for smp in smps.values():
    for _ in range(3):  # captures the attempt graph, settles its size
        smp.run(cvec, centre, x0, T0)
torch.cuda.synchronize()
ts = {t: [] for t in smps}
for _ in range(REP):
    for t, smp in smps.items():  # alternating
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        smp.run(cvec, centre, x0, T0)
        e1.record()
        e1.synchronize()
        ts[t].append(e0.elapsed_time(e1))
for t, smp in smps.items():
    att = [int(s["n_attempts"]) for s in smp.group_stats]
    v = ts[t]
    med = statistics.median(v)
    print(f"{smp.kernel_name:34s} solve {med:8.3f} ms [{min(v):.3f}, {max(v):.3f}]  attempts per group {min(att)}-{max(att)}  "
          f"{B * K / med * 1e3 / 1e3:8.1f} k rows/s")
m9, m32 = statistics.median(ts["bf16x9"]), min(ts["f32mfma"])
print(f"bf16x9 median {m9:.3f} ms vs fp32 chain minimum {m32:.3f} ms: " + ("FASTER" if m9 < m32 else "NOT faster"))
