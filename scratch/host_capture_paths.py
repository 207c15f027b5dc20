"""Host time of the capture / replay and pinned-upload paths (genpose_amd/graphs.py), the parent commit's Python against this tree's over
the SAME shared library (profiles/host_capture_paths.txt).  The parent's side is a copy of its genpose_amd/*.py in a directory of its own:
    mkdir -p $P/genpose_amd && for f in $(git ls-tree --name-only <parent> genpose_amd/ | grep 'py$'); do git show <parent>:$f > $P/$f; done
    export GENPOSE_HIP_LIB=$PWD/genpose_amd/lib/libgenpose_hip.so
then, alternating, one fresh process per version and repeat (each under its own `timeout`, chained with &&):
    python scratch/host_capture_paths.py child $P out.jsonl parent && python scratch/host_capture_paths.py child . out.jsonl change && ...
    python scratch/host_capture_paths.py report out.jsonl
A child imports genpose_amd from the root it is given, runs the four legs (host clock around each call + synchronise) and appends one JSON line."""
import json, os, statistics, sys, time


def report(path):
    rows = [json.loads(l) for l in open(path) if l.strip()]
    legs = [("a_tracking_ms_per_frame", "(a) TrackingRunner, graphs, 1 sequence x 5 objects x K = 50, 30 frames (6 warm-up): ms per frame", "ms"),
            ("b_fixed_step_ms_per_frame", "(b) FixedStepTracker(steps=8), 5 objects x K = 50, energy ranker: ms per frame (median of frames 6..29, step + synchronise)", "ms"),
            ("c_encode_replay_us", "(c) Pointnet2EncoderHIP.encode replay, 5 clouds: us per call (median of 200, call + synchronise)", "us"),
            ("d_heun_single_run_us", "(d) HeunSampler.run, 5 x 50 rows, N = 8, launches='single': us per call (median of 200, call + synchronise)", "us")]
    for key, title, unit in legs:
        print(title)
        v = {lab: [r[key] for r in rows if r["label"] == lab] for lab in ("parent", "change")}
        for lab in ("parent", "change"):
            print(f"  {lab:7s} median {statistics.median(v[lab]):9.3f} {unit}  [min {min(v[lab]):.3f}, max {max(v[lab]):.3f}]  by child {[round(x, 3) for x in v[lab]]}")
        ok = statistics.median(v["change"]) <= max(v["parent"])
        print(f"  change median <= parent max: {ok}")
    print("fixed-step stats of the last child:", rows[-1].get("b_stats"))


if sys.argv[1] == "report":
    report(sys.argv[2])
    sys.exit(0)

ROOT, OUT, LABEL = os.path.abspath(sys.argv[2]), sys.argv[3], sys.argv[4]
sys.path.insert(0, ROOT)
import torch
torch.set_num_threads(16)
import genpose_amd
assert os.path.dirname(os.path.abspath(genpose_amd.__file__)) == os.path.join(ROOT, "genpose_amd"), genpose_amd.__file__
from genpose_amd import synth
from genpose_amd.config import get_config
from genpose_amd.encoder import Pointnet2EncoderHIP
from genpose_amd.posenet_agent import PoseNet
from genpose_amd.runner import FixedStepTracker, TrackingRunner
from genpose_amd.samplers import HeunSampler
from genpose_amd.scorenet import ScoreNetHIP
from genpose_amd.weights_synth import make_state_dict

n_obj, K, nfr, warm = 5, 50, 30, 6
sd_s, sd_e = make_state_dict(0, "score"), make_state_dict(0, "energy")
base = torch.from_numpy(synth.make_batch(n_obj, start=0))
gt = torch.eye(4).repeat(n_obj, 1, 1); gt[:, :3, 3] = base.mean(dim=1)
frames = [(base + 0.002 * f).cuda() for f in range(nfr)]
names = [f"o{j}" for j in range(n_obj)]
res = {"label": LABEL}
torch.manual_seed(0)

# (a) TrackingRunner with graphs: ms per frame after warm-up, one synchronise at the end (scratch/bench_tracking.py)
sa = PoseNet(get_config(posenet_mode="score", sampler_mode=["ode"])); sa.load_state_dict(sd_s)
ea = PoseNet(get_config(posenet_mode="energy")); ea.load_state_dict(sd_e)
tr = TrackingRunner(sa, ea, repeat_num=K, T0=0.15)
for f in range(warm): tr.step(frames[f], names, gt)
torch.cuda.synchronize(); t = time.perf_counter()
for f in range(warm, nfr): tr.step(frames[f], names, gt)
torch.cuda.synchronize(); res["a_tracking_ms_per_frame"] = (time.perf_counter() - t) / (nfr - warm) * 1e3

# (b) FixedStepTracker(steps=8): host clock around step() + synchronise per frame, median over frames warm.. (scratch/fixed_step_tracking_measure.py)
sh = PoseNet(get_config(posenet_mode="score", sampler_mode=["heun"], sampling_steps=8)); sh.load_state_dict(sd_s)
ft = FixedStepTracker(sh, ea, steps=8, repeat_num=K, T0=0.15, seed=7)
ms = []
for f in range(nfr):
    torch.cuda.synchronize(); t = time.perf_counter()
    ft.step([(frames[f], names, gt)])
    torch.cuda.synchronize()
    if f >= warm: ms.append((time.perf_counter() - t) * 1e3)
res["b_fixed_step_ms_per_frame"] = statistics.median(ms)
res["b_stats"] = {k: ft.last_stats[k] for k in ("replays", "captures", "launches")}

# (c) Pointnet2EncoderHIP.encode replay at 5 clouds: host + device per call, with a synchronise
enc = Pointnet2EncoderHIP(sd_s, "cuda")
for _ in range(5): enc.encode(frames[0])
us = []
for i in range(200):
    torch.cuda.synchronize(); t = time.perf_counter()
    enc.encode(frames[i % nfr])
    torch.cuda.synchronize(); us.append((time.perf_counter() - t) * 1e6)
res["c_encode_replay_us"] = statistics.median(us)
assert len(enc._pass_graphs) == 1

# (d) HeunSampler.run at 5 x 50 rows, launches='single'
net = ScoreNetHIP(sd_s, "cuda")
gen = torch.Generator().manual_seed(5)
cvec = net.cloud_embed(torch.randn(n_obj, 1024, generator=gen).abs().cuda())
centre, x0 = (torch.randn(n_obj, 3, generator=gen) * 0.3).cuda(), (torch.randn(n_obj * K, 9, generator=gen) * 0.0358).cuda()
hs = HeunSampler(net, n_obj, K, 8, "cuda", launches="single")
for _ in range(5): hs.run(cvec, centre, x0, T0=0.15)
us = []
for i in range(200):
    torch.cuda.synchronize(); t = time.perf_counter()
    hs.run(cvec, centre, x0, T0=0.15)
    torch.cuda.synchronize(); us.append((time.perf_counter() - t) * 1e6)
res["d_heun_single_run_us"] = statistics.median(us)
assert hs.captures == 1
with open(OUT, "a") as f:
    f.write(json.dumps(res) + "\n")
print(json.dumps(res), flush=True)
