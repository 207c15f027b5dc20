"""Measurements of the mask-free front end (gp_box_sample, gp_cloud_extent, runner.DepthTracker; profiles/box_front_end.txt), one session:
  launch  gp_box_sample for 5 and 40 objects on a 640 x 480 frame - typical boxes (a rectangle of about 100 x 100 pixels) and boxes whose
          rectangle is the whole frame - beside gp_roi_sample_seeded for as many detections at crop 256, the launch it replaces;
          gp_cloud_extent at 5 and 256 clouds x 1024 points beside gp_rank_aggregate_rt at K = 50, its neighbour in a frame.  HIP events
          around 20 back-to-back raw launches on preallocated buffers, arms alternating in one loop, us per launch, median [min, max];
  frame   a DepthTracker.track frame (trained score checkpoint, consensus ranker, K = 50, N = 8) against FixedStepTracker.step fed the
          same clouds ready-made, same settings: host clock around the call + synchronize, arms alternating.
python scratch/box_front_end_measure.py [out file]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
torch.set_num_threads(16)

OUT = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.2f} [{min(v) * scale:.2f}, {max(v) * scale:.2f}]"

import box_front_end_reference as ref
import consensus_reference as cr
from genpose_amd import _lib, reward, synth
from genpose_amd._lib import ptr, stream_ptr
from genpose_amd.preprocess import DepthToClouds, get_bbox, inverse_crop_map

say(f"== device {torch.cuda.get_device_name(0)}")
INNER, WARM, REP = 20, 5, 31
say(f"HIP events around {INNER} back-to-back launches, {WARM} warm-up + {REP} timed samples, arms alternating, us per launch, median [min, max]; the C entry "
    "points through ctypes on PREALLOCATED buffers")
L, st = _lib.lib(), stream_ptr()
K = (591.0125, 590.16775, 322.525, 244.11084)
depth_h, masks_h, rois_h, _ = synth.golden_depth_frame(5)
H, W = depth_h.shape
depth = torch.from_numpy(depth_h.view(np.int16)).cuda()
fe = DepthToClouds()
seed = torch.from_numpy(np.array([1, 2, 3, 0, 0, 0, 0, 0], dtype=np.uint32).view(np.int32)).cuda()


def timed(arms):
    us = {a: [] for a in arms}
    for rep in range(WARM + REP):
        for a, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(INNER): fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= WARM: us[a].append(e0.elapsed_time(e1) * 1e3 / INNER)
    return us


rng = np.random.default_rng(3)
for n in (5, 40):
    # typical boxes: 0.055 m half-extents at 0.63 m (about 100 x 100 pixels) on the frame's large object, jittered; whole-frame boxes: behind the near plane
    rt = np.stack([ref.pose(ref.rotation(rng, about_z=float(rng.uniform(0, 90))), ref.centre_of(320 + rng.uniform(-40, 40), 240 + rng.uniform(-30, 30), 0.63, K)) for _ in range(n)])
    half = np.full((n, 3), 0.055 / 1.15, dtype=np.float32)
    rt_w = np.stack([ref.pose(ref.rotation(rng), [0, 0, 1.0]) for _ in range(n)])
    half_w = np.full((n, 3), 5.0, dtype=np.float32)
    t = [torch.from_numpy(a).cuda() for a in (rt, half, rt_w, half_w)]
    out = fe.empty_outputs_boxes(n)
    box = lambda r, h: L.gp_box_sample(H, W, 1, n, 1024, ptr(depth), None, ptr(r), ptr(h), 1.15, 0.01, 2, *K, ptr(seed), None, ptr(out["points"]), ptr(out["count"]),
                                       ptr(out["valid"]), st)
    # the comparator: n detections with object 0's mask and roi at crop 256
    masks = torch.from_numpy(np.repeat(masks_h[:, :, :1], n, axis=2).astype(np.uint8)).cuda()
    minv = torch.from_numpy(np.stack([inverse_crop_map(get_bbox(rois_h[0], H, W), 256, H, W)] * n).reshape(n, 6)).cuda()
    o2 = fe.empty_outputs(n)
    roi = lambda: L.gp_roi_sample_seeded(H, W, n, 256, 1024, ptr(depth), ptr(masks), ptr(minv), *K, ptr(seed), ptr(o2["points"]), ptr(o2["count"]),
                                         ptr(o2["depth_count"]), ptr(o2["valid"]), st)
    us = timed({"gp_roi_sample_seeded, crop 256": roi, "gp_box_sample, typical boxes": lambda: box(t[0], t[1]), "gp_box_sample, whole-frame rectangle": lambda: box(t[2], t[3])})
    say(f"  {n:3d} objects, 640 x 480, 1024 points")
    for a in us: say(f"    {a:44s} {mmm(us[a])} us")

for B in (5, 256):
    Kc = 50
    poses = torch.from_numpy(cr.make_clouds(B + Kc, B, Kc)[0]).cuda()
    energy = reward.consensus_energy(poses)
    o = reward.rank_aggregate(poses, energy, selected_num=30, with_rt=True)
    outs = [ptr(o[k]) for k in ("sorted_poses", "sorted_energy", "order", "avg_pose", "sorted_RTs", "avg_RT")]
    pts = torch.from_numpy(synth.make_batch(B)).float().cuda()
    rt = torch.eye(4, device="cuda").repeat(B, 1, 1)
    rt[:, :3, 3] = pts.mean(1)
    half = torch.empty(B, 3, device="cuda")
    alls = torch.ones(B, dtype=torch.int8, device="cuda")
    ext = lambda trim=0, sy=None: L.gp_cloud_extent(B, 1024, ptr(pts), ptr(rt), trim, ptr(sy), ptr(half), st)
    us = timed({"gp_rank_aggregate_rt, K = 50": lambda: L.gp_rank_aggregate_rt(B, Kc, 30, 0, ptr(poses), ptr(energy), *outs, st),
                "gp_cloud_extent, trim 0": ext, "gp_cloud_extent, trim 10": lambda: ext(10), "gp_cloud_extent, trim 0, symmetric": lambda: ext(0, alls)})
    say(f"  {B:3d} clouds x 1024 points")
    for a in us: say(f"    {a:44s} {mmm(us[a])} us")

# ---- a frame
import test_gpu_depth_tracker as tt
from genpose_amd.runner import DepthTracker, FixedStepTracker
mk = lambda: FixedStepTracker(tt._score_agent(), None, steps=8, repeat_num=50, ranker="consensus", seed=1, init="prior")
depths, _ = tt._frames()
dt, plain = DepthTracker(mk()), mk()
a = dt.acquire(*tt._acquisition(), tt.NAMES)
plain.step([(a["points"], tt.NAMES, None)])
clouds = dt.track(depths[1])["points"].clone()
plain.step([(clouds, tt.NAMES, None)])
ms = {"FixedStepTracker.step, ready-made clouds": [], "DepthTracker.track, host depth": [], "DepthTracker.track, device depth": []}
d_dev = torch.from_numpy(depths[2].view(np.int16)).cuda()
for rep in range(3 + 15):
    for name, fn in (("FixedStepTracker.step, ready-made clouds", lambda: plain.step([(clouds, tt.NAMES, None)])),
                     ("DepthTracker.track, host depth", lambda: dt.track(depths[2])), ("DepthTracker.track, device depth", lambda: dt.track(d_dev))):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if rep >= 3: ms[name].append((time.perf_counter() - t0) * 1e3)
say(f"  a frame of {tt.N_OBJ} objects (the test's splatted sequence), K = 50, N = 8, consensus ranker, host clock around call + synchronize, 3 warm-up + 15 samples, arms alternating")
for a in ms: say(f"    {a:44s} {mmm(ms[a])} ms")
say("  NOT measured: a five-object frame (the sequence has three), tracking error over a 30-frame sequence at inflate 1.0 / 1.15 / 1.3 and trim 0 / 10, REAL275, sensor noise, "
    "occlusion between objects")
