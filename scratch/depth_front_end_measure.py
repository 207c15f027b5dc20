"""Measurements of the depth front end (profiles/depth_front_end.txt), one session, arms alternating, median [min, max]:
  front   preprocess.DepthToClouds.__call__ (full clouds, count read-back, numpy permutation, ids upload, gp_cloud_sample) against
          device_clouds (gp_roi_sample_seeded, nothing read back) on synth.golden_depth_frame(5) and on a frame of five usable detections,
          crop 256, 1024 points: host clock around the call + synchronize; and the kernels alone - HIP events around 20 back-to-back raw
          launches on preallocated buffers, gp_roi_to_cloud + gp_cloud_sample against gp_roi_sample_seeded.
python scratch/depth_front_end_measure.py [out file]"""
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
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"

from genpose_amd import _lib, synth
from genpose_amd._lib import ptr, stream_ptr
from genpose_amd.preprocess import DepthToClouds, get_bbox, inverse_crop_map

say(f"== depth front end: device {torch.cuda.get_device_name(0)}")

def five_usable():
    """Five detections the reference keeps: golden_depth_frame(5, n_inst=7) without its empty mask and its depth hole."""
    depth, masks, rois, cls = synth.golden_depth_frame(5, n_inst=7)
    keep = [0, 1, 2, 3, 6]
    return depth, np.ascontiguousarray(masks[:, :, keep]), rois[keep], cls[keep]

FRAMES = {"golden_depth_frame(5): 6 detections, 4 kept": synth.golden_depth_frame(5), "five usable detections": five_usable()}
fe = DepthToClouds()  # crop 256, 1024 points
WARM, REP = 10, 101

# ---- front: the calls
for name, (depth, masks, rois, cls) in FRAMES.items():
    rng = np.random.default_rng(0)
    n = len(rois)
    out = fe.empty_outputs(n)
    d_dev, m_dev = torch.from_numpy(depth.view(np.int16)).cuda(), torch.from_numpy(masks.astype(np.uint8)).cuda()
    arms = {"__call__ (host arrays in)": lambda: fe(depth, masks, rois, cls, rng=rng),
            "device_clouds (host arrays in)": lambda r=[0]: (fe.device_clouds(depth, masks, rois, 7, r[0], out=out), r.__setitem__(0, r[0] + 1)),
            "__call__ (device depth / masks in)": lambda: fe(d_dev, m_dev, rois, cls, rng=rng),
            "device_clouds (device depth / masks in)": lambda r=[0]: (fe.device_clouds(d_dev, m_dev, rois, 7, r[0], out=out), r.__setitem__(0, r[0] + 1))}
    ms = {a: [] for a in arms}
    for rep in range(WARM + REP):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
    cnt = fe.device_clouds(depth, masks, rois, 7, 0)["count"].tolist()
    say(f"  {name}: valid pixels per detection {cnt}; host clock around the call + synchronize, {WARM} warm-up + {REP} timed, arms alternating, ms per frame")
    for a in arms:
        say(f"    {a:42s} {mmm(ms[a])} ms")
    for kind in ("host arrays in", "device depth / masks in"):
        say(f"    {kind}: __call__ / device_clouds (medians) = {statistics.median(ms[f'__call__ ({kind})']) / statistics.median(ms[f'device_clouds ({kind})']):.2f}x")

    # ---- front: the kernels alone
    L, INNER = _lib.lib(), 20
    H, W = depth.shape
    minv = torch.from_numpy(np.stack([inverse_crop_map(get_bbox(r, H, W), fe.img, H, W) for r in rois]).reshape(n, 6)).cuda()
    seed = torch.tensor([7, 0, 3, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    cap = fe.img * fe.img
    pcl = torch.empty(n, cap, 3, device="cuda")
    c32, d32 = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ids = torch.from_numpy(np.stack([rng.permutation(cap)[:fe.n_pts] for _ in range(n)]).astype(np.int32)).cuda()
    o2 = torch.empty(n, fe.n_pts, 3, device="cuda")
    k, st = (fe.fx, fe.fy, fe.cx, fe.cy), stream_ptr()
    def two():
        L.gp_roi_to_cloud(H, W, n, fe.img, ptr(d_dev), ptr(m_dev), ptr(minv), *k, ptr(pcl), ptr(c32), ptr(d32), st)
        L.gp_cloud_sample(n, cap, fe.n_pts, ptr(pcl), ptr(c32), ptr(ids), ptr(o2), st)
    one = lambda: L.gp_roi_sample_seeded(H, W, n, fe.img, fe.n_pts, ptr(d_dev), ptr(m_dev), ptr(minv), *k, ptr(seed), ptr(out["points"]), ptr(out["count"]),
                                         ptr(out["depth_count"]), ptr(out["valid"]), st)
    karms = {"gp_roi_to_cloud + gp_cloud_sample": two, "gp_roi_sample_seeded": one}
    us = {a: [] for a in karms}
    for rep in range(5 + 31):
        for a, fn in karms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(INNER): fn()
            e1.record()
            torch.cuda.synchronize()
            if rep >= 5: us[a].append(e0.elapsed_time(e1) * 1e3 / INNER)
    say(f"    kernels alone, HIP events around {INNER} back-to-back launches on preallocated buffers, 5 warm-up + 31 timed, us per frame:")
    for a in karms:
        say(f"      {a:36s} {mmm(us[a])} us")
