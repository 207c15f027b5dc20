"""Measurements of the many-frame depth front end (profiles/depth_front_end_frames.txt), one session, arms alternating, median [min, max]:
  front   F calls of preprocess.DepthToClouds.device_clouds (gp_roi_sample_seeded, one launch per frame) against ONE device_clouds_frames
          (gp_roi_sample_frames) on F = 1, 8, 43 frames synth.golden_depth_frame(5 + f) (6 detections each), crop 256, 1024 points, host
          arrays in and device inputs in: host clock around the call(s) + synchronize; the packing + pinned upload of the masks alone; and
          the kernels alone - HIP events around back-to-back raw launches on preallocated buffers, F launches against one.
  runner  DPM-Solver++(2M) N = 8, K = 50, energy ranker, trained checkpoints: a loop of SingleFrameRunner.infer_depth over 43 frames against
          one infer_depth_frames; clouds per second.
python scratch/depth_frames_measure.py [out file] [front|runner ...]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
torch.set_num_threads(16)

OUT = open(sys.argv[1], "a") if len(sys.argv) > 1 else None
PARTS = sys.argv[2:] or ["front", "runner"]
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"

from genpose_amd import _lib, synth
from genpose_amd._lib import ptr, stream_ptr
from genpose_amd.graphs import PinnedBlock
from genpose_amd.preprocess import DepthToClouds, frame_tables

say(f"== depth front end over many frames: device {torch.cuda.get_device_name(0)}")
FMAX = 43
ALL = [synth.golden_depth_frame(5 + f) for f in range(FMAX)]
fe = DepthToClouds()  # crop 256, 1024 points

def timed(arms, warm, rep):
    ms = {a: [] for a in arms}
    for r in range(warm + rep):
        for a, fn in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warm: ms[a].append((time.perf_counter() - t0) * 1e3)
    return ms

if "front" in PARTS:
    for F in (1, 8, 43):
        frames = [fr[:3] for fr in ALL[:F]]
        t = frame_tables(frames, fe.img)
        n, H, W = t["ndet"], t["H"], t["W"]
        outs = [fe.empty_outputs(len(fr[2])) for fr in frames]
        out = fe.empty_outputs_frames(n)
        d_dev = torch.from_numpy(np.stack([fr[0] for fr in frames]).view(np.int16)).cuda()
        m_dev = [torch.from_numpy(fr[1].astype(np.uint8)).cuda() for fr in frames]
        dev = [(d_dev[f], m_dev[f], frames[f][2]) for f in range(F)]
        blk, mbuf = PinnedBlock((t["mask_bytes"],), torch.uint8), torch.empty(t["mask_bytes"], dtype=torch.uint8, device="cuda")
        hm = [torch.from_numpy(fr[1]) for fr in frames]
        def fill(h):
            for f, m in enumerate(hm):
                o = int(t["mask_off"][f])
                h[o:o + m.numel()].view(m.shape).copy_(m)
        run = [0]
        def per_frame(src):
            for f in range(F):
                fe.device_clouds(*src[f], 7, run[0] + f, out=outs[f])
            run[0] += F
        def batched(src):
            fe.device_clouds_frames(src, 7, first_run=run[0], out=out)
            run[0] += F
        arms = {f"{F} x device_clouds (host arrays in)": lambda: per_frame(frames), "device_clouds_frames (host arrays in)": lambda: batched(frames),
                f"{F} x device_clouds (device depth / masks in)": lambda: per_frame(dev), "device_clouds_frames (device depth / masks in)": lambda: batched(dev),
                "masks alone: packed into a pinned block (bool -> uint8) and sent": lambda: blk.send(mbuf, fill)}
        WARM, REP = 10, 101 if F < 43 else 51
        ms = timed(arms, WARM, REP)
        say(f"  F = {F}: {n} detections, {t['mask_bytes'] / 1e6:.1f} MB of masks, {d_dev.numel() * 2 / 1e6:.1f} MB of depth; host clock around the call(s) + synchronize, "
            f"{WARM} warm-up + {REP} timed, arms alternating, ms per batch of {F} frame(s)")
        for a in arms:
            say(f"    {a:66s} {mmm(ms[a])} ms")
        med = lambda a: statistics.median(ms[a])
        for kind in ("host arrays in", "device depth / masks in"):
            say(f"    {kind}: {F} calls / one batched call (medians) = {med(f'{F} x device_clouds ({kind})') / med(f'device_clouds_frames ({kind})'):.2f}x")
        say(f"    masks alone / batched call with host arrays in (medians) = {med('masks alone: packed into a pinned block (bool -> uint8) and sent') / med('device_clouds_frames (host arrays in)'):.2f}")

        # ---- the kernels alone
        L, INNER = _lib.lib(), 20 if F < 43 else 5
        k, st = (fe.fx, fe.fy, fe.cx, fe.cy), stream_ptr()
        packed = torch.cat([m.reshape(-1) for m in m_dev])
        tabs = {name: torch.from_numpy(t[name].view(np.int32) if name == "draw" else t[name]).cuda() for name in ("mask_off", "det", "draw", "minv")}
        off = np.cumsum([0] + [len(fr[2]) for fr in frames])
        minvs = [tabs["minv"][off[f]:off[f + 1]].contiguous() for f in range(F)]
        seeds = [torch.tensor([7, 0, f, 0, 0, 0, 0, 0], dtype=torch.int32, device="cuda") for f in range(F)]
        def many():
            for f in range(F):
                L.gp_roi_sample_seeded(H, W, len(frames[f][2]), fe.img, fe.n_pts, ptr(d_dev[f]), ptr(m_dev[f]), ptr(minvs[f]), *k, ptr(seeds[f]),
                                       ptr(outs[f]["points"]), ptr(outs[f]["count"]), ptr(outs[f]["depth_count"]), ptr(outs[f]["valid"]), st)
        def one():
            L.gp_roi_sample_frames(H, W, F, n, fe.img, fe.n_pts, ptr(d_dev), ptr(packed), packed.numel(), ptr(tabs["mask_off"]), ptr(tabs["det"]), ptr(tabs["draw"]),
                                   ptr(tabs["minv"]), *k, ptr(seeds[0]), ptr(out["points"]), ptr(out["count"]), ptr(out["depth_count"]), ptr(out["valid"]), st)
        karms = {f"{F} x gp_roi_sample_seeded": many, "gp_roi_sample_frames": one}
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
        same = all(torch.equal(out[key], torch.cat([o[key] for o in outs])) for key in ("points", "count", "depth_count", "valid"))
        say(f"    kernels alone, HIP events around {INNER} back-to-back repetitions on preallocated buffers, 5 warm-up + 31 timed, us per batch of {F} frame(s) "
            f"(outputs of the two arms bit-equal: {same}):")
        for a in karms:
            say(f"      {a:36s} {mmm(us[a])} us")
        say(f"      {F} launches / one launch (medians) = {statistics.median(us[f'{F} x gp_roi_sample_seeded']) / statistics.median(us['gp_roi_sample_frames']):.2f}x")

if "runner" in PARTS:
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import SingleFrameRunner
    N, F = 8, FMAX
    runner = SingleFrameRunner(tr._agent("score", "dpm2m", N), tr._agent("energy"), repeat_num=tr.K, T0=tr.T0, batch_size=256)
    n = sum(len(fr[2]) for fr in ALL[:F])
    torch.manual_seed(0)
    def loop():
        for f, fr in enumerate(ALL[:F]):
            runner.infer_depth(*fr, seed=7, frame=f)
    arms = {f"{F} x infer_depth": loop, "infer_depth_frames": lambda: runner.infer_depth_frames(ALL[:F], seed=7)}
    WARM, REP = 2, 9
    ms = timed(arms, WARM, REP)
    say(f"  runner: {F} frames, {n} detections, DPM-Solver++(2M) N = {N}, K = {tr.K}, T0 = {tr.T0}, energy ranker, trained checkpoints, batch_size 256; host arrays "
        f"in; host clock around the arm + synchronize, {WARM} warm-up + {REP} timed, arms alternating, ms per {F} frames")
    for a in arms:
        say(f"    {a:24s} {mmm(ms[a])} ms   {n / statistics.median(ms[a]) * 1e3:9.0f} clouds / s")
    say(f"    {F} calls / one batched call (medians) = {statistics.median(ms[f'{F} x infer_depth']) / statistics.median(ms['infer_depth_frames']):.2f}x")
