"""One tracking sequence frame by frame: where does the spread of the per-frame time come from?  Variants of how the ENERGY model's encoder
graph (A') is scheduled against the adaptive solve, each as 7 repeats of 60 frames (ms per frame by repeat):
  side      as shipped: A' on a side stream underneath the solve
  lowprio   the side stream created with the lowest priority
  before    A' on the main stream right behind graph A (before the solve)
  after     A' on the main stream after the solve (right before graph B)
    python scratch/track_variants.py"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from genpose_amd import runner, synth  # noqa: E402
from genpose_amd.config import get_config  # noqa: E402
from genpose_amd.posenet_agent import PoseNet  # noqa: E402
from genpose_amd.weights_synth import make_state_dict  # noqa: E402

sa = PoseNet(get_config(posenet_mode="score", sampler_mode=["ode"])); sa.load_state_dict(make_state_dict(0, "score"))
ea = PoseNet(get_config(posenet_mode="energy")); ea.load_state_dict(make_state_dict(0, "energy"))
n_obj, K, nfr = 5, 50, 30
base = torch.from_numpy(synth.make_batch(n_obj, start=0))
gt = torch.eye(4).repeat(n_obj, 1, 1); gt[:, :3, 3] = base.mean(dim=1)
frames = [(base + 0.002 * f).cuda() for f in range(nfr)]
names = [f"o{j}" for j in range(n_obj)]


def patch(mode):
    FG = runner._FrameGraphs
    if not hasattr(FG, "_embed_orig"):
        FG._embed_orig, FG._rank_orig = FG.embed, FG.rank
    if mode in ("side", "lowprio"):
        FG.embed, FG.rank = FG._embed_orig, FG._rank_orig
        return

    def embed(self, pts):
        key = (tuple(pts.shape), pts.dtype)
        if self._a.get(key) is None:
            return FG._embed_orig(self, pts)  # capture through the shipped path
        ent = self._a.get(key)
        cur = torch.cuda.current_stream(pts.device)
        ent.replay(pts)
        if mode == "before":
            ent.extra["side"].replay()
        self.ev_e.record(cur)
        return ent.outs

    def rank(self, pred, centre, cvec_e):
        if mode == "after":
            key = next(iter(self._a.keys()))
            self._a.get(key).extra["side"].replay()
            self.ev_e.record(torch.cuda.current_stream(pred.device))
        return FG._rank_orig(self, pred, centre, cvec_e)
    FG.embed, FG.rank = embed, rank


for mode in ("side", "lowprio", "before", "after", "side"):
    patch(mode)
    tr = runner.TrackingRunner(sa, ea, repeat_num=K, T0=0.15)
    if mode == "lowprio":
        tr.step(frames[0], names, gt)
        lo, hi = torch.cuda.Stream.priority_range() if hasattr(torch.cuda.Stream, "priority_range") else (0, -1)
        tr._graphs.side = torch.cuda.Stream(priority=max(lo, hi))  # the numerically largest value is the lowest priority
    for f in range(8):
        tr.step(frames[f % nfr], names, gt)
    torch.cuda.synchronize()
    per = []
    for rep in range(7):
        t0 = time.perf_counter()
        for f in range(60):
            tr.step(frames[(8 + rep * 60 + f) % nfr], names, gt)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / 60 * 1e3)
    print(f"{mode:8s} median {statistics.median(per):.3f} ms per frame  by repeat {[round(p, 3) for p in per]}  nfev {int(sa.net.last_sampler.last_stats['nfev'])}", flush=True)
