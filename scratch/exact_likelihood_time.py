"""Cost of the exact-divergence likelihood against the one-probe one, in one session (profiles/exact_likelihood.txt):
  1. gp_score_div_exact against gp_score_div at 800 and 32 000 rows: HIP events around a captured graph of back-to-back launches,
     the two kernels alternating, median [min, max] of the repeats;
  2. attempts of both divergences on the SAME inputs: fixture G12 (3 rows) and the 2 x 3 problem of the solve test;
  3. one exact against one Hutchinson likelihood solve at 256 clouds x 50 poses (same clouds, same poses), HIP events around
     cond_ode_likelihood on a warmed solver, alternating, with attempt counts.
python scratch/exact_likelihood_time.py [repeats=9] [out=-]"""
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import exact_likelihood_ref as er  # noqa: E402
from genpose_amd import _lib  # noqa: E402
from genpose_amd._lib import ptr, stream_ptr  # noqa: E402
from genpose_amd.likelihood import cond_ode_likelihood  # noqa: E402
from genpose_amd.samplers import ODESampler  # noqa: E402
from genpose_amd.scorenet import ScoreNetHIP  # noqa: E402
from genpose_amd.weights_synth import make_state_dict  # noqa: E402

REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 and sys.argv[2] != "-" else None
WARM = 3
SIGMA_MAX = 50.0


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if OUT:
        OUT.write(line + "\n")
        OUT.flush()


def mmm(v):
    return f"{statistics.median(v):9.1f} [{min(v):.1f}, {max(v):.1f}]"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def problem(B, K, t, seed):
    gen = torch.Generator().manual_seed(seed)
    pf = torch.randn(B, 1024, generator=gen).abs()
    x = er.unit_axis_poses(B * K, t, gen)
    probe = torch.randn(B * K, 9, generator=gen)
    return pf.cuda(), x.cuda(), probe.cuda()


def kernels(net, rows, t=0.3, K=50):
    B = rows // K
    pf, x, probe = problem(B, K, t, 1)
    cvec = net.cloud_embed(pf)
    tvec = net.time_embed(torch.tensor([t], device="cuda"))[0].contiguous()
    sigma = torch.tensor([0.01 * 5000.0 ** t], device="cuda")
    score, div = torch.empty(rows, 9, device="cuda"), torch.empty(rows, device="cuda")
    n = max(8, min(200, 160_000 // rows * 4))  # launches per timed replay: a window of several milliseconds at either size
    common = (B, K, net.w.ref(), ptr(cvec), ptr(tvec), ptr(x))
    launch = {"gp_score_div": lambda: _lib.call("gp_score_div", *common, ptr(probe), ptr(sigma), ptr(score), ptr(div), stream_ptr()),
              "gp_score_div_exact": lambda: _lib.call("gp_score_div_exact", *common, ptr(sigma), ptr(score), ptr(div), stream_ptr())}
    graphs = {}
    for name, fn in launch.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(n):
                fn()
        graphs[name] = g
    us = {name: [] for name in launch}
    for rep in range(WARM + REPEATS):
        for name, g in graphs.items():  # alternating
            ms, _ = timed(g.replay)
            if rep >= WARM:
                us[name].append(ms * 1e3 / n)
    tiles = (rows + 15) // 16
    for name in launch:
        say(f"  {name:19s} rows {rows:6d} ({tiles} tiles, {n} launches per replay): {mmm(us[name])} us per launch")
    ratios = [a / b for a, b in zip(us["gp_score_div_exact"], us["gp_score_div"])]
    say(f"  exact / one-probe at {rows} rows: {statistics.median(ratios):.2f} [{min(ratios):.2f}, {max(ratios):.2f}] (pairwise, same repeat)")


def attempts_same_inputs(net):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    cases = {}
    g = np.load(os.path.join(ROOT, "tests", "golden", "g12_likelihood.npz"))
    agent = PoseNet(get_config(posenet_mode="score"))
    agent.load_state_dict(make_state_dict(0, "score"))
    pts = torch.from_numpy(g["pts"]).cuda()
    feat = agent.net({"pts": pts, "pts_center": pts.mean(dim=1)}, mode="pts_feature").float()
    cases["fixture G12 (3 rows, its own probe)"] = (feat, 1, torch.from_numpy(g["pose"]).cuda(), torch.from_numpy(g["probe"]).cuda(), 1e-5)
    gen = torch.Generator().manual_seed(5)
    pf = torch.randn(2, 1024, generator=gen).abs()
    x = er.unit_axis_poses(6, 1e-5, gen)
    cases["solve test, 2 clouds x 3 poses"] = (pf.cuda(), 3, x.cuda(), torch.randn(6, 9, generator=gen).cuda() * SIGMA_MAX, 1e-5)
    for name, (pf, K, x, probe, tol) in cases.items():
        cvec = net.cloud_embed(pf)
        for div, e in (("hutchinson", probe), ("exact", None)):
            st = {}
            _, bits = cond_ode_likelihood(net, cvec, K, x, e, rtol=tol, atol=tol, stats=st, divergence=div)
            say(f"  {name}, rtol = atol = {tol:g}, {div:10s}: {st['attempts']:5d} attempts, bits {np.round(bits.cpu().numpy(), 3).tolist()}")


def solves(net, B=256, K=50):
    pf, x, probe = problem(B, K, 1e-5, 2)
    probe = probe * SIGMA_MAX  # the reference draws the probe from the prior, N(0, sigma_max^2)
    cvec = net.cloud_embed(pf)
    solver = {d: ODESampler(net, B, K, "cuda", model=m) for d, m in (("hutchinson", "likelihood"), ("exact", "likelihood_exact"))}
    ms, att, bits = {d: [] for d in solver}, {}, {}
    for rep in range(2 + REPEATS):
        for d in solver:  # alternating
            st = {}
            t, (_, b) = timed(lambda: cond_ode_likelihood(net, cvec, K, x, probe if d == "hutchinson" else None, stats=st, solver=solver[d], divergence=d))
            att[d], bits[d] = st["attempts"], b
            if rep >= 2:
                ms[d].append(t)
            say(f"    repeat {rep - 2:2d} {d:10s} {t:9.1f} ms, {st['attempts']} attempts ({solver[d].kernel_name}, {solver[d].last_replays})")
    for d in solver:
        say(f"  {d:10s} {B} clouds x {K} poses, rtol = atol = 1e-5: {mmm(ms[d])} ms per solve, {att[d]} attempts, "
            f"{statistics.median(ms[d]) * 1e3 / att[d]:.0f} us per attempt")
    r = [a / b for a, b in zip(ms["exact"], ms["hutchinson"])]
    say(f"  exact / one-probe solve: {statistics.median(r):.2f} [{min(r):.2f}, {max(r):.2f}] in time, {att['exact'] / att['hutchinson']:.2f} in attempts")
    d = (bits["hutchinson"] - bits["exact"]).cpu().numpy()
    say(f"  one-probe minus exact log-likelihood over the {B * K} rows (bits): mean {d.mean():.3f}, std {d.std():.3f}, max |.| {np.abs(d).max():.3f}; "
        f"exact bits: mean {bits['exact'].mean().item():.3f}, std over rows {bits['exact'].std().item():.3f}")


if __name__ == "__main__":
    _lib.check_device()
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    say(f"device {torch.cuda.get_device_name(0)}; {REPEATS} repeats after warm-up; seeded weights (seed 0)")
    say("1. kernels, HIP events, us per launch, median [min, max]")
    for rows in (800, 32000):
        kernels(net, rows)
    say("2. attempts of both divergences on the same inputs")
    attempts_same_inputs(net)
    say("3. likelihood solves, HIP events, ms per solve, median [min, max]")
    solves(net)
