"""Measurements of the schedule classes on the fixed-step solvers and of runner.FixedStepTracker(init='prior') (profiles/sched_classes.txt),
one session (process) per part:
  solve    HeunSampler uniform, 250 and 3 200 rows (K = 50), N = 8, T0 = 0.15, 'chain' and 'single': HIP events around run() on warmed, captured
           samplers, median [min, max].  The same part run from a checkout of the parent commit (SC_ROOT=<that tree>) gives the parent's
           figures; the caller alternates the two processes.  With classes available it adds the class-aware sampler on the same geometry,
           every cloud in class 0 and one cloud of five in class 1.
  frame    a five-object frame (K = 50, N = 8, energy ranker, trained checkpoints) with ONE object acquired under init='prior', against what a
           user of the parent commit does - the same frame with four objects on FixedStepTracker plus a separate HeunSampler solve from
           acquire_T0 for the fifth, serial on one stream - and against the uniform five-object init='gt' frame; and init='prior' with
           nothing acquired.  Host clock around the arm + synchronize, arms alternating per frame.
  quality  the 30-frame synthetic sequence of profiles/fixed_step_tracking.txt: init='prior' beside init='gt', N = 8 / 16, acquire_T0 0.55 / 1.0;
           frame 0 is an acquisition under 'prior'.
python scratch/sched_classes_measure.py solve|frame|quality [out file]"""
import os, statistics, sys, time
ROOT = os.environ.get("SC_ROOT") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
torch.set_num_threads(16)

PART = sys.argv[1]
OUT = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"

import inspect
from genpose_amd.samplers import HeunSampler
HAVE_CLASSES = "classes" in inspect.signature(HeunSampler.__init__).parameters
say(f"== {PART}: device {torch.cuda.get_device_name(0)}; tree {'with' if HAVE_CLASSES else 'WITHOUT (parent)'} schedule classes")

if PART == "solve":
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    K, N, T0, WARM, REP = 50, 8, 0.15, 5, 25
    say(f"HIP events around HeunSampler.run (input copies + one graph replay), N = {N}, {WARM} warm-up + {REP} timed repeats, arms alternating, ms, median [min, max]")
    for B in (5, 64):
        gen = torch.Generator().manual_seed(B)
        cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
        centre, x0 = (torch.randn(B, 3, generator=gen) * 0.3).cuda(), (torch.randn(B * K, 9, generator=gen) * 0.0358).cuda()
        arms = {}
        for form in ("chain", "single"):
            arms[f"uniform {form}"] = (HeunSampler(net, B, K, N, "cuda", launches=form), dict(T0=T0))
            if HAVE_CLASSES:
                s = HeunSampler(net, B, K, N, "cuda", launches=form, classes=2)
                arms[f"classes {form}, all class 0"] = (s, dict(T0=(T0, 0.55), cls=torch.zeros(B, dtype=torch.int32, device="cuda")))
                s = HeunSampler(net, B, K, N, "cuda", launches=form, classes=2)
                arms[f"classes {form}, 1 of 5 class 1"] = (s, dict(T0=(T0, 0.55), cls=(torch.arange(B, device="cuda") % 5 == 4).int()))
        ms = {a: [] for a in arms}
        for rep in range(WARM + REP):
            for a, (s, kw) in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); s.run(cvec, centre, x0, **kw); e1.record(); torch.cuda.synchronize()
                if rep >= WARM: ms[a].append(e0.elapsed_time(e1))
        for a, (s, _) in arms.items():
            say(f"  {B * K:6d} rows plan {s.plan:3d} {a:32s} {mmm(ms[a])}   {s.kernel_name}")

def _sequence(seed, F, n_obj):
    from genpose_amd import synth
    seq = synth.posed_sequence(seed, n_frames=F, n_obj=n_obj)
    gt0 = torch.eye(4).repeat(n_obj, 1, 1)
    gt0[:, :3, :3], gt0[:, :3, 3] = torch.from_numpy(seq["R"][0]).float(), torch.from_numpy(seq["t"][0]).float()
    return seq, gt0, [torch.from_numpy(seq["pts"][f]).float().cuda() for f in range(F)]

def _errors(seq, f, avg):
    sym = np.isin(seq["cat"], (0, 1, 3))
    Ra, Rg = avg[:, :3, :3].double().cpu().numpy(), seq["R"][f]
    cos_full = np.clip((np.trace(Ra @ Rg.transpose(0, 2, 1), axis1=1, axis2=2) - 1) / 2, -1, 1)
    cos_y = np.clip(np.sum(Ra[:, :, 1] * Rg[:, :, 1], axis=1), -1, 1)
    return np.degrees(np.arccos(np.where(sym, cos_y, cos_full))), np.linalg.norm(avg[:, :3, 3].cpu().numpy() - seq["t"][f], axis=1) * 100

if PART == "frame":
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import FixedStepTracker
    from genpose_amd.sde import SIGMA_MAX, SIGMA_MIN
    F, n_obj, K, N, WARM, ACQ = 30, 5, 50, 8, 6, 0.55
    seq, gt0, clouds = _sequence(3, F, n_obj)
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    ea = tr._agent("energy")
    mk = lambda **kw: FixedStepTracker(tr._agent("score", "heun", N), ea, steps=N, repeat_num=K, T0=0.15, seed=7, **kw)
    for form in ("single", "chain"):
        gt5, gt4, pr_acq, pr_steady = mk(launches=form), mk(launches=form), mk(launches=form, init="prior", acquire_T0=ACQ), mk(launches=form, init="prior", acquire_T0=ACQ)
        # the parent's user: the fifth object's solve from the prior at acquire_T0 on a stand-alone sampler (its cloud embedding is taken as given)
        net = gt4.sampling_agent.net
        net._need_weights()
        fifth = HeunSampler(net.pose_score_net, 1, K, N, "cuda", launches=form)
        cvec5 = torch.randn(1, 768, device="cuda")
        cen5, x5 = torch.zeros(1, 3, device="cuda"), torch.randn(K, 9, device="cuda") * float(SIGMA_MIN * (SIGMA_MAX / SIGMA_MIN) ** ACQ)
        def two_solves(f):
            gt4.step([(clouds[f][:4], names[:4], gt0[:4])])
            fifth.run(cvec5, cen5, x5, T0=ACQ)
        arms = {
            "prior, one of five acquired": lambda f: pr_acq.step([(clouds[f], names[:4] + [f"new{f}"], None)]),
            "gt, four objects + separate solve": two_solves,
            "gt, five objects (uniform)": lambda f: gt5.step([(clouds[f], names, gt0)]),
            "prior, five objects, none acquired": lambda f: pr_steady.step([(clouds[f], names, None)]),
        }
        ms = {a: [] for a in arms}
        for f in range(F):
            for a, fn in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(f)
                torch.cuda.synchronize()
                if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
            assert pr_acq.last_stats["acquired"] == (5 if f == 0 else 1) and pr_steady.last_stats["acquired"] == (5 if f == 0 else 0)
        say(f"launches='{form}': {F} frames x {n_obj} objects x K = {K}, N = {N}, energy ranker, trained checkpoints; host clock around the arm + synchronize, arms alternating per "
            f"frame, frames {WARM}.. timed; ms per frame, median [min, max]")
        med = {a: statistics.median(v) for a, v in ms.items()}
        for a in arms:
            say(f"  {a:36s} {mmm(ms[a])} ms")
        two, uni = "gt, four objects + separate solve", "gt, five objects (uniform)"
        say(f"  two solves / mixed = {med[two] / med['prior, one of five acquired']:.3f}x   mixed median below the two-solve arm's minimum: {med['prior, one of five acquired'] < min(ms[two])}   "
            f"mixed / uniform gt = {med['prior, one of five acquired'] / med[uni]:.3f}x   prior with nothing acquired / uniform gt = {med['prior, five objects, none acquired'] / med[uni]:.3f}x")
        say(f"  captures: prior-acquiring {pr_acq.captures}, prior-steady {pr_steady.captures}, gt5 {gt5.captures}; {pr_acq.last_stats}")

if PART == "quality":
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import FixedStepTracker
    F, n_obj, K = 30, 5, 50
    seq, gt0, clouds = _sequence(3, F, n_obj)
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {}
    for N in (8, 16):
        mk = lambda **kw: FixedStepTracker(tr._agent("score", "heun", N), ea, steps=N, repeat_num=K, T0=0.15, seed=7, launches="single", **kw)
        arms[f"N={N:2d} init='gt'"] = mk()
        for acq in (0.55, 1.0):
            arms[f"N={N:2d} init='prior' acquire_T0={acq}"] = mk(init="prior", acquire_T0=acq)
    err = {a: [] for a in arms}
    for f in range(F):
        for a, t in arms.items():
            out = t.step([(clouds[f], names, None if "prior" in a else gt0)])[0]
            err[a].append(_errors(seq, f, out["average_sRT"]))
    say(f"one sequence (seed 3), {F} frames x {n_obj} objects x K = {K}, trained checkpoints, energy ranker, seed 7; error of the aggregated pose against the ground truth")
    for a in arms:
        r, t = np.array([e[0] for e in err[a]]), np.array([e[1] for e in err[a]])
        say(f"  {a:36s} median over objects and frames {np.median(r):5.2f} deg {np.median(t):5.2f} cm; frame 0 {np.median(r[0]):5.2f} deg {np.median(t[0]):5.2f} cm; frames 1.. "
            f"{np.median(r[1:]):5.2f} deg {np.median(t[1:]):5.2f} cm; worst frame {np.median(r, axis=1).max():5.2f} deg {np.median(t, axis=1).max():5.2f} cm; last frame "
            f"{np.median(r[-1]):5.2f} deg {np.median(t[-1]):5.2f} cm")
        say("      per frame, median over objects: rotation deg " + " ".join(f"{np.median(e[0]):.1f}" for e in err[a]) + " | translation cm " + " ".join(f"{np.median(e[1]):.2f}" for e in err[a]))
