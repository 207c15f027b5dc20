"""Measurements of the one-launch Heun solve and of runner.FixedStepTracker (profiles/fixed_step_tracking.txt), one session per part:
  solve  HeunSampler(launches='chain') against launches='single' on the same plan: 250 / 800 / 3 200 / 12 800 rows (K = 50), N = 8 / 16,
         T0 = 0.15; HIP events around run() on warmed, captured samplers, the arms alternating in one loop, median [min, max]; the two arms'
         outputs are compared bit for bit at every size;
  frame  a 30-frame synthetic sequence of 5 moving objects, K = 50, trained checkpoints: TrackingRunner (RK45, frame graphs) against
         FixedStepTracker N = 8 / 16, 'chain' / 'single', energy / likelihood ranker - host clock around step() + synchronize per frame,
         the arms alternating frame by frame - and the aggregated pose's error against the ground truth per arm;
  multi  128 such sequences sharing the launches: MultiSequenceTracker against FixedStepTracker.
python scratch/fixed_step_tracking_measure.py solve|frame|multi [out file]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
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

say(f"== {PART}: device {torch.cuda.get_device_name(0)}")

if PART == "solve":
    from genpose_amd.samplers import HeunSampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    K, T0, WARM, REP = 50, 0.15, 3, 15
    say(f"HIP events around HeunSampler.run (three input copies + one graph replay), {WARM} warm-up + {REP} timed repeats, arms alternating, ms, median [min, max]")
    for B in (5, 16, 64, 256):
        gen = torch.Generator().manual_seed(B)
        cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
        centre, x0 = (torch.randn(B, 3, generator=gen) * 0.3).cuda(), (torch.randn(B * K, 9, generator=gen) * 0.0358).cuda()
        auto = HeunSampler(net, B, K, 8, "cuda").plan
        for tile in sorted({auto if auto != 128 else 64, 16}):
            for N in (8, 16):
                try:
                    arms = {"chain": HeunSampler(net, B, K, N, "cuda", tile=tile), "single": HeunSampler(net, B, K, N, "cuda", tile=tile, launches="single")}
                except ValueError as e:
                    say(f"  {B * K:6d} rows tile {tile}: {e}")
                    continue
                if auto == 128:
                    arms["chain128"] = HeunSampler(net, B, K, N, "cuda")
                ms, pose = {a: [] for a in arms}, {}
                for rep in range(WARM + REP):
                    for a, s in arms.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(); _, p = s.run(cvec, centre, x0, T0=T0); e1.record(); torch.cuda.synchronize()
                        pose[a] = p.clone()
                        if rep >= WARM: ms[a].append(e0.elapsed_time(e1))
                same = torch.equal(pose["chain"], pose["single"])
                med = {a: statistics.median(v) for a, v in ms.items()}
                say(f"  {B * K:6d} rows ({(B * K + tile - 1) // tile:4d} workgroups of {tile}, auto plan {auto}) N = {N:2d}: " + "   ".join(f"{a} {mmm(ms[a])}" for a in arms)
                    + f"   chain / single = {med['chain'] / med['single']:.2f}x   single median below chain minimum: {med['single'] < min(ms['chain'])}   same bits: {same}")
                del arms

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
    from genpose_amd.runner import FixedStepTracker, TrackingRunner
    F, n_obj, K, WARM = 30, 5, 50, 6
    seq, gt0, clouds = _sequence(3, F, n_obj)
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    sa_ode, ea = tr._agent("score"), tr._agent("energy")
    arms = {"rk45 TrackingRunner": TrackingRunner(sa_ode, ea, repeat_num=K, T0=0.15)}
    for N in (8, 16):
        for ranker in ("energy", "likelihood"):
            for form in ("chain", "single"):
                sa = tr._agent("score", "heun", N)
                arms[f"fixed N={N:2d} {form:6s} {ranker}"] = FixedStepTracker(sa, ea if ranker == "energy" else None, steps=N, repeat_num=K, T0=0.15, ranker=ranker,
                                                                              seed=7, launches=form)
    ms, err, avg = {a: [] for a in arms}, {a: [] for a in arms}, {a: [] for a in arms}
    for f in range(F):
        for a, t in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.step(clouds[f], names, gt0) if a.startswith("rk45") else t.step([(clouds[f], names, gt0)])[0]
            torch.cuda.synchronize()
            if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
            err[a].append(_errors(seq, f, out["average_sRT"]))
            avg[a].append(out["average_sRT"].double().cpu())
    say(f"one sequence, {F} frames x {n_obj} objects x K = {K}, trained checkpoints; host clock around step() + synchronize, arms alternating per frame, frames {WARM}.. timed; ms per frame, median [min, max]")
    ref = "rk45 TrackingRunner"
    for a in arms:
        r, t = np.array([e[0] for e in err[a]]), np.array([e[1] for e in err[a]])
        d = torch.stack(avg[a]) - torch.stack(avg[ref])
        say(f"  {a:32s} {mmm(ms[a])} ms   rk45 / this = {statistics.median(ms[ref]) / statistics.median(ms[a]):.2f}x   error vs ground truth, median over objects and frames: "
            f"{np.median(r):.2f} deg {np.median(t):.2f} cm; worst frame (median over objects) {np.median(r, axis=1).max():.2f} deg {np.median(t, axis=1).max():.2f} cm; "
            f"last frame {np.median(r[-1]):.2f} deg {np.median(t[-1]):.2f} cm; distance to rk45's pose: translation median {float(d[:, :, :3, 3].norm(dim=-1).median()) * 100:.3f} cm, "
            f"rotation entries max {float(d[:, :, :3, :3].abs().max()):.3f}" + ("" if a == ref else f"; {arms[a].last_stats}"))
    for a in (ref, "fixed N= 8 single energy", "fixed N=16 single energy", "fixed N= 8 single likelihood"):
        say(f"  per frame, median over objects, {a}: rotation deg " + " ".join(f"{np.median(e[0]):.1f}" for e in err[a]) + " | translation cm " + " ".join(f"{np.median(e[1]):.2f}" for e in err[a]))

if PART == "multi":
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import FixedStepTracker, MultiSequenceTracker
    S, F, n_obj, K, WARM = 128, 10, 5, 50, 3
    seqs = [_sequence(100 + s, F, n_obj) for s in range(8)]  # eight distinct sequences, each used by sixteen trackers' slots
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {"rk45 MultiSequenceTracker": MultiSequenceTracker(tr._agent("score"), ea, S, repeat_num=K, T0=0.15)}
    for N in (8, 16):
        for form in ("chain", "single", None):
            arms[f"fixed N={N:2d} {str(form):6s} energy"] = FixedStepTracker(tr._agent("score", "heun", N), ea, steps=N, repeat_num=K, T0=0.15, seed=7, launches=form)
    ms = {a: [] for a in arms}
    for f in range(F):
        frames = [(seqs[s % 8][2][f], names, seqs[s % 8][1]) for s in range(S)]
        for a, t in list(arms.items()):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                t.step(frames)
            except ValueError as e:  # launches='single' where the plan of the step's rows is the 128-row chain form
                say(f"  {a}: {e}")
                del arms[a], ms[a]
                continue
            torch.cuda.synchronize()
            if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
    say(f"{S} sequences sharing the launches ({S * n_obj} clouds, {S * n_obj * K} rows), {F} frames, frames {WARM}.. timed; ms per step, median [min, max]")
    ref = "rk45 MultiSequenceTracker"
    for a in arms:
        say(f"  {a:32s} {mmm(ms[a])} ms   rk45 / this = {statistics.median(ms[ref]) / statistics.median(ms[a]):.2f}x   per sequence {statistics.median(ms[a]) / S * 1e3:.1f} us"
            + ("" if a == ref else f"; {arms[a].last_stats}"))
