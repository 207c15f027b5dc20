"""Measurements of the DPM-Solver++(2M) fixed-step sampler beside the Heun one (profiles/dpm2m_sampler.txt), one session per part:
  time     Dpm2mSampler N = 8 / 16 / 32 against HeunSampler N = 4 / 8 / 16 / 32 (equal NFE and equal N): 256 clouds x 50 from T0 = 0.55, ten
           64-cloud batches x 50 from T0 = 1, 5 clouds x 50 from T0 = 0.15 as a chain and as one launch; HIP events around run() on warmed,
           captured samplers, the arms alternating in one loop, median [min, max]; seeded random weights;
  proxy    the accuracy proxy of tests/test_gpu_trained_regime.py (512 held-out instances, trained checkpoints, shared prior draws) for
           RK45, Heun and DPM-Solver++(2M) at N = 8 / 16 / 32, and the candidates' median distance to the RK45 candidates;
  tracker  a 30-frame synthetic sequence of 5 moving objects, K = 50, trained checkpoints: FixedStepTracker solver='heun' against 'dpm2m',
           N = 8 / 16 - host clock around step() + synchronize per frame, the arms alternating frame by frame - and the aggregated pose's
           error against the ground truth per arm.
python scratch/dpm2m_measure.py time|proxy|tracker [out file]"""
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

if PART == "time":
    from genpose_amd.samplers import Dpm2mSampler, HeunSampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")
    K, WARM, REP = 50, 3, 9
    say(f"HIP events around sampler.run (three input copies + one graph replay), {WARM} warm-up + {REP} timed repeats, arms alternating, ms, median [min, max]")
    for name, B, groups, T0, forms in (("256 clouds x 50 (12 800 rows), T0 = 0.55", 256, 1, 0.55, ("chain",)),
                                       ("ten 64-cloud batches x 50 (32 000 rows), T0 = 1", 640, 10, 1.0, ("chain",)),
                                       ("tracking: 5 clouds x 50 (250 rows), T0 = 0.15", 5, 1, 0.15, ("chain", "single"))):
        gen = torch.Generator().manual_seed(B)
        cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
        sig = 0.01 * (50.0 / 0.01) ** T0
        centre, x0 = (torch.randn(B, 3, generator=gen) * 0.3).cuda(), (torch.randn(B * K, 9, generator=gen) * sig).cuda()
        arms = {}
        for form in forms:
            for N in (8, 16, 32):
                arms[f"Dpm2mSampler N = {N:2d} {form}"] = Dpm2mSampler(net, B, K, N, "cuda", groups=groups, launches=form)
            for N in (4, 8, 16, 32):
                arms[f"HeunSampler  N = {N:2d} {form}"] = HeunSampler(net, B, K, N, "cuda", groups=groups, launches=form)
        ms = {a: [] for a in arms}
        for rep in range(WARM + REP):
            for a, s in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); s.run(cvec, centre, x0, T0=T0); e1.record(); torch.cuda.synchronize()
                if rep >= WARM: ms[a].append(e0.elapsed_time(e1))
        say(f"  {name}")
        for a, s in arms.items():
            st = s.last_stats
            say(f"    {a:32s} ({st['kernel_name']}, nfev {st['nfev']}, launches {st['nlaunch']}, captures {s.captures}): {mmm(ms[a])}   per evaluation {statistics.median(ms[a]) / st['nfev'] * 1e3:.1f} us")
        med = lambda a: statistics.median(ms[a])
        for form in forms:
            say(f"    {form}: DPM++2M / Heun at equal N   = " + "  ".join(f"N {N}: {med(f'Dpm2mSampler N = {N:2d} {form}') / med(f'HeunSampler  N = {N:2d} {form}'):.3f}" for N in (8, 16, 32)))
            say(f"    {form}: DPM++2M / Heun at equal NFE = " + "  ".join(f"NFE {N}+1: {med(f'Dpm2mSampler N = {N:2d} {form}') / med(f'HeunSampler  N = {N // 2:2d} {form}'):.3f}" for N in (8, 16, 32)))
        del arms

def _rot(p):
    c1, c2 = p[..., 0:3], p[..., 3:6]
    return np.stack([c1, c2, np.cross(c1, c2)], -1)

if PART == "proxy":
    import test_gpu_trained_regime as tr
    from oracle import genpose_oracle as go

    def _batch(sa, ea, pts, prior):
        """one batch as SingleFrameRunner.infer_tensors runs it, the prior draw injected (test_gpu_trained_regime._hip_batch)"""
        from genpose_amd import reward, rotation
        from genpose_amd.runner import make_batch_sample
        sa.net.prior_fn = lambda shape, T=1.0: prior * float(go.ve_sigma(T))
        sample = make_batch_sample(pts)
        pred = sa.pred_func(data=sample, repeat_num=tr.K, save_path=None, T0=tr.T0)
        energy = ea.get_energy(data=sample, pose_samples=pred, T=1e-5)
        r = reward.rank_aggregate(pred, energy, ratio=tr.RATIO)
        return {"pred": pred.cpu().clone(), "sorted_energy": r["sorted_energy"].cpu().clone(), "sorted_RTs": rotation.pose9_to_RT(r["sorted_poses"]).cpu().clone()}
    NI, NB = 512, 256
    d = tr._posed(NI)
    ea = tr._agent("energy")
    priors = [torch.randn(NB * tr.K, 9, generator=torch.Generator().manual_seed(1000 + b)) for b in range(NI // NB)]
    arms = [("RK45 (rtol = atol = 1e-5)", tr._agent("score"))]
    for solver, label in (("heun", "Heun"), ("dpm2m", "DPM++2M")):
        for N in (8, 16, 32):
            arms.append((f"{label} N = {N}", tr._agent("score", solver, N)))
    keys = ["5deg2cm", "5deg5cm", "10deg2cm", "10deg5cm", "10deg10cm"]
    say(f"accuracy proxy: {NI} held-out synthetic instances, trained checkpoints, K = {tr.K}, T0 = {tr.T0}, top {int(tr.RATIO * 100)} % by energy averaged, shared prior "
        "draws; evaluation.compute_mAP, mean AP over the six categories, percent; median distance of the K x instances candidate poses to the RK45 run's")
    say(f"{'':40s}" + "".join(f"{k:>11s}" for k in keys) + "   nfev   median rot (deg) / trans (mm) to RK45")
    ref, rows = None, {}
    for name, sa in arms:
        runs = [_batch(sa, ea, torch.from_numpy(d["pts"][NB * b:NB * (b + 1)]).cuda(), priors[b]) for b in range(NI // NB)]
        cat = lambda key: np.concatenate([np.asarray(r[key]) for r in runs], 0)
        s = tr._proxy(d, cat("sorted_RTs"), cat("sorted_energy"))
        pred = cat("pred").astype(np.float64).reshape(-1, 9)
        nfev = sa.net.last_sampler.last_stats["nfev"]
        dist = ""
        if ref is None:
            ref = pred
        else:
            tr_ = np.einsum("nij,nij->n", _rot(pred), _rot(ref))
            ang = np.degrees(np.arccos(np.clip((tr_ - 1) / 2, -1, 1)))
            dist = f"{np.median(ang):.4f} / {np.median(np.linalg.norm(pred[:, 6:] - ref[:, 6:], axis=1)) * 1e3:.4f}"
        rows[name] = s
        say(f"{name:40s}" + "".join(f"{s[k]:11.2f}" for k in keys) + f"  {nfev:5d}   {dist}")
    base = rows[arms[0][0]]
    for name, _ in arms[1:]:
        dl = {k: rows[name][k] - base[k] for k in keys[:4]}
        say(f"{name + ' - RK45':40s}" + "".join(f"{dl[k]:+11.2f}" for k in keys[:4]) + f"   inside +-2 pt at all four thresholds: {all(abs(v) <= 2.0 for v in dl.values())}")

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

if PART == "tracker":
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import FixedStepTracker, TrackingRunner
    F, n_obj, K, WARM = 30, 5, 50, 6
    seq, gt0, clouds = _sequence(3, F, n_obj)
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {"rk45 TrackingRunner": TrackingRunner(tr._agent("score"), ea, repeat_num=K, T0=0.15)}
    for N in (8, 16):
        for solver in ("heun", "dpm2m"):
            for form in ("single", "chain"):
                arms[f"fixed {solver:5s} N={N:2d} {form:6s}"] = FixedStepTracker(tr._agent("score", "heun", N), ea, steps=N, repeat_num=K, T0=0.15, seed=7, launches=form,
                                                                              solver=solver)
    ms, err = {a: [] for a in arms}, {a: [] for a in arms}
    for f in range(F):
        for a, t in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.step(clouds[f], names, gt0) if a.startswith("rk45") else t.step([(clouds[f], names, gt0)])[0]
            torch.cuda.synchronize()
            if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
            err[a].append(_errors(seq, f, out["average_sRT"]))
    say(f"one sequence, {F} frames x {n_obj} objects x K = {K}, trained checkpoints, energy ranker; host clock around step() + synchronize, arms alternating per frame, "
        f"frames {WARM}.. timed; ms per frame, median [min, max]")
    for a in arms:
        r, t = np.array([e[0] for e in err[a]]), np.array([e[1] for e in err[a]])
        say(f"  {a:28s} {mmm(ms[a])} ms   error vs ground truth, median over objects and frames: {np.median(r):.2f} deg {np.median(t):.2f} cm; worst frame (median over "
            f"objects) {np.median(r, axis=1).max():.2f} deg {np.median(t, axis=1).max():.2f} cm; last frame {np.median(r[-1]):.2f} deg {np.median(t[-1]):.2f} cm"
            + ("" if a.startswith("rk45") else f"; nfev {arms[a].last_stats['nfev']}, {arms[a].last_stats['kernel']}"))
