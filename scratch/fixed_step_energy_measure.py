"""Measurements of the fixed-step solvers on the ENERGY model and of the one-network pipelines (profiles/fixed_step_energy.txt):
  launch  per launch, against the PC energy step of the same session: heun_step_chain_kernel<2,energy> / dpm2m_... at 32 000 rows against
          pc_step_chain_kernel<2,1>, the 16-row forms at 250 and 3 200 rows against pc_step_kernel<16,1>; HIP events around the replay of
          each sampler's captured chain (ten launches in every arm), divided by the launches; seeded random weights;
  solve   the one-launch solve against its chain at 250 and 3 200 rows (plan 16), N = 8, both solvers; outputs compared bit for bit;
  frame   a 30-frame synthetic sequence of 5 moving objects, K = 50, trained checkpoints: FixedStepTracker(sample_from='energy') against the
          two-network FixedStepTracker (score solve + energy ranker), N = 8 / 16, both solvers - host clock around step() + synchronize per
          frame - and the aggregated pose's error against the ground truth per arm;
  single  256 clouds x 50: SingleFrameRunner(sample_from='energy') against the two-network runner, DPM-Solver++(2M) at N = 8 / 16 / 32;
  proxy   the accuracy proxy of tests/test_gpu_trained_regime.py (512 held-out instances, trained checkpoints, shared prior draws):
          score-sampled + energy-ranked (RK45, DPM-Solver++(2M)) against energy-sampled + energy-ranked (DPM-Solver++(2M) N = 8 / 16 / 32,
          Heun N = 16).
The arms of a part alternate within one loop; median [min, max].
python scratch/fixed_step_energy_measure.py launch|solve|frame|single|proxy [out file]
python scratch/fixed_step_energy_measure.py all [out file]   every part as a child process under its own time limit; a failure ends the run"""
import os, statistics, subprocess, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

PART = sys.argv[1]
LIMITS = {"launch": 150, "solve": 120, "frame": 240, "single": 180, "proxy": 420}  # seconds per part
if PART == "all":  # (this process never touches the device)
    for part, limit in LIMITS.items():
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), part] + sys.argv[2:3], timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"part {part} ended with status {rc}: stopping", flush=True)
            sys.exit(rc)
    sys.exit(0)

import numpy as np, torch
torch.set_num_threads(16)
OUT = open(sys.argv[2], "a") if len(sys.argv) > 2 else None
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.3f} [{min(v) * scale:.3f}, {max(v) * scale:.3f}]"

say(f"== {PART}: device {torch.cuda.get_device_name(0)}")

def _replay_ms(arms, prepare, warm, rep):
    """HIP events around the replay of each arm's captured graph, the arms alternating; prepare(arm) puts its inputs back first (untimed)"""
    ms = {a: [] for a in arms}
    for r in range(warm + rep):
        for a, s in arms.items():
            prepare(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); s.graph.replay(); e1.record(); torch.cuda.synchronize()
            if r >= warm: ms[a].append(e0.elapsed_time(e1))
    return ms

if PART in ("launch", "solve"):
    from genpose_amd.samplers import Dpm2mSampler, HeunSampler, PCSampler
    from genpose_amd.scorenet import ScoreNetHIP
    from genpose_amd.weights_synth import make_state_dict
    net = ScoreNetHIP(make_state_dict(0, "energy"), "cuda")
    K, T0, WARM, REP = 50, 0.15, 3, 15
    sig = 0.01 * (50.0 / 0.01) ** T0

    def _inputs(B):
        gen = torch.Generator().manual_seed(B)
        cvec = net.cloud_embed(torch.randn(B, 1024, generator=gen).abs().cuda())
        return cvec, (torch.randn(B, 3, generator=gen) * 0.3).cuda(), (torch.randn(B * K, 9, generator=gen) * sig).cuda()

if PART == "launch":
    say(f"HIP events around the replay of the captured chain (kernels only; ten launches per arm: Heun N = 4 with denoise, DPM++2M N = 8 with denoise, PC n = 9), "
        f"{WARM} warm-up + {REP} timed, arms alternating; us per launch = replay / 10, median [min, max].  Energy network, seeded random weights, T0 = {T0}")
    for B, tile in ((5, 16), (64, 16), (640, 128)):
        cvec, centre, x0 = _inputs(B)
        arms = {"heun  energy": HeunSampler(net, B, K, 4, "cuda", tile=tile, model="energy"), "dpm2m energy": Dpm2mSampler(net, B, K, 8, "cuda", tile=tile, model="energy"),
                "pc    energy": PCSampler(net, B, K, 9, "cuda", tile=tile, model="energy")}
        for a, s in arms.items():  # the first run captures
            s.run(cvec, centre, x0, **({} if a.startswith("pc") else {"T0": T0}))
            assert (s.n + 1 if a.startswith("pc") else s.nlaunch) == 10
        torch.cuda.synchronize()
        ms = _replay_ms(arms, lambda s: s.x.copy_(x0), WARM, REP)
        say(f"  {B * K:6d} rows, plan {tile}")
        pc = statistics.median(ms["pc    energy"])
        for a, s in arms.items():
            say(f"    {a} ({s.kernel_name:34s}): {mmm(ms[a], 100.0)} us per launch   / pc = {statistics.median(ms[a]) / pc:.3f}")

if PART == "solve":
    say(f"HIP events around the replay of the captured solve, {WARM} warm-up + {REP} timed, arms alternating, ms, median [min, max]; plan 16, N = 8, T0 = {T0}")
    for B in (5, 64):
        cvec, centre, x0 = _inputs(B)
        for cls in (HeunSampler, Dpm2mSampler):
            arms = {"chain": cls(net, B, K, 8, "cuda", tile=16, model="energy"), "single": cls(net, B, K, 8, "cuda", tile=16, model="energy", launches="single")}
            pose = {a: s.run(cvec, centre, x0, T0=T0)[1].clone() for a, s in arms.items()}
            torch.cuda.synchronize()
            ms = _replay_ms(arms, lambda s: s.x.copy_(x0), WARM, REP)
            med = {a: statistics.median(v) for a, v in ms.items()}
            say(f"  {B * K:6d} rows {arms['single'].kernel_name:30s}: " + "   ".join(f"{a} {mmm(ms[a])}" for a in arms) + f"   chain / single = {med['chain'] / med['single']:.2f}x   "
                f"single median below chain minimum: {med['single'] < min(ms['chain'])}   same bits: {torch.equal(pose['chain'], pose['single'])}")

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
    F, n_obj, K, WARM = 30, 5, 50, 6
    seq, gt0, clouds = _sequence(3, F, n_obj)
    names = [f"obj{o}" for o in range(n_obj)]
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {}
    for N in (8, 16):
        for solver in ("heun", "dpm2m"):
            arms[f"two networks {solver:5s} N={N:2d}"] = FixedStepTracker(tr._agent("score", "heun", N), ea, steps=N, repeat_num=K, T0=0.15, seed=7, solver=solver)
            arms[f"one network  {solver:5s} N={N:2d}"] = FixedStepTracker(None, ea, steps=N, repeat_num=K, T0=0.15, seed=7, solver=solver, sample_from="energy")
    ms, err = {a: [] for a in arms}, {a: [] for a in arms}
    for f in range(F):
        for a, t in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.step([(clouds[f], names, gt0)])[0]
            torch.cuda.synchronize()
            if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
            err[a].append(_errors(seq, f, out["average_sRT"]))
    say(f"one sequence, {F} frames x {n_obj} objects x K = {K}, trained checkpoints, energy ranker, launches=None; host clock around step() + synchronize, arms "
        f"alternating per frame, frames {WARM}.. timed; ms per frame, median [min, max]")
    for a in arms:
        r, t = np.array([e[0] for e in err[a]]), np.array([e[1] for e in err[a]])
        st = arms[a].last_stats
        say(f"  {a:28s} {mmm(ms[a])} ms   error vs ground truth, median over objects and frames: {np.median(r):.2f} deg {np.median(t):.2f} cm; worst frame (median over "
            f"objects) {np.median(r, axis=1).max():.2f} deg {np.median(t, axis=1).max():.2f} cm; last frame {np.median(r[-1]):.2f} deg {np.median(t[-1]):.2f} cm; "
            f"replays {st['replays']}, nfev {st['nfev']}, {st['kernel']}")
    for N in (8, 16):
        for solver in ("heun", "dpm2m"):
            one, two = statistics.median(ms[f"one network  {solver:5s} N={N:2d}"]), statistics.median(ms[f"two networks {solver:5s} N={N:2d}"])
            say(f"  {solver} N = {N}: one network / two networks = {one / two:.3f} ({one - two:+.3f} ms)")

if PART == "single":
    import test_gpu_trained_regime as tr
    from genpose_amd.runner import SingleFrameRunner
    B, WARM, REP = 256, 3, 9
    clouds = torch.from_numpy(tr._posed(B)["pts"]).float().cuda()
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {}
    for N in (8, 16, 32):
        arms[f"two networks dpm2m N={N:2d}"] = SingleFrameRunner(tr._agent("score", "dpm2m", N), ea, repeat_num=tr.K, T0=tr.T0, batch_size=B)
        arms[f"one network  dpm2m N={N:2d}"] = SingleFrameRunner(None, tr._agent("energy", "dpm2m", N, fixed_step_energy=True), repeat_num=tr.K, T0=tr.T0, batch_size=B,
                                                                 sample_from="energy")
    ms = {a: [] for a in arms}
    for r in range(WARM + REP):
        for a, run in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run.infer_tensors(clouds)
            torch.cuda.synchronize()
            if r >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
    say(f"{B} clouds x {tr.K} candidates, T0 = {tr.T0}, trained checkpoints, energy ranker: host clock around SingleFrameRunner.infer_tensors + synchronize (prior drawn on "
        f"the host, encoder(s), solve, energies, ranking, 4x4 poses), {WARM} warm-up + {REP} timed, arms alternating; ms, median [min, max]")
    for a, run in arms.items():
        smp = (run.energy_agent if run.sample_from == "energy" else run.score_agent).net.last_sampler
        say(f"  {a:28s} {mmm(ms[a])} ms   {smp.kernel_name}, nfev {smp.last_stats['nfev']}")
    for N in (8, 16, 32):
        one, two = statistics.median(ms[f"one network  dpm2m N={N:2d}"]), statistics.median(ms[f"two networks dpm2m N={N:2d}"])
        say(f"  N = {N}: one network / two networks = {one / two:.3f} ({one - two:+.3f} ms)")

if PART == "proxy":
    import test_gpu_trained_regime as tr
    from oracle import genpose_oracle as go

    def _batch(sampling_agent, ea, pts, prior, one_network):
        """one batch as SingleFrameRunner.infer_tensors runs it, the prior draw injected (test_gpu_trained_regime._hip_batch)"""
        from genpose_amd import reward, rotation
        from genpose_amd.runner import make_batch_sample
        sampling_agent.net.prior_fn = lambda shape, T=1.0: prior * float(go.ve_sigma(T))
        sample = make_batch_sample(pts)
        pred = sampling_agent.pred_func(data=sample, repeat_num=tr.K, save_path=None, T0=tr.T0)
        energy = (sampling_agent.get_energy(data=sample, pose_samples=pred, T=1e-5, extract_pts_feature=False) if one_network
                  else ea.get_energy(data=sample, pose_samples=pred, T=1e-5))
        r = reward.rank_aggregate(pred, energy, ratio=tr.RATIO)
        return {"sorted_energy": r["sorted_energy"].cpu().clone(), "sorted_RTs": rotation.pose9_to_RT(r["sorted_poses"]).cpu().clone()}
    NI, NB = 512, 256
    d = tr._posed(NI)
    ea = tr._agent("energy")
    priors = [torch.randn(NB * tr.K, 9, generator=torch.Generator().manual_seed(1000 + b)) for b in range(NI // NB)]
    arms = [("score-sampled RK45 (rtol = atol = 1e-5)", tr._agent("score"), False)]
    arms += [(f"score-sampled DPM++2M N = {N}", tr._agent("score", "dpm2m", N), False) for N in (8, 16, 32)]
    arms += [(f"energy-sampled DPM++2M N = {N}", tr._agent("energy", "dpm2m", N, fixed_step_energy=True), True) for N in (8, 16, 32)]
    arms += [("energy-sampled Heun N = 16", tr._agent("energy", "heun", 16, fixed_step_energy=True), True)]
    keys = ["5deg2cm", "5deg5cm", "10deg2cm", "10deg5cm"]
    say(f"accuracy proxy: {NI} held-out synthetic instances, trained checkpoints, K = {tr.K}, T0 = {tr.T0}, top {int(tr.RATIO * 100)} % by energy averaged, shared prior "
        "draws, every arm ranked by the energy model; evaluation.compute_mAP, mean AP over the six categories, percent")
    say(f"{'':44s}" + "".join(f"{k:>11s}" for k in keys) + "   nfev")
    rows = {}
    for name, agent, one in arms:
        runs = [_batch(agent, ea, torch.from_numpy(d["pts"][NB * b:NB * (b + 1)]).cuda(), priors[b], one) for b in range(NI // NB)]
        cat = lambda key: np.concatenate([np.asarray(r[key]) for r in runs], 0)
        s = rows[name] = tr._proxy(d, cat("sorted_RTs"), cat("sorted_energy"))
        st = getattr(agent.net, "last_sampler", None)
        say(f"{name:44s}" + "".join(f"{s[k]:11.2f}" for k in keys) + f"  {st.last_stats['nfev'] if st is not None else -1:5d}")
    base = rows[arms[0][0]]
    for name, _, _ in arms[1:]:
        dl = {k: rows[name][k] - base[k] for k in keys}
        say(f"{name + ' - RK45':44s}" + "".join(f"{dl[k]:+11.2f}" for k in keys) + f"   inside +-2 pt at all four thresholds: {all(abs(v) <= 2.0 for v in dl.values())}")
