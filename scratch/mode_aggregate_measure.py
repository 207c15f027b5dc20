"""Measurements of the mode-seeking aggregation (reward.mode_aggregate, csrc/rank.hip; profiles/mode_aggregate.txt), one session per part:
  launch  gp_mode_aggregate (every output written, the top 60 % per column as the weight) beside gp_rank_aggregate_rt, 5 x 50, 256 x 50,
          5 x 512 and 256 x 512: HIP events around 20 back-to-back raw launches on preallocated buffers, the arms alternating in one loop,
          microseconds per launch, median [min, max]; then a SingleFrameRunner.infer_tensors frame (5 clouds, K = 50, trained checkpoints,
          energy ranker) with aggregate 'mode' against 'mean', host clock around the call + synchronize, arms alternating;
  proxy   the accuracy proxy on 512 held-out synthetic instances, trained checkpoints, the SAME ODE candidates under the energy, consensus
          and likelihood (RK45 exact) rankers, each with the mean and with the mode of the ranker's top 60 %, the mode over all candidates,
          and a bandwidth sweep {5, 10, 20} deg x {1, 2, 4} cm; GP_RANK_SEED picks the draws.
python scratch/mode_aggregate_measure.py launch|proxy [out file]"""
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
def mmm(v, scale=1.0): return f"{statistics.median(v) * scale:8.2f} [{min(v) * scale:.2f}, {max(v) * scale:.2f}]"

say(f"== {PART}: device {torch.cuda.get_device_name(0)}")
SYM_CATS = (0, 1, 3)  # synth's categories symmetric about y: bottle, bowl, can

if PART == "launch":
    import consensus_reference as cr
    import test_gpu_trained_regime as tr
    from genpose_amd import _lib, reward
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.runner import SingleFrameRunner
    INNER, WARM, REP = 20, 5, 31
    say(f"HIP events around {INNER} back-to-back launches, {WARM} warm-up + {REP} timed samples, arms alternating, us per launch, median [min, max]; float32 poses "
        "(tests/consensus_reference.make_clouds), sel = 60 %; the C entry points through ctypes on PREALLOCATED buffers, every output written; the mode at the "
        f"defaults ({reward.MODE_BW_ROT_DEG} deg, {reward.MODE_BW_TRANS} m, {reward.MODE_ITERS} iterations) with the ranking's top 60 % per column as the weight")
    L = _lib.lib()
    for B, K in ((5, 50), (256, 50), (5, 512), (256, 512)):
        poses = torch.from_numpy(cr.make_clouds(B + K, B, K)[0]).cuda()
        sel = max(1, int(0.6 * K))
        energy = reward.consensus_energy(poses)
        o = reward.rank_aggregate(poses, energy, selected_num=sel, with_rt=True)
        w = reward.selection_weight(o["order"], sel)
        m = reward.mode_aggregate(poses, None, w, with_rt=True)
        alls = torch.ones(B, dtype=torch.int8, device="cuda")
        st = stream_ptr()
        outs = [ptr(o[k]) for k in ("sorted_poses", "sorted_energy", "order", "avg_pose", "sorted_RTs", "avg_RT")]
        mouts = [ptr(m[k]) for k in ("density", "mode_pose", "mode_RT", "mass", "start")]
        hr, ht = float(np.deg2rad(reward.MODE_BW_ROT_DEG)), reward.MODE_BW_TRANS
        mode = lambda it=reward.MODE_ITERS, sy=None, ww=w, mo=mouts: L.gp_mode_aggregate(B, K, 0, ptr(poses), ptr(sy), ptr(ww), hr, ht, it, *mo, st)
        arms = {"rank_aggregate_rt": lambda: L.gp_rank_aggregate_rt(B, K, sel, 0, ptr(poses), ptr(energy), *outs, st),
                "mode_aggregate": mode, "mode_aggregate, symmetric": lambda: mode(sy=alls), "mode_aggregate, no weight": lambda: mode(ww=None),
                "mode_aggregate, 0 iterations": lambda: mode(it=0), "mode_aggregate, 64 iterations": lambda: mode(it=64),
                "mode_aggregate, density only": lambda: mode(mo=[mouts[0], None, None, None, None]),
                "wrapper: selection_weight + mode_aggregate": lambda: reward.mode_aggregate(poses, None, reward.selection_weight(o["order"], sel), with_rt=True)}
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
        say(f"  {B:3d} clouds x {K:3d} candidates")
        for a in arms: say(f"    {a:44s} {mmm(us[a])} us")
        say(f"    mode_aggregate / rank_aggregate_rt (medians): {statistics.median(us['mode_aggregate']) / statistics.median(us['rank_aggregate_rt']):.2f}x")
    # a frame of the single-frame runner
    n, K, WARMF, REPF = 5, 50, 3, 15
    d = tr._posed(n)
    clouds = torch.from_numpy(d["pts"]).cuda()
    sa, ea = tr._agent("score"), tr._agent("energy")
    runs = {a: SingleFrameRunner(sa, ea, repeat_num=K, aggregate=a) for a in ("mean", "mode")}
    ms = {a: [] for a in runs}
    for rep in range(WARMF + REPF):
        for a, run in runs.items():
            torch.manual_seed(rep)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = run.infer_tensors(clouds)
            torch.cuda.synchronize()
            if rep >= WARMF: ms[a].append((time.perf_counter() - t0) * 1e3)
    say(f"  SingleFrameRunner.infer_tensors, {n} clouds x K = {K}, ODE sampler from T0 = 0.55, energy ranker, trained checkpoints; host clock around the call + "
        f"synchronize, {WARMF} warm-up + {REPF} timed frames, arms alternating, the same seed per pair; ms per frame, median [min, max]")
    for a in runs: say(f"    aggregate={a!r:8s} {mmm(ms[a])} ms")
    say(f"    mode minus mean (medians): {statistics.median(ms['mode']) - statistics.median(ms['mean']):+.3f} ms; mode_mass of the last frame {out['mode_mass'].double().cpu().numpy().round(3).tolist()}")

if PART == "proxy":
    SEED, NI = int(os.environ.get("GP_RANK_SEED", "7")), int(os.environ.get("GP_RANK_INSTANCES", "512"))
    import test_gpu_trained_regime as tr
    from genpose_amd import evaluation, reward, rotation
    from genpose_amd.runner import make_batch_sample
    K, RATIO = 50, 0.6
    sel = max(1, int(K * RATIO))
    say(f"accuracy proxy: trained checkpoints, {NI} held-out synthetic instances (synth 1 000 000 ..) in batches of 256, K = {K} candidates from the ODE sampler at "
        f"T0 = 0.55, torch.manual_seed({SEED}); the same candidates under every arm.  'mean': the ranker's top 60 % averaged (gp_rank_aggregate_rt's avg_RT); 'mode': "
        f"gp_mode_aggregate on the same top 60 % per column as the weight, at {reward.MODE_BW_ROT_DEG} deg / {reward.MODE_BW_TRANS} m / {reward.MODE_ITERS} iterations "
        "unless the line says otherwise, symmetric categories by their y axis; every aggregated pose scored as a single hypothesis by evaluation.compute_mAP")
    d = tr._posed(NI)
    sym = torch.from_numpy(np.isin(d["cat"], SYM_CATS).astype(np.int8)).cuda()
    sa, ea = tr._agent("score"), tr._agent("energy")
    torch.manual_seed(SEED)
    preds, energies, lls = [], [], []
    for b in range(NI // 256):
        sample = make_batch_sample(torch.from_numpy(d["pts"][256 * b:256 * (b + 1)]).cuda())
        pred = sa.pred_func(data=sample, repeat_num=K, save_path=None, T0=0.55)
        preds.append(pred)
        energies.append(ea.get_energy(data=sample, pose_samples=pred, T=1e-5))
        lls.append(sa.get_likelihood(sample, pred, extract_pts_feature=False).float())
    pred, energy, ll = torch.cat(preds, 0), torch.cat(energies, 0), torch.cat(lls, 0)
    keys = ["5deg2cm", "5deg5cm", "10deg2cm", "10deg5cm"]
    deg, sh, iou = [5, 10], [2, 5, 10], [0.1]
    def score(rt):  # rt [NI,4,4]: one aggregated pose per instance
        rt = rt.double().cpu().numpy()[:, None]
        ia, pa, _, _ = evaluation.compute_mAP(tr._map_results(d, rt, np.zeros((NI, 1, 2))), None, deg, sh, iou, iou_pose_thres=0.1, use_matches_for_pose=True,
                                              repeat_num=1, pooling_mode="average", ratio=1.0, ranker="energy_ranker")
        return evaluation.summary(ia, pa, iou, deg + [360], sh + [100])
    def pooled(en):  # the existing path: K hypotheses, pooling 'average' inside compute_mAP - beside score(avg_RT), to show the two agree
        r = reward.rank_aggregate(pred, en, ratio=RATIO)
        ia, pa, _, _ = evaluation.compute_mAP(tr._map_results(d, rotation.pose9_to_RT(r["sorted_poses"]).cpu().numpy(), r["sorted_energy"].cpu().numpy()), None, deg, sh, iou,
                                              iou_pose_thres=0.1, use_matches_for_pose=True, repeat_num=K, pooling_mode="average", ratio=RATIO, ranker="energy_ranker")
        return evaluation.summary(ia, pa, iou, deg + [360], sh + [100])
    res = {}
    def line(name, r):
        res[name] = r
        say(f"  {name:58s}" + "".join(f"{r[k]:10.2f}" for k in keys))
    rankers = {"energy": energy, "consensus": reward.consensus_energy(pred, sym), "likelihood, RK45 exact": torch.stack([ll, ll], -1).contiguous()}
    say(f"  seed {SEED:<3d} {'':50s}" + "".join(f"{k:>10s}" for k in keys))
    masses = {}
    for name, en in rankers.items():
        r = reward.rank_aggregate(pred, en, selected_num=sel, with_rt=True)
        line(f"{name}: mean", score(r["avg_RT"]))
        m = reward.mode_aggregate(pred, sym, reward.selection_weight(r["order"], sel), with_rt=True)
        line(f"{name}: mode", score(m["mode_RT"]))
        masses[name] = m["mass"].cpu().numpy()
    line("energy: mean, pooled inside compute_mAP (the existing path)", pooled(energy))
    allm = reward.mode_aggregate(pred, sym, None, with_rt=True)
    line("all candidates (ratio 1): mode", score(allm["mode_RT"]))
    line("all candidates (ratio 1): mean", score(reward.rank_aggregate(pred, energy, selected_num=K, with_rt=True)["avg_RT"]))
    line("all candidates (ratio 1): mode, no symmetry flags", score(reward.mode_aggregate(pred, None, None, with_rt=True)["mode_RT"]))
    line("all candidates: the densest candidate (0 iterations)", score(reward.mode_aggregate(pred, sym, None, iters=0, with_rt=True)["mode_RT"]))
    dens = reward.mode_aggregate(pred, sym)["density"]
    r = reward.rank_aggregate(pred, dens, selected_num=sel, with_rt=True)
    line("density as the ranker: mean of its top 60 %", score(r["avg_RT"]))
    w_e = reward.selection_weight(reward.rank_aggregate(pred, energy, selected_num=sel)["order"], sel)
    for bw_r in (5.0, 10.0, 20.0):
        for bw_t in (0.01, 0.02, 0.04):
            line(f"sweep {bw_r:4.0f} deg {100 * bw_t:.0f} cm: mode of all candidates", score(reward.mode_aggregate(pred, sym, None, bw_r, bw_t, with_rt=True)["mode_RT"]))
            line(f"sweep {bw_r:4.0f} deg {100 * bw_t:.0f} cm: mode of the energy ranker's top 60 %", score(reward.mode_aggregate(pred, sym, w_e, bw_r, bw_t, with_rt=True)["mode_RT"]))
    for name in rankers:
        dd = [res[f"{name}: mode"][k] - res[f"{name}: mean"][k] for k in keys]
        say(f"  {name}: mode minus mean: " + " ".join(f"{x:+.2f}" for x in dd) + f" pt; inside the +-2 pt seed-to-seed spread at every threshold: {all(abs(x) <= 2.0 for x in dd)}")
    dd = [res["all candidates (ratio 1): mode"][k] - res["energy: mean"][k] for k in keys]
    say("  mode of all candidates minus the energy ranker's mean: " + " ".join(f"{x:+.2f}" for x in dd) + f" pt; inside the spread at every threshold: {all(abs(x) <= 2.0 for x in dd)}")
    sw = {n: r for n, r in res.items() if n.startswith("sweep")}
    for k in keys:
        best = max(sw, key=lambda n: sw[n][k])
        say(f"  sweep, best at {k}: {best} {sw[best][k]:.2f} ({sw[best][k] - res['energy: mean'][k]:+.2f} pt against the energy ranker's mean)")
    # the confidence: mass against the error of the aggregated pose
    am = allm["mass"].cpu().numpy()
    rt = allm["mode_RT"].double().cpu().numpy()
    gt = np.tile(np.eye(4), (NI, 1, 1)); gt[:, :3, :3], gt[:, :3, 3] = d["R"], d["t"]
    cls = d["cat"].astype(np.int64) + 1
    ov = np.stack([evaluation.compute_RT_overlaps(cls[i:i + 1], gt[i:i + 1], np.ones(1), cls[i:i + 1], rt[i:i + 1])[0, 0] for i in range(NI)])
    say(f"  mass of the mode over all candidates: rotation median {np.median(am[:, 0]):.3f} [{am[:, 0].min():.3f}, {am[:, 0].max():.3f}], translation median {np.median(am[:, 1]):.3f} "
        f"[{am[:, 1].min():.3f}, {am[:, 1].max():.3f}]; instances with rotation mass < 0.5: {int((am[:, 0] < 0.5).sum())} of {NI}")
    lo, hi = am[:, 0] < np.median(am[:, 0]), am[:, 0] >= np.median(am[:, 0])
    say(f"  rotation error of the mode, median: lower-mass half {np.median(ov[lo, 0]):.2f} deg, upper-mass half {np.median(ov[hi, 0]):.2f} deg; within 5 deg: "
        f"{100 * np.mean(ov[lo, 0] <= 5):.1f} % / {100 * np.mean(ov[hi, 0] <= 5):.1f} %; correlation of mass and -error {np.corrcoef(am[:, 0], -ov[:, 0])[0, 1]:+.3f}")
