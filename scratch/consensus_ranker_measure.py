"""Measurements of the consensus ranker (reward.consensus_rank_aggregate, csrc/rank.hip; profiles/consensus_ranker.txt), one session per part:
  launch  the fused launch (score + ranking + aggregation + both 4x4 forms) against gp_rank_aggregate_rt alone and against the two-launch
          form, 5 x 50 and 256 x 50 (and K = 512): HIP events around 20 back-to-back raw launches on preallocated buffers (and, beside
          them, the Python wrappers), the arms alternating in one loop, microseconds per launch and host time per call, median [min, max];
  frame   a 30-frame synthetic sequence of 5 moving objects, K = 50, trained checkpoints: FixedStepTracker N = 8 / 16 under the energy,
          likelihood and consensus rankers - host clock around step() + synchronize per frame, the arms alternating frame by frame - and
          the aggregated pose's error against the ground truth per arm, first and last frame;
  proxy   the accuracy proxy on 512 held-out synthetic instances, trained checkpoints, the SAME ODE candidates under the energy,
          likelihood (RK45 exact), consensus and random rankers; GP_RANK_SEED picks the draws.
python scratch/consensus_ranker_measure.py launch|frame|proxy [out file]"""
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
    from genpose_amd import _lib, reward
    from genpose_amd._lib import ptr, stream_ptr
    INNER, WARM, REP = 20, 5, 31
    say(f"HIP events around {INNER} back-to-back launches, {WARM} warm-up + {REP} timed samples, arms alternating, us per launch, median [min, max]; float32 poses "
        "(tests/consensus_reference.make_clouds), sel = 60 %, every output written, no cloud symmetric / all symmetric.  The arms are the C entry points called "
        "through ctypes on PREALLOCATED buffers (no allocation, no Python wrapper between the launches); the last two lines of a block time the Python wrappers "
        "(reward.rank_aggregate / consensus_rank_aggregate: 6 - 8 torch.empty per call), which is what a caller outside a captured graph pays")
    L = _lib.lib()
    for B, K in ((5, 50), (256, 50), (5, 512), (256, 512)):
        poses = torch.from_numpy(cr.make_clouds(B + K, B, K)[0]).cuda()
        sel = max(1, int(0.6 * K))
        alls = torch.ones(B, dtype=torch.int8, device="cuda")
        energy = reward.consensus_energy(poses)
        o = reward.consensus_rank_aggregate(poses, None, selected_num=sel, with_rt=True)
        st = stream_ptr()
        outs = [ptr(o[k]) for k in ("sorted_poses", "sorted_energy", "order", "avg_pose", "sorted_RTs", "avg_RT")]
        rank = lambda: L.gp_rank_aggregate_rt(B, K, sel, 0, ptr(poses), ptr(energy), *outs, st)
        score = lambda: L.gp_consensus_energy(B, K, 0, ptr(poses), None, ptr(o["energy"]), st)
        def two():
            L.gp_consensus_energy(B, K, 0, ptr(poses), None, ptr(o["energy"]), st)
            L.gp_rank_aggregate_rt(B, K, sel, 0, ptr(poses), ptr(o["energy"]), *outs, st)
        arms = {"rank_aggregate_rt alone": rank, "consensus_energy alone": score, "two launches": two,
                "fused": lambda: L.gp_consensus_rank_aggregate_rt(B, K, sel, 0, ptr(poses), None, ptr(o["energy"]), *outs, st),
                "fused, symmetric": lambda: L.gp_consensus_rank_aggregate_rt(B, K, sel, 0, ptr(poses), ptr(alls), ptr(o["energy"]), *outs, st),
                "wrapper: rank_aggregate": lambda: reward.rank_aggregate(poses, energy, selected_num=sel, with_rt=True),
                "wrapper: consensus fused": lambda: reward.consensus_rank_aggregate(poses, None, selected_num=sel, with_rt=True)}
        us, host = {a: [] for a in arms}, {a: [] for a in arms}
        for rep in range(WARM + REP):
            for a, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(INNER): fn()
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                if rep >= WARM:
                    us[a].append(e0.elapsed_time(e1) * 1e3 / INNER)
                    host[a].append((t1 - t0) * 1e6 / INNER)
        say(f"  {B:3d} clouds x {K:3d} candidates")
        for a in arms:
            say(f"    {a:26s} {mmm(us[a])} us   (host time to issue one call: median {statistics.median(host[a]):.1f} us)")
        say(f"    fused minus rank_aggregate_rt alone (medians): {statistics.median(us['fused']) - statistics.median(us['rank_aggregate_rt alone']):.2f} us; "
            f"two launches / fused = {statistics.median(us['two launches']) / statistics.median(us['fused']):.2f}x")

def _sequence(seed, F, n_obj):
    from genpose_amd import synth
    seq = synth.posed_sequence(seed, n_frames=F, n_obj=n_obj)
    gt0 = torch.eye(4).repeat(n_obj, 1, 1)
    gt0[:, :3, :3], gt0[:, :3, 3] = torch.from_numpy(seq["R"][0]).float(), torch.from_numpy(seq["t"][0]).float()
    return seq, gt0, [torch.from_numpy(seq["pts"][f]).float().cuda() for f in range(F)]

def _errors(seq, f, avg):
    sym = np.isin(seq["cat"], SYM_CATS)
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
    symmetric = lambda name: int(seq["cat"][int(name[3:])]) in SYM_CATS
    say(f"categories of the five objects {seq['cat'].tolist()} (symmetric about y: {[symmetric(n) for n in names]})")
    torch.manual_seed(0)
    ea = tr._agent("energy")
    arms = {}
    for N in (8, 16):
        for ranker in ("energy", "likelihood", "consensus", "consensus, no symmetry flags"):
            sa = tr._agent("score", "heun", N)
            rk = ranker.split(",")[0]
            arms[f"N={N:2d} {ranker}"] = FixedStepTracker(sa, ea if rk == "energy" else None, steps=N, repeat_num=K, T0=0.15, ranker=rk, seed=7,
                                                          symmetric=symmetric if ranker == "consensus" else None)
    ms, err = {a: [] for a in arms}, {a: [] for a in arms}
    for f in range(F):
        for a, t in arms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = t.step([(clouds[f], names, gt0)])[0]
            torch.cuda.synchronize()
            if f >= WARM: ms[a].append((time.perf_counter() - t0) * 1e3)
            err[a].append(_errors(seq, f, out["average_sRT"]))
    say(f"one sequence, {F} frames x {n_obj} objects x K = {K}, trained checkpoints; host clock around step() + synchronize, arms alternating per frame, frames {WARM}.. timed; "
        "ms per frame, median [min, max]; errors: median over the objects")
    for a in arms:
        r, t = np.array([e[0] for e in err[a]]), np.array([e[1] for e in err[a]])
        say(f"  {a:36s} {mmm(ms[a])} ms   rotation first frame {np.median(r[0]):.2f} deg, last frame {np.median(r[-1]):.2f} deg, median over frames {np.median(r):.2f}, "
            f"worst frame {np.median(r, axis=1).max():.2f}; translation first {np.median(t[0]):.2f} cm, last {np.median(t[-1]):.2f} cm; {arms[a].last_stats}")
    for N in (8, 16):
        e_med = statistics.median(ms[f"N={N:2d} energy"])
        say(f"  N = {N}: consensus median {statistics.median(ms[f'N={N:2d} consensus']):.3f} ms against energy's median {e_med:.3f} ms (minimum {min(ms[f'N={N:2d} energy']):.3f}): "
            f"below the median: {statistics.median(ms[f'N={N:2d} consensus']) < e_med}; likelihood median {statistics.median(ms[f'N={N:2d} likelihood']):.3f} ms")
    for a in arms:
        say(f"  per frame, median over objects, {a}: rotation deg " + " ".join(f"{np.median(e[0]):.1f}" for e in err[a]))

if PART == "proxy":
    SEED, NI = int(os.environ.get("GP_RANK_SEED", "7")), int(os.environ.get("GP_RANK_INSTANCES", "512"))
    import test_gpu_trained_regime as tr
    from genpose_amd import evaluation, reward, rotation
    from genpose_amd.runner import make_batch_sample
    K, RATIO = 50, 0.6
    say(f"accuracy proxy: trained checkpoints, {NI} held-out synthetic instances (synth 1 000 000 ..) in batches of 256, K = {K} candidates from the ODE sampler at "
        f"T0 = 0.55, torch.manual_seed({SEED}); the same candidates under every ranker; top 60 % averaged")
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
    def proxy(en):
        r = reward.rank_aggregate(pred, en, ratio=RATIO)
        deg, sh, iou = [5, 10], [2, 5, 10], [0.1]
        ia, pa, _, _ = evaluation.compute_mAP(tr._map_results(d, rotation.pose9_to_RT(r["sorted_poses"]).cpu().numpy(), r["sorted_energy"].cpu().numpy()), None, deg, sh, iou,
                                              iou_pose_thres=0.1, use_matches_for_pose=True, repeat_num=K, pooling_mode="average", ratio=RATIO, ranker="energy_ranker")
        return evaluation.summary(ia, pa, iou, deg + [360], sh + [100])
    cons = reward.consensus_energy(pred, sym)
    rr = torch.from_numpy(np.random.default_rng(0).standard_normal((NI, K))).float().cuda()
    rows = {"energy ranker": energy, "likelihood, RK45 exact": torch.stack([ll, ll], -1).contiguous(), "consensus": cons,
            "consensus, no symmetry flags": reward.consensus_energy(pred), "random order": torch.stack([rr, rr], -1).contiguous()}
    say(f"  seed {SEED:<3d} {'':28s}" + "".join(f"{k:>10s}" for k in keys))
    res = {}
    for name, en in rows.items():
        t0 = time.time()
        res[name] = proxy(en)
        say(f"  {name:36s}" + "".join(f"{res[name][k]:10.2f}" for k in keys) + f"   ({time.time() - t0:.0f} s)")
    for other in ("energy ranker", "likelihood, RK45 exact", "random order"):
        dd = [res["consensus"][k] - res[other][k] for k in keys]
        say(f"  consensus minus {other}: " + " ".join(f"{x:+.2f}" for x in dd) + f" pt; inside the +-2 pt seed-to-seed spread at every threshold: {all(abs(x) <= 2.0 for x in dd)}")
    # how the consensus order relates to the others: top-30 overlap, mean over the clouds (two random orders share 0.60)
    def top30(a, b):
        ta, tb = np.argsort(-a, axis=1)[:, :30], np.argsort(-b, axis=1)[:, :30]
        return float(np.mean([len(set(u) & set(v)) / 30.0 for u, v in zip(ta, tb)]))
    c, e, l = cons.cpu().numpy(), energy.cpu().numpy(), ll.cpu().numpy()
    say(f"  top-30 overlap: consensus rotation vs energy rotation {top30(c[..., 0], e[..., 0]):.3f}, consensus translation vs energy translation {top30(c[..., 1], e[..., 1]):.3f}, "
        f"consensus rotation vs likelihood {top30(c[..., 0], l):.3f}, consensus translation vs likelihood {top30(c[..., 1], l):.3f}")
