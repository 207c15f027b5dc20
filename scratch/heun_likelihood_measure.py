"""Measurements of the fixed-step Heun likelihood solve (samplers.HeunLikelihood; profiles/heun_likelihood.txt), in one session:
  time  solve time at 256 x 50 and 64 x 50, Heun N = 8 / 16 / 32 against the RK45 exact-divergence solve of the same inputs: HIP events around
        cond_ode_likelihood on warmed solvers, the arms alternating in one loop, median [min, max];
  band  the smallest N inside the 2e-3 band of tests/test_gpu_heun_likelihood.py::test_converges_to_the_adaptive_solve (bisection);
  rank  ranking quality on the trained checkpoints: top-30 overlap and rank correlation of the Heun likelihood against the RK45 exact
        likelihood and the energy model, and the accuracy proxy's mAP under each ranker on the same candidates.
python scratch/heun_likelihood_measure.py [all | time | band | rank] [out file]"""
import os, statistics, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np, torch
torch.set_num_threads(16)
import exact_likelihood_ref as er
from oracle import genpose_oracle as go
from genpose_amd.likelihood import cond_ode_likelihood
from genpose_amd.samplers import HeunLikelihood, ODESampler
from genpose_amd.scorenet import ScoreNetHIP
from genpose_amd.weights_synth import make_state_dict

OUT = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
def say(*a):
    line = " ".join(str(x) for x in a); print(line, flush=True)
    if OUT:
        OUT.write(line + "\n"); OUT.flush()
def mmm(v): return f"{statistics.median(v):8.2f} [{min(v):.2f}, {max(v):.2f}]"
def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out

PART = sys.argv[1] if len(sys.argv) > 1 else "all"
say(f"device {torch.cuda.get_device_name(0)}")
net = ScoreNetHIP(make_state_dict(0, "score"), "cuda")

if PART in ("all", "time"):
    say("1. solve time, HIP events around cond_ode_likelihood on warmed solvers, arms alternating in one loop, 2 warm-up + 7 timed repeats, ms, median [min, max]; seeded weights (seed 0), poses unit_axis_poses(t = 1e-5)")
    for B, K in ((256, 50), (64, 50)):
        gen = torch.Generator().manual_seed(2)
        pf = torch.randn(B, 1024, generator=gen).abs().cuda()
        x = er.unit_axis_poses(B * K, 1e-5, gen).cuda()
        cvec = net.cloud_embed(pf)
        arms = {"rk45": ODESampler(net, B, K, "cuda", model="likelihood_exact")}
        for N in (8, 16, 32):
            arms[f"heun{N}"] = HeunLikelihood(net, B, K, "cuda", N)
        ms, nfe, bits = {a: [] for a in arms}, {}, {}
        for rep in range(9):
            for a, s in arms.items():
                st = {}
                t, (_, b) = timed(lambda: cond_ode_likelihood(net, cvec, K, x, None, stats=st, solver=s, divergence="exact"))
                nfe[a], bits[a] = (st["nfev"], st["attempts"]), b
                if rep >= 2: ms[a].append(t)
        for a in arms:
            say(f"  {B:3d} clouds x {K} poses  {a:7s} {mmm(ms[a])} ms   NFE {nfe[a][0]:5d} ({nfe[a][1]} {'attempts' if a == 'rk45' else 'steps'}; kernel {arms[a].kernel_name})"
                + ("" if a == "rk45" else f"   rk45 / this = {statistics.median(ms['rk45']) / statistics.median(ms[a]):.1f}x; per evaluation {statistics.median(ms[a]) * 1e3 / nfe[a][0]:.0f} us"))
        del arms

if PART in ("all", "band"):
    say("3. smallest N inside the 2e-3 band, solve test's inputs (2 clouds x 3 poses, seed-0 weights) against the adaptive float64 solve")
    B, K = 2, 3
    sd = go.make_state_dict(0, "score")
    gen = torch.Generator().manual_seed(5)
    pf = torch.randn(B, 1024, generator=gen).abs()
    x = er.unit_axis_poses(B * K, 1e-5, gen)
    z_ref, bits_ref, att = er.solve_f64(sd, pf.repeat_interleave(K, 0), x)
    cvec = net.cloud_embed(pf.cuda())
    def inside(N, grid="geometric"):
        z, bits = cond_ode_likelihood(net, cvec, K, x.cuda(), None, divergence="exact", solver="heun", steps=N, grid=grid)
        z, bits = z.cpu().numpy(), bits.cpu().numpy()
        ok = np.allclose(bits, bits_ref, rtol=2e-3, atol=2e-3 * np.abs(bits_ref).max()) and np.allclose(z, z_ref, rtol=2e-3, atol=2e-3 * np.abs(z_ref).max())
        return ok, np.abs(bits - bits_ref).max() / np.abs(bits_ref).max(), np.abs(z - z_ref).max() / np.abs(z_ref).max()
    for grid in ("geometric", "edm"):
        for N in (8, 16, 32, 64, 128, 256, 512, 1024):
            ok, eb, ez = inside(N, grid)
            say(f"  {grid} N = {N}: bits err {eb:.3e}  z err {ez:.3e}  inside band {ok}")
        lo, hi = 512, 1024
        assert not inside(lo, grid)[0] and inside(hi, grid)[0]
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if inside(mid, grid)[0]: hi = mid
            else: lo = mid
        say(f"  {grid}: smallest N inside = {hi}: {inside(hi, grid)}; N - 1 = {lo}: {inside(lo, grid)}; neighbours " + ", ".join(f"{n}: {inside(n, grid)[0]}" for n in range(hi - 4, hi + 5)))

if PART in ("all", "rank"):
    SEED, NI = int(os.environ.get("GP_RANK_SEED", "7")), int(os.environ.get("GP_RANK_INSTANCES", "256"))
    say(f"2. ranking quality: trained checkpoints, {NI} held-out synthetic instances (synth 1 000 000 ..) in batches of 256, K = 50 candidates from the ODE "
        f"sampler at T0 = 0.55, torch.manual_seed({SEED})")
    import test_gpu_trained_regime as tr
    from genpose_amd import reward, rotation
    from genpose_amd.runner import make_batch_sample
    K, RATIO = 50, 0.6
    d = tr._posed(NI)
    sa, ea = tr._agent("score"), tr._agent("energy")
    torch.manual_seed(SEED)
    preds, energies, lls = [], [], {}
    for b in range(NI // 256):
        sample = make_batch_sample(torch.from_numpy(d["pts"][256 * b:256 * (b + 1)]).cuda())
        pred = sa.pred_func(data=sample, repeat_num=K, save_path=None, T0=0.55)
        preds.append(pred)
        energies.append(ea.get_energy(data=sample, pose_samples=pred, T=1e-5))
        sa.get_likelihood(sample, pred, extract_pts_feature=False)
        t, v = timed(lambda: sa.get_likelihood(sample, pred, extract_pts_feature=False))
        lls.setdefault("rk45", []).append(v)
        say(f"  batch {b}: rk45 exact likelihood {t:.1f} ms (second call), {sa.net.last_likelihood_stats}")
        for N in (8, 16, 32, 64, 128):
            sa.get_likelihood(sample, pred, extract_pts_feature=False, solver="heun", steps=N)
            t, v = timed(lambda: sa.get_likelihood(sample, pred, extract_pts_feature=False, solver="heun", steps=N))
            lls.setdefault(f"heun{N}", []).append(v)
            say(f"  batch {b}: heun N = {N}: {t:.2f} ms (second call, whole get_likelihood), {sa.net.last_likelihood_stats}")
    pred, energy = torch.cat(preds, 0), torch.cat(energies, 0)
    ll = {k: torch.cat(v, 0) for k, v in lls.items()}
    ll = {k: v.cpu().numpy() for k, v in ll.items()}
    e = energy.cpu().numpy().astype(np.float64)
    def ranks(a): return np.argsort(np.argsort(-a, axis=1), axis=1).astype(np.float64)
    def spearman(a, b):
        ra, rb = ranks(a), ranks(b)
        ra -= ra.mean(1, keepdims=True); rb -= rb.mean(1, keepdims=True)
        return float(np.mean((ra * rb).sum(1) / np.sqrt((ra ** 2).sum(1) * (rb ** 2).sum(1))))
    def top30(a, b):
        ta, tb = np.argsort(-a, axis=1)[:, :30], np.argsort(-b, axis=1)[:, :30]
        return float(np.mean([len(set(u) & set(v)) / 30.0 for u, v in zip(ta, tb)]))
    say(f"  bits of the candidates: rk45 mean {ll['rk45'].mean():.1f}, std within a cloud {ll['rk45'].std(1).mean():.1f}")
    for k in ll:
        if k != "rk45":
            dd = ll[k] - ll["rk45"]
            say(f"  {k:8s} minus rk45 (bits): mean {dd.mean():.1f}, std over all {dd.std():.1f}, std within a cloud {dd.std(1).mean():.2f}")
    say("  top-30 overlap (share of 30, mean over clouds; chance 0.60) / Spearman rank correlation (mean over clouds) of the K = 50 candidates")
    say(f"  {'':10s} {'vs rk45 exact':>18s} {'vs energy (rot)':>18s} {'vs energy (trans)':>18s}")
    for k in ll:
        say(f"  {k:10s} {top30(ll[k], ll['rk45']):8.3f} /{spearman(ll[k], ll['rk45']):7.3f} {top30(ll[k], e[:, :, 0]):9.3f} /{spearman(ll[k], e[:, :, 0]):7.3f} {top30(ll[k], e[:, :, 1]):9.3f} /{spearman(ll[k], e[:, :, 1]):7.3f}")
    say(f"  energy rot vs trans: {top30(e[:, :, 0], e[:, :, 1]):.3f} / {spearman(e[:, :, 0], e[:, :, 1]):.3f}")
    say("  accuracy proxy (evaluation.compute_mAP, mean AP over six categories, %, top 60 % averaged), the same candidates:")
    keys = ["5deg2cm", "5deg5cm", "10deg2cm", "10deg5cm"]
    def proxy(en, ranker):
        r = reward.rank_aggregate(pred, en, ratio=RATIO)
        from genpose_amd import evaluation
        deg, sh, iou = [5, 10], [2, 5, 10], [0.1]
        ia, pa, _, _ = evaluation.compute_mAP(tr._map_results(d, rotation.pose9_to_RT(r["sorted_poses"]).cpu().numpy(), r["sorted_energy"].cpu().numpy()), None, deg, sh, iou,
                                              iou_pose_thres=0.1, use_matches_for_pose=True, repeat_num=K, pooling_mode="average", ratio=RATIO, ranker=ranker)
        return evaluation.summary(ia, pa, iou, deg + [360], sh + [100])
    t0 = time.time()
    s = proxy(energy, "energy_ranker")
    say(f"  {'energy ranker':24s}" + "".join(f"{k}: {s[k]:6.2f}  " for k in keys) + f"({time.time() - t0:.0f} s)")
    for k in ll:
        l32 = torch.from_numpy(ll[k]).float().cuda()
        s = proxy(torch.stack([l32, l32], -1).contiguous(), "likelihood_ranker")
        say(f"  {'likelihood ' + k:24s}" + "".join(f"{kk}: {s[kk]:6.2f}  " for kk in keys))
    rng = np.random.default_rng(0)
    rr = torch.from_numpy(rng.standard_normal((NI, K))).float().cuda()
    s = proxy(torch.stack([rr, rr], -1).contiguous(), "likelihood_ranker")
    say(f"  {'random order':24s}" + "".join(f"{kk}: {s[kk]:6.2f}  " for kk in keys))
