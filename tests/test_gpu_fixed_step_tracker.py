"""GPU: runner.FixedStepTracker and, first, its prior and warm start on the device (csrc/noise.hip: track_warm_start_kernel, gp_track_warm_start,
gp_track_prior_fill; genpose_amd.samplers.track_warm_start / track_prior_fill).  The warm start equals init + sigma * z computed by fp32
torch from the dumped draws BIT FOR BIT (the kernel rounds the product and the sum separately); the draws' raw words equal the numpy
restatement (tests/track_prior_reference.py) through gp_philox_raw, and the normals match it at the tolerance tests/test_gpu_seeded_noise.py
gives the PC draws.  The tracker: a three-frame sequence equals the pieces called one after the other, bit for bit and for both forms of the
solve; sequences stepped together equal each stepped alone; the likelihood ranker; reset and the caller's copy."""
import functools

import numpy as np
import pytest
import torch

import philox_reference as pr
import track_prior_reference as tp

pytestmark = pytest.mark.gpu

SEED = 0xC0FFEE1234567890  # (bit 63 set: the whole 64 bits travel)


def _state(frame, row_base=0, seed=SEED):
    from genpose_amd.samplers import _seed_state
    return _seed_state(seed, frame, row_base, "cuda")


def _poses(n, seed):
    """n rigid 4x4 poses (a rotation from a QR factorisation, a translation), float32"""
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(n, 3, 3, generator=g).double())
    m = torch.eye(4).repeat(n, 1, 1)
    m[:, :3, :3] = q.float()
    m[:, :3, 3] = torch.randn(n, 3, generator=g) * 0.4
    return m


def _host_warm_start(prev, src, fallback, centre, sigma, z, K):
    """evaluation_tracking.py:302-310 + samplers.py:180 in fp32 torch on the host: the product and the sum are two roundings"""
    init_sRT = fallback.clone()
    for i, s in enumerate(src.tolist()):
        if s >= 0:
            init_sRT[i] = prev[s]
    init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre], dim=1)
    n = centre.shape[0]
    return (init_x.unsqueeze(1) + (sigma * z).view(n, K, 9)).view(n * K, 9)


@pytest.mark.parametrize("n,K,src,row_base", [(1, 1, [-1], 0), (3, 10, [-1, 0, 0], 0), (3, 10, [1, -1, 0], 8 * 10 * 5), (40, 50, None, (1 << 40) + 7)])
def test_warm_start_equals_the_host_formula_bit_for_bit(n, K, src, row_base):
    """One fallback and a duplicate taking the first match (src = [-1, 0, 0]); a non-zero row base; 2 000 rows = eight blocks."""
    from genpose_amd.samplers import track_prior_fill, track_warm_start
    frame = 5
    if src is None:
        src = [(-1 if i % 3 == 0 else (7 * i) % 6) for i in range(n)]
    prev, fallback = _poses(6, 1), _poses(n, 2)
    centre = torch.randn(n, 3, generator=torch.Generator().manual_seed(3)) * 0.3
    sigma = torch.tensor([0.0358731], dtype=torch.float32)  # ~ sigma(0.15)
    srct = torch.tensor(src, dtype=torch.int32)
    x0 = track_warm_start(_state(frame, row_base), sigma.cuda(), prev.cuda(), srct.cuda(), fallback.cuda(), centre.cuda(), K)
    z = track_prior_fill(SEED, frame, n * K, "cuda", row_base=row_base)
    torch.cuda.synchronize()
    assert tuple(x0.shape) == (n * K, 9) and x0.dtype == torch.float32 and torch.isfinite(x0).all()
    want = _host_warm_start(prev, srct, fallback, centre, sigma, z.cpu(), K)
    assert torch.equal(x0.cpu(), want), f"{int((x0.cpu() != want).sum())} words differ, max |diff| {float((x0.cpu() - want).abs().max()):.3e}"
    # the draws are those of the restatement (the tolerance of test_gpu_seeded_noise.py: 4 x the difference measured there)
    from test_gpu_seeded_noise import NORMALS_MAX_ABS_DIFF_MEASURED
    ref = tp.normals(SEED, frame, np.uint64(row_base) + np.arange(n * K, dtype=np.uint64))
    diff = float(np.abs(z.cpu().numpy() - ref).max())
    print(f"prior normals, {n * K} rows: max |device - numpy| = {diff:.3e}")
    assert diff <= 4 * NORMALS_MAX_ABS_DIFF_MEASURED
    # another frame index draws something else; the same one draws the same
    assert not torch.equal(z, track_prior_fill(SEED, frame + 1, n * K, "cuda", row_base=row_base))
    assert torch.equal(z, track_prior_fill(SEED, frame, n * K, "cuda", row_base=row_base))


def test_row_base_and_row0_are_slices_of_a_longer_fill():
    from genpose_amd.samplers import track_prior_fill
    full = track_prior_fill(SEED, 2, 700, "cuda")
    assert torch.equal(track_prior_fill(SEED, 2, 300, "cuda", row_base=400), full[400:])
    assert torch.equal(track_prior_fill(SEED, 2, 300, "cuda", row0=123), full[123:423])
    assert torch.equal(track_prior_fill(SEED, 2, 100, "cuda", row_base=200, row0=50), full[250:350])
    # the global row of (sequence, object, candidate): a sequence stepped alone or in company draws the same prior
    K, cap = 10, 8
    rows = tp.global_rows(3, 5, K, cap)
    assert int(rows[0]) == 3 * cap * K and len(rows) == 5 * K
    long = track_prior_fill(SEED, 2, 4 * cap * K, "cuda")
    assert torch.equal(track_prior_fill(SEED, 2, 5 * K, "cuda", row_base=int(rows[0])), long[int(rows[0]):int(rows[0]) + 5 * K])


def test_raw_words_of_the_priors_counters_and_no_pc_draw_shares_them():
    """The prior's counters through gp_philox_raw equal the published generator, give the uniforms behind the filled normals, and the
    same rows' PC draws (both streams, the last step a seeded sampler can take) are other numbers."""
    from genpose_amd.samplers import pc_noise_fill, philox_raw, track_prior_fill
    frame, rows = 9, np.uint64((1 << 33) + 5) + np.arange(64, dtype=np.uint64)
    ctr, key = tp.counters(SEED, frame, rows)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    got = philox_raw(dev(ctr.reshape(-1, 4)), dev(key.reshape(-1, 2))).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, pr.philox4x32_10(ctr.reshape(-1, 4), key.reshape(-1, 2)))
    assert np.array_equal(got.reshape(64, 12), pr.words(SEED, frame, tp.PRIOR_STEP, tp.PRIOR_STREAM, rows))
    assert (ctr[..., 3] >> 3 == tp.PRIOR_STEP).all() and (ctr[..., 2] == frame).all()
    z = track_prior_fill(SEED, frame, 64, "cuda", row_base=int(rows[0]))
    # gp_pc_noise_fill reaches the reserved step as its last one: stream 0 there IS the prior, every sampler step below it is not
    z1, z2 = pc_noise_fill(SEED, frame, 2, 64, "cuda", row_base=int(rows[0]), step0=tp.PRIOR_STEP - 1)
    assert torch.equal(z1[1], z) and not torch.equal(z2[1], z) and not torch.equal(z1[0], z) and not torch.equal(z2[0], z)


def test_einval_and_zero_rows_write_nothing():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    n, K = 3, 4
    st, sigma = _state(0), torch.ones(1, device="cuda")
    prev, fb, centre = _poses(2, 1).cuda(), _poses(n, 2).cuda(), torch.zeros(n, 3, device="cuda")
    src = torch.zeros(n, dtype=torch.int32, device="cuda")
    x0, z = torch.full((n * K, 9), -777.0, device="cuda"), torch.full((n * K, 9), -777.0, device="cuda")
    good = [n, K, ptr(st), ptr(sigma), ptr(prev), ptr(src), ptr(fb), ptr(centre), ptr(x0)]
    for i, v in [(0, -1), (1, 0), (1, -2)] + [(j, None) for j in range(2, 9)]:
        a = list(good)
        a[i] = v
        assert L.gp_track_warm_start(*a, stream_ptr()) == -1, (i, v)
    assert L.gp_track_warm_start(0, K, *good[2:], stream_ptr()) == 0
    assert L.gp_track_prior_fill(None, 0, 4, ptr(z), stream_ptr()) == -1
    assert L.gp_track_prior_fill(ptr(st), -1, 4, ptr(z), stream_ptr()) == -1
    assert L.gp_track_prior_fill(ptr(st), 0, -4, ptr(z), stream_ptr()) == -1
    assert L.gp_track_prior_fill(ptr(st), 0, 4, None, stream_ptr()) == -1
    assert L.gp_track_prior_fill(ptr(st), 0, 0, ptr(z), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((x0 == -777.0).all()) and bool((z == -777.0).all())


# ------------------------------------------------------------------------------------------------ runner.FixedStepTracker
# 1024-point synthetic clouds, K = 10 candidates, 4 Heun steps
K, STEPS, T0, TSEED = 10, 4, 0.15, 1234


@functools.lru_cache(maxsize=None)
def _agents():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from oracle import genpose_oracle as go
    sa = PoseNet(get_config(posenet_mode="score", sampler_mode=["heun"], sampling_steps=STEPS))
    sa.load_state_dict(go.make_state_dict(0, "score"))
    ea = PoseNet(get_config(posenet_mode="energy"))
    ea.load_state_dict(go.make_state_dict(0, "energy"))
    return sa, ea


@functools.lru_cache(maxsize=None)
def _sequence(seq):
    """Three frames of a sequence: frame 2 drops one object, adds a new one and has two objects of the same name; frame 3 repeats frame 2's
    names (the duplicates then both take the first one's pose); 2 -> 3 -> 3 clouds."""
    from genpose_amd import synth
    names = [["mug", "can"], ["mug", "bowl", "bowl"], ["mug", "bowl", "bowl"]]
    frames = []
    for f, nm in enumerate(names):
        pts = torch.from_numpy(synth.make_batch(len(nm), start=300 * seq + 17 * f)).float().cuda() + 0.002 * f
        frames.append((pts, nm, _poses(len(nm), 50 + 10 * seq + f)))
    return frames


def _tracker(ranker="energy", **kw):
    from genpose_amd.runner import FixedStepTracker
    sa, ea = _agents()
    return FixedStepTracker(sa, ea if ranker == "energy" else None, steps=STEPS, repeat_num=K, T0=T0, ranker=ranker, seed=TSEED, **kw)


def _same(got, want, what):
    for k in ("init_x", "pred_pose", "energy", "sorted_RTs", "average_sRT"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, want[k].dtype)
        assert torch.isfinite(got[k]).all(), (what, k)
        assert torch.equal(got[k], want[k]), f"{what} {k}: {int((got[k] != want[k]).sum())} of {got[k].numel()} words differ"
    assert got["nfev"] == want["nfev"]


def _pieces(tr, seq, frames):
    """The same frames through the pieces called one after the other: extract_pts_feature, the host warm-start formula on the dumped
    draws, HeunSampler as a chain, get_energy, rank_aggregate."""
    from genpose_amd import reward
    from genpose_amd.runner import make_batch_sample
    from genpose_amd.samplers import HeunSampler, heun_schedule, track_prior_fill
    sa, ea = _agents()
    net = sa.net
    sel = max(1, int(tr.ratio * K))
    sigma = torch.tensor([heun_schedule(STEPS, T0, net.sampling_eps, "geometric")[1][0, 0]])
    names_prev, prev, outs = [], None, []
    for f, (pts, names, gt) in enumerate(frames):
        n = pts.shape[0]
        sample = make_batch_sample(pts)
        sample["pts_feat"] = net.extract_pts_feature(sample)
        centre = sample["pts_center"]
        g = torch.Generator().manual_seed((TSEED * 1000003 + seq * 7919 + f) % (1 << 63))
        from genpose_amd.runner import add_noise_to_RT
        draws = [torch.randn(n, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)]
        fallback = add_noise_to_RT(gt.float(), draws=draws)
        src = torch.tensor([names_prev.index(nm) if nm in names_prev else -1 for nm in names], dtype=torch.int32)
        z = track_prior_fill(TSEED, f, n * K, "cuda", row_base=seq * tr.max_objects * K)
        x0 = _host_warm_start(prev.cpu() if prev is not None else torch.zeros(1, 4, 4), src, fallback, centre.cpu(), sigma, z.cpu(), K)
        init_sRT = fallback.clone()  # the caller's init_x is the un-noised start
        for i, s in enumerate(src.tolist()):
            if s >= 0:
                init_sRT[i] = prev[s].cpu()
        init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre.cpu()], dim=1).cuda()
        smp = HeunSampler(net.pose_score_net, n, K, STEPS, "cuda")
        _, pose = smp.run(net.pose_score_net.cloud_embed(sample["pts_feat"].float()), centre.float(), x0.cuda(), T0=T0, eps=net.sampling_eps)
        pred = pose.clone().view(n, K, 9)
        energy = ea.get_energy(data=sample, pose_samples=pred, T=1e-5)
        r = reward.rank_aggregate(pred, energy, selected_num=sel, with_rt=True)
        prev, names_prev = r["avg_RT"].clone(), list(names)
        outs.append({"init_x": init_x, "pred_pose": pred, "energy": energy.clone(), "sorted_RTs": r["sorted_RTs"].clone(), "average_sRT": prev.clone(),
                     "nfev": 2 * STEPS + 1})
    return outs


@functools.lru_cache(maxsize=None)
def _reference(seq):
    return _pieces(_tracker(), seq, _sequence(seq))


@pytest.mark.parametrize("launches", ["single", "chain"])
def test_three_frames_equal_the_pieces_called_one_after_the_other(launches):
    want = _reference(0)
    tr = _tracker(launches=launches)
    caps = []
    for f, frame in enumerate(_sequence(0)):
        got = tr.step([frame])[0]
        _same(got, want[f], f"{launches} frame {f}")
        st = tr.last_stats
        assert st["replays"] <= 3 and st["launches"] == launches and st["nfev"] == 2 * STEPS + 1
        assert st["kernel"] == ("heun_solve_kernel<16>" if launches == "single" else "heun_step_kernel<16>")
        caps.append(tr.captures)
    assert caps == [1, 2, 2]  # 2 -> 3 -> 3 clouds: one recapture, none on the repeated shape
    assert tr.last_stats["uploaded_src"] is True  # frame 3: the duplicates now continue from the first match
    tr.step([_sequence(0)[2]])
    assert tr.captures == 2 and tr.last_stats["uploaded_src"] is False and tr.last_stats["uploaded_fallback"] is False  # steady state
    assert _tracker().SINGLE_MAX_ROWS >= 0 and _tracker().launches is None


def test_sequences_stepped_together_equal_each_stepped_alone():
    """Two sequences sharing every launch, one of which skips a step: each equals the sequence stepped alone in a fresh tracker with the
    same seed, bit for bit."""
    a, b = _sequence(0), _sequence(1)
    both = _tracker(launches="single")
    got = [both.step([a[0], b[0]]), both.step([a[1], None]), both.step([a[2], b[1]])]
    assert got[1][1] is None
    alone_a, alone_b = _tracker(launches="single"), _tracker(launches="single")
    for f in range(3):
        _same(got[f][0], alone_a.step([a[f], None])[0], f"sequence 0 frame {f}")
    _same(got[0][1], alone_b.step([None, b[0]])[1], "sequence 1 frame 0")
    _same(got[2][1], alone_b.step([None, b[1]])[1], "sequence 1 frame 1")
    _same(got[2][0], _reference(0)[2], "sequence 0 frame 2 against the pieces")
    assert not torch.equal(got[0][0]["pred_pose"], got[0][1]["pred_pose"])
    with pytest.raises(ValueError, match="max_objects_per_frame"):
        _tracker(max_objects_per_frame=2).step([a[1]])


def test_likelihood_ranker_needs_no_energy_agent():
    sa, _ = _agents()
    tr = _tracker(ranker="likelihood", launches="single")
    assert tr.energy_agent is None
    pts, names, gt = _sequence(0)[1]
    out = tr.step([(pts, names, gt)])[0]
    assert tr.last_stats["replays"] <= 3
    from genpose_amd.runner import make_batch_sample
    sample = make_batch_sample(pts)
    ll = sa.get_likelihood(sample, out["pred_pose"], solver="heun", steps=STEPS).float()
    assert torch.equal(out["energy"][..., 0], ll) and torch.equal(out["energy"][..., 1], ll)
    # the ranking is the stable descending one
    from genpose_amd import rotation
    order = torch.sort(ll, dim=1, descending=True, stable=True).indices
    ranked = torch.gather(out["pred_pose"], 1, order.unsqueeze(-1).expand(-1, -1, 9))
    assert torch.equal(out["sorted_RTs"], rotation.pose9_to_RT(ranked))


def test_reset_and_the_callers_copy():
    frames = _sequence(0)
    tr = _tracker(launches="chain")
    first = tr.step([frames[0]])[0]
    first["average_sRT"].mul_(100.0)  # the caller's copy: editing it does not move the next frame
    second = tr.step([frames[0]])[0]
    ref = _tracker(launches="chain")
    ref.step([frames[0]])
    _same(second, ref.step([frames[0]])[0], "after the caller's edit")
    assert not torch.equal(second["init_x"], first["init_x"])  # (frame 2 continued from the aggregated poses)
    tr.reset()
    again = tr.step([frames[0]])[0]
    first["average_sRT"].div_(100.0)
    assert torch.equal(again["init_x"], first["init_x"]) and torch.equal(again["pred_pose"], first["pred_pose"])  # the jittered starts are back
