"""GPU: the consensus ranker (csrc/rank.hip: consensus_energy_kernel, consensus_rank_aggregate_kernel; reward.consensus_energy,
reward.consensus_rank_aggregate) against the float64 restatement of its definition (tests/consensus_reference.py), the fused launch against
the two-launch form bit for bit, graph capture, and the two runners that take ranker='consensus'.

Shapes: (1, 1) the empty sum, (1, 2) the exact tie, (3, 7) a small cloud, (5, 50) fewer candidates than lanes, (2, 64) / (2, 65) the
stride boundary, (2, 130) candidates beyond one pass of the wave.

Bounds.  Values: the device accumulates in float64 what the restatement accumulates in float64 (same order of the sum; asin and sqrt
differ by a few float64 ulp, ~1e-13 relative after K additions), and both round to float32 - values that close round to the same float32
or to neighbours: one float32 ulp.  Order: two scores 1e-5 apart (relative) cannot swap under a float32 rounding (6e-8); adjacent pairs of
the reference's order that lie closer are not compared, pairs that tie exactly in the reference must keep candidate order, and the pairs
not compared may be at most 2 % of all adjacent pairs."""
import functools

import numpy as np
import pytest
import torch

import consensus_reference as cr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (3, 7), (5, 50), (2, 64), (2, 65), (2, 130)]
SYMS = ("none", "mixed", "all")
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def _sym(kind, B):
    return None if kind == "none" else np.array([(b + 1) % 2 if kind == "mixed" else 1 for b in range(B)], dtype=np.int8)


@functools.lru_cache(maxsize=None)
def _clouds(B, K):
    poses, _, _ = cr.make_clouds(1000 * B + K, B, K)
    poses.setflags(write=False)
    return poses


@functools.lru_cache(maxsize=None)
def _ref(B, K, kind):
    s = cr.scores(_clouds(B, K), _sym(kind, B))
    s.setflags(write=False)
    return s


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached clouds are read-only)
    return t if dtype is None else t.to(dtype)


def _ulp_apart(got, want64):
    """float32 ulps between the device's float32 scores and the float64 reference cast to float32 (0 where both are the same value)"""
    want = want64.astype(np.float32)
    a, b = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    d = np.abs(a - b)
    d[got == want] = 0  # (-0.0 and 0.0, -inf and -inf)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    return d


def _check_order(order, s_ref):
    """-> (pairs not compared, all adjacent pairs)"""
    B, K, _ = s_ref.shape
    o_ref = cr.stable_order(s_ref)
    skipped = total = 0
    for b in range(B):
        for c in range(2):
            assert sorted(order[b, :, c].tolist()) == list(range(K)), (b, c)
            rank = np.empty(K, dtype=np.int64)
            rank[order[b, :, c]] = np.arange(K)
            for r in range(K - 1):
                i, j = int(o_ref[b, r, c]), int(o_ref[b, r + 1, c])
                si, sj = s_ref[b, i, c], s_ref[b, j, c]
                total += 1
                if si == sj:
                    assert i < j and rank[i] < rank[j], (b, c, r, i, j)
                elif np.isfinite(sj) and (si - sj) < 1e-5 * max(abs(si), abs(sj)):
                    skipped += 1
                else:
                    assert rank[i] < rank[j], (b, c, r, i, j, si, sj)
    return skipped, total


def _same(a, b, what):
    for k in ("energy", "sorted_poses", "sorted_energy", "order", "avg_pose", "sorted_RTs", "avg_RT"):
        if k not in a or k not in b:
            continue
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{what} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} values differ"


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,K", SHAPES)
def test_values_order_and_the_fused_launch(B, K, dtype):
    from genpose_amd import _lib, reward, rotation
    from genpose_amd._lib import ptr, stream_ptr
    poses = _dev(_clouds(B, K), DTYPES[dtype])
    worst = skipped = total = 0
    for kind in SYMS:
        sym, s_ref = _sym(kind, B), _ref(B, K, kind)
        e = reward.consensus_energy(poses, sym)
        assert e.shape == (B, K, 2) and e.dtype == torch.float32
        worst = max(worst, int(_ulp_apart(e.cpu().numpy(), s_ref).max()))
        for sel in sorted({1, max(1, int(0.6 * K)), K}):
            two = reward.rank_aggregate(poses, e, selected_num=sel, with_rt=True)
            two["energy"] = e
            one = reward.consensus_rank_aggregate(poses, sym, selected_num=sel, with_rt=True)
            _same(one, two, f"{kind} sel {sel}")
            assert torch.equal(one["sorted_RTs"], rotation.pose9_to_RT(one["sorted_poses"]))
            assert torch.equal(one["avg_RT"], rotation.quat_trans_to_RT(one["avg_pose"]))
            assert torch.isfinite(one["avg_pose"]).all()
            # the same launch without the energy output
            bare = {k: torch.full_like(v, -7) for k, v in one.items() if k != "energy"}
            symd = reward._sym_arg(sym, B, poses.device)
            _lib.call("gp_consensus_rank_aggregate_rt", B, K, sel, int(dtype == "f64"), ptr(poses), ptr(symd), None, ptr(bare["sorted_poses"]),
                      ptr(bare["sorted_energy"]), ptr(bare["order"]), ptr(bare["avg_pose"]), ptr(bare["sorted_RTs"]), ptr(bare["avg_RT"]), stream_ptr())
            _same(bare, two, f"{kind} sel {sel} without energy_out")
        rk = reward.consensus_rank_aggregate(poses, sym)  # ranking only, no 4x4 forms
        assert rk["avg_pose"] is None and torch.equal(rk["order"], one["order"]) and torch.equal(rk["energy"], e)
        sk, tot = _check_order(one["order"].cpu().numpy(), s_ref)
        skipped, total = skipped + sk, total + tot
    print(f"({B}, {K}) {dtype}: worst float32 ulp distance {worst}; adjacent pairs closer than 1e-5: {skipped} of {total}")
    assert worst <= 1
    assert skipped <= 0.02 * total
    if K == 1:
        assert (e.cpu().numpy() == 0).all()
    if K == 2:
        en = e.cpu().numpy()
        assert (en[:, 0] == en[:, 1]).all() and (one["order"].cpu().numpy()[:, :, 0] == [0, 1]).all()  # the exact tie keeps candidate order


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_duplicates_tie_and_keep_candidate_order(dtype):
    from genpose_amd import reward
    p = _clouds(3, 7).copy()
    p[0, 5] = p[0, 2]
    p[2, 6] = p[2, 0]
    for kind in SYMS:
        r = reward.consensus_rank_aggregate(_dev(p, DTYPES[dtype]), _sym(kind, 3), ratio=0.6)
        e, order = r["energy"].cpu().numpy(), r["order"].cpu().numpy()
        for b, lo, hi in ((0, 2, 5), (2, 0, 6)):
            assert (e[b, lo] == e[b, hi]).all()
            for c in range(2):
                o = order[b, :, c].tolist()
                assert o.index(hi) == o.index(lo) + 1, (kind, b, c, o)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_non_finite_candidates(dtype):
    """Cloud A has one NaN candidate, cloud B is A without it: A's finite candidates score as B's bit for bit, the NaN one ranks last in
    both columns and the aggregate stays finite; a cloud of only non-finite candidates scores -inf throughout, in candidate order."""
    from genpose_amd import reward
    base = _clouds(3, 7)[:1].copy()
    for bad, col, val in ((3, 4, np.nan), (0, 8, np.inf), (6, 0, -np.inf)):
        a = base.copy()
        a[0, bad, col] = val
        b = np.delete(base, bad, axis=1)
        for kind in ("none", "all"):
            sym = _sym(kind, 1)
            ra = reward.consensus_rank_aggregate(_dev(a, DTYPES[dtype]), sym, selected_num=4, with_rt=True)
            eb = reward.consensus_energy(_dev(b, DTYPES[dtype]), sym).cpu().numpy()
            ea, order = ra["energy"].cpu().numpy(), ra["order"].cpu().numpy()
            assert np.array_equal(np.delete(ea, bad, axis=1).view(np.int32), eb.view(np.int32))
            assert np.isneginf(ea[0, bad]).all() and (order[0, -1] == bad).all()
            assert torch.isfinite(ra["avg_pose"]).all() and torch.isfinite(ra["avg_RT"]).all()
            assert int(_ulp_apart(ea, cr.scores(a, sym)).max()) <= 1
    dead = _clouds(3, 7).copy()
    dead[1, :, 2] = np.nan
    r = reward.consensus_rank_aggregate(_dev(dead, DTYPES[dtype]), None)
    e, order = r["energy"].cpu().numpy(), r["order"].cpu().numpy()
    assert np.isneginf(e[1]).all() and (order[1] == np.arange(7)[:, None]).all()
    assert np.isfinite(e[[0, 2]]).all() and np.array_equal(e[[0, 2]], reward.consensus_energy(_dev(_clouds(3, 7)[[0, 2]], DTYPES[dtype])).cpu().numpy())


def test_a_captured_launch_replays_on_new_inputs():
    from genpose_amd import reward
    B, K, sel = 5, 50, 30
    first, second = _dev(_clouds(5, 50)), _dev(cr.make_clouds(77, B, K)[0])
    sym_a, sym_b = _dev(np.array([1, 0, 0, 1, 0], dtype=np.int8)), _dev(np.array([0, 1, 1, 1, 0], dtype=np.int8))
    poses, sym = first.clone(), sym_a.clone()
    reward.consensus_rank_aggregate(poses, sym, selected_num=sel, with_rt=True)
    reward.consensus_energy(poses, sym)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = reward.consensus_rank_aggregate(poses, sym, selected_num=sel, with_rt=True)
        e2 = reward.consensus_energy(poses, sym)
    poses.copy_(second)
    sym.copy_(sym_b)
    g.replay()
    torch.cuda.synchronize()
    want = reward.consensus_rank_aggregate(second, sym_b, selected_num=sel, with_rt=True)
    _same(out, want, "replay")
    assert torch.equal(e2, want["energy"])
    assert not torch.equal(want["energy"], reward.consensus_energy(first, sym_a))


# ------------------------------------------------------------------------------------------------ the runners
KR, STEPS, T0, TSEED = 10, 2, 0.15, 4321


@functools.lru_cache(maxsize=None)
def _score_agent():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from oracle import genpose_oracle as go
    sa = PoseNet(get_config(posenet_mode="score", sampler_mode=["heun"], sampling_steps=STEPS))
    sa.load_state_dict(go.make_state_dict(0, "score"))
    return sa


def test_single_frame_runner_ranks_by_consensus():
    from genpose_amd import reward, rotation, synth
    from genpose_amd.runner import SingleFrameRunner
    run = SingleFrameRunner(_score_agent(), ranker="consensus", repeat_num=KR, batch_size=2)  # 3 clouds: two batches
    assert run.energy_agent is None
    clouds = torch.from_numpy(synth.make_batch(3, start=40)).float().cuda()
    for sym in (None, np.array([1, 0, 1])):
        torch.manual_seed(5)
        out = run.infer_tensors(clouds) if sym is None else run.infer_tensors(clouds, sym=sym)
        pred = out["pred_pose"]
        assert pred.shape == (3, KR, 9) and out["energy"].shape == (3, KR, 2) and out["energy"].dtype == torch.float32
        assert torch.equal(out["energy"], reward.consensus_energy(pred, sym))
        r = reward.rank_aggregate(pred, out["energy"], ratio=run.ratio)
        assert torch.equal(out["sorted_RTs"], rotation.pose9_to_RT(r["sorted_poses"]))
        assert torch.equal(out["average_sRT"], rotation.quat_trans_to_RT(r["avg_pose"].double()))
        assert torch.equal(out["multi_hypothesis_pred_RTs"], rotation.pose9_to_RT(pred))
    with pytest.raises(ValueError, match="sym"):
        run.infer_tensors(clouds, sym=[1, 0])
    assert set(run.infer(clouds.cpu().numpy(), sym=[0, 1, 0])) >= {"pred_pose", "energy", "sorted_RTs", "average_sRT"}


_SYMMETRIC = lambda name: name in ("bottle", "bowl", "can")
_NAMES = [["mug", "can"], ["mug", "can"], ["bowl", "mug"]]  # frame 3: a new object first, the mug continues from slot 0; the flags change


@functools.lru_cache(maxsize=None)
def _sequence(seq):
    from genpose_amd import synth
    from test_gpu_fixed_step_tracker import _poses
    frames = []
    for f, nm in enumerate(_NAMES):
        pts = torch.from_numpy(synth.make_batch(2, start=500 * seq + 23 * f)).float().cuda() + 0.002 * f
        frames.append((pts, nm, _poses(2, 80 + 10 * seq + f)))
    return frames


def _tracker(**kw):
    from genpose_amd.runner import FixedStepTracker
    return FixedStepTracker(_score_agent(), steps=STEPS, repeat_num=KR, T0=T0, ranker="consensus", seed=TSEED, symmetric=_SYMMETRIC, **kw)


def _pieces(tr, seq, frames):
    """The frames through the pieces called one after the other: extract_pts_feature, the host warm-start formula on the dumped draws,
    HeunSampler as a chain, consensus_energy, rank_aggregate."""
    from genpose_amd import reward
    from genpose_amd.runner import add_noise_to_RT, make_batch_sample
    from genpose_amd.samplers import HeunSampler, heun_schedule, track_prior_fill
    from test_gpu_fixed_step_tracker import _host_warm_start
    net = _score_agent().net
    sel = max(1, int(tr.ratio * KR))
    sigma = torch.tensor([heun_schedule(STEPS, T0, net.sampling_eps, "geometric")[1][0, 0]])
    names_prev, prev, outs = [], None, []
    for f, (pts, names, gt) in enumerate(frames):
        n = pts.shape[0]
        sample = make_batch_sample(pts)
        sample["pts_feat"] = net.extract_pts_feature(sample)
        centre = sample["pts_center"]
        g = torch.Generator().manual_seed((TSEED * 1000003 + seq * 7919 + f) % (1 << 63))
        draws = [torch.randn(n, generator=g), torch.randn(n, 4, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)]
        fallback = add_noise_to_RT(gt.float(), draws=draws)
        src = torch.tensor([names_prev.index(nm) if nm in names_prev else -1 for nm in names], dtype=torch.int32)
        z = track_prior_fill(TSEED, f, n * KR, "cuda", row_base=seq * tr.max_objects * KR)
        x0 = _host_warm_start(prev.cpu() if prev is not None else torch.zeros(1, 4, 4), src, fallback, centre.cpu(), sigma, z.cpu(), KR)
        init_sRT = fallback.clone()
        for i, s in enumerate(src.tolist()):
            if s >= 0:
                init_sRT[i] = prev[s].cpu()
        init_x = torch.cat([init_sRT[:, :3, 0], init_sRT[:, :3, 1], init_sRT[:, :3, 3] - centre.cpu()], dim=1).cuda()
        smp = HeunSampler(net.pose_score_net, n, KR, STEPS, "cuda")
        _, pose = smp.run(net.pose_score_net.cloud_embed(sample["pts_feat"].float()), centre.float(), x0.cuda(), T0=T0, eps=net.sampling_eps)
        pred = pose.clone().view(n, KR, 9)
        energy = reward.consensus_energy(pred, [int(_SYMMETRIC(nm)) for nm in names])
        r = reward.rank_aggregate(pred, energy, selected_num=sel, with_rt=True)
        prev, names_prev = r["avg_RT"].clone(), list(names)
        outs.append({"init_x": init_x, "pred_pose": pred, "energy": energy.clone(), "sorted_RTs": r["sorted_RTs"].clone(), "average_sRT": prev.clone(),
                     "nfev": 2 * STEPS + 1})
    return outs


def test_fixed_step_tracker_frames_equal_the_pieces():
    from test_gpu_fixed_step_tracker import _same as same_frame
    tr = _tracker()
    assert tr.energy_agent is None
    want = _pieces(tr, 0, _sequence(0))
    for f, frame in enumerate(_sequence(0)):
        got = tr.step([frame])[0]
        same_frame(got, want[f], f"frame {f}")
        assert tr.last_stats["replays"] <= 2 and tr.last_stats["nfev"] == 2 * STEPS + 1
    assert tr.captures == 1
    # the flags reach the kernel: without them the symmetric objects' rotation column is another array, the translation column is not
    plain = _tracker()
    plain.symmetric = None
    first = plain.step([_sequence(0)[0]])[0]
    assert torch.equal(first["pred_pose"], want[0]["pred_pose"]) and torch.equal(first["energy"][..., 1], want[0]["energy"][..., 1])
    assert torch.equal(first["energy"][0], want[0]["energy"][0]) and not torch.equal(first["energy"][1, :, 0], want[0]["energy"][1, :, 0])


def test_fixed_step_tracker_sequences_together_and_reset():
    from test_gpu_fixed_step_tracker import _same as same_frame
    a, b = _sequence(0), _sequence(1)
    both = _tracker()
    got = [both.step([a[0], b[0]]), both.step([a[1], None]), both.step([a[2], b[1]])]
    assert got[1][1] is None and both.last_stats["replays"] <= 2
    alone_a, alone_b = _tracker(), _tracker()
    for f in range(3):
        same_frame(got[f][0], alone_a.step([a[f], None])[0], f"sequence 0 frame {f}")
    same_frame(got[0][1], alone_b.step([None, b[0]])[1], "sequence 1 frame 0")
    same_frame(got[2][1], alone_b.step([None, b[1]])[1], "sequence 1 frame 1")
    assert not torch.equal(got[0][0]["pred_pose"], got[0][1]["pred_pose"])
    # reset: the jittered starts are back
    tr = _tracker()
    first = tr.step([a[0]])[0]
    second = tr.step([a[0]])[0]
    assert not torch.equal(second["init_x"], first["init_x"])
    tr.reset()
    again = tr.step([a[0]])[0]
    same_frame(again, first, "after reset")
