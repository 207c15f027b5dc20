"""GPU: the mode-seeking aggregation (csrc/rank.hip: mode_aggregate_kernel; reward.mode_aggregate, reward.selection_weight,
SingleFrameRunner(aggregate='mode')) against the float64 restatement of its definition (tests/mode_reference.py).

Shapes (b, k): (1, 1) one candidate, (1, 2) the exact tie, (3, 3), (5, 50) fewer candidates than lanes, (2, 63) / (2, 64) / (2, 65) the stride
boundary, (1, 512) the cap; float32 and float64 poses; symmetry flags absent and mixed within the batch; 0 and 8 iterations.

Bounds.  density, mass: both sides sum float64 terms that differ by a few float64 ulp (exp, asin, sqrt; the order of the sums), ~1e-13
relative, and both round to float32: the same float32 or its neighbour - one float32 ulp.  start: exact, where the reference's two highest
float64 densities among the candidates that can start differ by more than 1e-9 relative - asserted on the reference for every cloud; exempt
are only the clouds whose top densities tie EXACTLY by construction (deliberate duplicates; k = 2 with equal weights, where the bitwise
symmetric distance makes both densities the same sum), and those must resolve to the lowest index.  mode_RT: atol 2e-6 against the float64
mode, rotation block and translation alike - the bound G8 holds avg_pose to (a float32 quaternion, 6e-8 per component, through
quaternion_to_matrix); matrices are compared, so the sign of a quaternion with w ~ 0 cannot matter."""
import functools

import numpy as np
import pytest
import torch

import consensus_reference as cr
import mode_reference as mr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (3, 3), (5, 50), (2, 63), (2, 64), (2, 65), (1, 512)]
DTYPES = {"f32": torch.float32, "f64": torch.float64}
OUTS = ("density", "mode_pose", "mode_RT", "mass", "start")


def _sym(kind, B):
    return None if kind == "none" else np.array([(b + 1) % 2 for b in range(B)], dtype=np.int8)


@functools.lru_cache(maxsize=None)
def _clouds(B, K):
    """make_clouds at 70 % inliers for the even (B + K), 50 % for the odd, and one bimodal cloud (60 % / 40 %) in batches of five.  K <= 3
    has inliers only: two inliers and a far outlier are as dense as each other up to the outlier's kernel value (~1e-11), a near tie by
    construction, which the condition on the inputs excludes."""
    poses = cr.make_clouds(3000 * B + K, B, K, inlier=1.0 if K <= 3 else (0.7 if (B + K) % 2 == 0 else 0.5))[0].copy()
    if B == 5:
        poses[3] = mr.make_bimodal(K, 1, K - 2 * K // 5, 2 * K // 5)[0][0]
    poses.setflags(write=False)
    return poses


@functools.lru_cache(maxsize=None)
def _top_weight(B, K):
    """0/1 weights: per cloud and column the first max(1, int(0.6 K)) of a seeded ranking (K = 50: the top 30)"""
    rng = np.random.default_rng(17 * B + K)
    w = np.zeros((B, K, 2), dtype=np.float32)
    for b in range(B):
        for c in range(2):
            w[b, rng.permutation(K)[:max(1, int(0.6 * K))], c] = 1.0
    w.setflags(write=False)
    return w


def _ref(poses, sym, weight, iters, exact_tie=()):
    """The reference, with the condition on the inputs asserted: every cloud's top two densities are 1e-9 apart (or, for the clouds listed
    in exact_tie, exactly equal)."""
    r = mr.modes(poses, sym, weight, iters=iters)
    for b in range(poses.shape[0]):
        gap = mr.top_gap(r["density"][b], None if weight is None else weight[b])
        if b in exact_tie:
            assert (gap == 0).all(), (b, gap)
        else:
            assert (gap > 1e-9).all(), f"cloud {b}: the two highest densities are {gap} apart (relative): choose another seed"
    return r


@functools.lru_cache(maxsize=None)
def _ref_cached(B, K, kind, wkind, iters):
    w = None if wkind == "none" else _top_weight(B, K)
    r = _ref(_clouds(B, K), _sym(kind, B), w, iters, exact_tie=range(B) if K == 2 and w is None else ())
    for v in r.values():
        v.setflags(write=False)
    return r


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()  # (a copy: the cached arrays are read-only)
    return t if dtype is None else t.to(dtype)


def _ulp_apart(got, want64):
    want = want64.astype(np.float32)
    a, b = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    d = np.abs(a - b)
    d[got == want] = 0  # (-0.0 and 0.0, -inf and -inf)
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    return d


def _same(a, b, what):
    for k in OUTS:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), f"{what} {k}: {int((a[k] != b[k]).sum())} of {a[k].numel()} values differ"


def _check(out, ref, what):
    """-> the worst float32 ulp distance of density and mass"""
    from genpose_amd import rotation
    B, K = ref["density"].shape[:2]
    assert out["density"].shape == (B, K, 2) and out["mode_pose"].shape == (B, 7) and out["mode_RT"].shape == (B, 4, 4)
    assert out["mass"].shape == (B, 2) and out["start"].shape == (B, 2) and out["start"].dtype == torch.int32
    assert all(out[k].dtype == torch.float32 for k in OUTS[:4])
    got = {k: out[k].cpu().numpy() for k in OUTS}
    assert np.array_equal(got["start"], ref["start"]), (what, got["start"].tolist(), ref["start"].tolist())
    worst = max(int(_ulp_apart(got["density"], ref["density"]).max()), int(_ulp_apart(got["mass"], ref["mass"]).max()))
    assert worst <= 1, (what, worst)
    assert (got["mass"] >= 0).all() and (got["mass"] <= 1).all()
    err = np.abs(got["mode_RT"].astype(np.float64) - ref["RT"])
    print(f"{what}: density / mass worst float32 ulp distance {worst}; |mode_RT - reference| rotation {err[:, :3, :3].max():.2e}, "
          f"translation {err[:, :3, 3].max():.2e}")
    assert err.max() <= 2e-6, (what, err.max())
    assert np.array_equal(got["mode_pose"][:, 4:], got["mode_RT"][:, :3, 3]) and (got["mode_pose"][:, 0] >= 0).all()
    assert torch.equal(out["mode_RT"], rotation.quat_trans_to_RT(out["mode_pose"]))  # bit for bit gp_quat_trans_to_rt
    return worst


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,K", SHAPES)
def test_against_the_reference(B, K, dtype):
    from genpose_amd import reward
    poses = _dev(_clouds(B, K), DTYPES[dtype])
    for kind in ("none", "mixed"):
        for iters in (0, 8):
            out = reward.mode_aggregate(poses, _sym(kind, B), iters=iters, with_rt=True)
            _check(out, _ref_cached(B, K, kind, "none", iters), f"({B}, {K}) {dtype} sym {kind} iters {iters}")
            if iters == 0:  # the start candidate itself
                start = out["start"].long()
                rows = torch.arange(B, device="cuda")
                assert torch.equal(out["mode_pose"][:, 4:], poses[rows, start[:, 1], 6:9].float())
    if K == 1:
        assert (out["mass"] == 1).all() and (out["density"] == 1).all() and (out["start"] == 0).all()
    if K == 2:  # the exact tie: both candidates as dense, the lower index starts
        d = out["density"].cpu().numpy()
        assert (d[:, 0] == d[:, 1]).all() and (out["start"] == 0).all()
    # a cloud's outputs alone and inside the batch: the same bits
    if B > 1:
        sym = _sym("mixed", B)
        for b in (0, B - 1):
            alone = reward.mode_aggregate(poses[b:b + 1], sym[b:b + 1], with_rt=True)
            _same(alone, {k: out[k][b:b + 1] for k in OUTS}, f"cloud {b} alone")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,K", [(5, 50), (2, 65)])
def test_weights(B, K, dtype):
    """The top 60 % per column (K = 50: the top 30) of a ranking as the weight, then the same with one cloud's weights all zero, then
    arbitrary positive weights; selection_weight makes the 0/1 array from a ranking's order on the device."""
    from genpose_amd import reward
    poses, w = _dev(_clouds(B, K), DTYPES[dtype]), _top_weight(B, K)
    for kind in ("none", "mixed"):
        out = reward.mode_aggregate(poses, _sym(kind, B), _dev(w), with_rt=True)
        _check(out, _ref_cached(B, K, kind, "top", 8), f"({B}, {K}) {dtype} sym {kind} top weights")
        on = torch.gather(_dev(w), 1, out["start"].long()[:, None, :])
        assert (on == 1).all()  # a weighted candidate starts
    sym = _sym("mixed", B)
    wz = w.copy()
    wz[1] = 0.0
    wz[0, :, 1] = 0.0
    wz[0, 3, 0] = -2.0  # (a negative weight counts as none)
    out = reward.mode_aggregate(poses, sym, _dev(wz), with_rt=True)
    ref = _ref(_clouds(B, K), sym, wz, 8)
    _check(out, ref, f"({B}, {K}) {dtype} a cloud without weight")
    got = {k: out[k].cpu().numpy() for k in OUTS}
    assert np.array_equal(got["mode_pose"][1], [1, 0, 0, 0, 0, 0, 0]) and np.array_equal(got["mode_RT"][1], np.eye(4))
    assert (got["mass"][1] == 0).all() and (got["start"][1] == -1).all() and (got["density"][1] == 0).all()
    assert got["mass"][0, 1] == 0 and got["start"][0, 1] == -1 and np.array_equal(got["mode_pose"][0, 4:], [0, 0, 0]) and got["mass"][0, 0] > 0
    rng = np.random.default_rng(5)
    wa = (w * rng.uniform(0.25, 4.0, w.shape)).astype(np.float32)
    _check(reward.mode_aggregate(poses, sym, _dev(wa), with_rt=True), _ref(_clouds(B, K), sym, wa, 8), f"({B}, {K}) {dtype} real weights")
    # selection_weight: a ranking's first 0.6 K per column
    energy = torch.from_numpy(rng.standard_normal((B, K, 2)).astype(np.float32)).cuda()
    sel = max(1, int(0.6 * K))
    order = reward.rank_aggregate(poses, energy, selected_num=sel)["order"]
    ws = reward.selection_weight(order, sel)
    want = np.zeros((B, K, 2), dtype=np.float32)
    o = np.argsort(-energy.cpu().numpy(), axis=1, kind="stable")[:, :sel]
    for b in range(B):
        for c in range(2):
            want[b, o[b, :, c], c] = 1.0
    assert ws.dtype == torch.float32 and np.array_equal(ws.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_non_finite_candidates_and_duplicates(dtype):
    from genpose_amd import reward
    B, K = 5, 50
    base = _clouds(B, K)
    sym = _sym("mixed", B)
    # two non-finite candidates: -inf density, no weight in any sum - the rest is the cloud without them
    p = base.copy()
    p[0, 7, 4] = np.nan
    p[0, 31, 8] = np.inf
    p[2, 0, 0] = -np.inf
    p[2, 49, 6] = np.nan
    out = reward.mode_aggregate(_dev(p, DTYPES[dtype]), sym, with_rt=True)
    _check(out, _ref(p, sym, None, 8), f"{dtype} non-finite candidates")
    d = out["density"].cpu().numpy()
    assert np.isneginf(d[0, [7, 31]]).all() and np.isneginf(d[2, [0, 49]]).all() and np.isfinite(out["mode_RT"].cpu().numpy()).all()
    less = reward.mode_aggregate(_dev(np.delete(p[:1], [7, 31], axis=1), DTYPES[dtype]), sym[:1], with_rt=True)
    assert np.array_equal(np.delete(d[0], [7, 31], axis=0).view(np.int32), less["density"][0].cpu().numpy().view(np.int32))
    # (the centre's sums are lane partials: other candidates per lane, other last bits - the float32 outputs agree to a few ulp)
    for k in ("mode_pose", "mode_RT", "mass"):
        assert torch.allclose(out[k][0], less[k][0], rtol=0, atol=1e-6), k
    dead = base.copy()
    dead[4, :, 1] = np.nan  # a cloud of only non-finite candidates: as no weight at all
    out = reward.mode_aggregate(_dev(dead, DTYPES[dtype]), sym, with_rt=True)
    assert np.isneginf(out["density"][4].cpu().numpy()).all() and (out["start"][4] == -1).all() and (out["mass"][4] == 0).all()
    assert np.array_equal(out["mode_RT"][4].cpu().numpy(), np.eye(4))
    # duplicates: the densest candidate copied to two other places ties with its copies exactly, and the lowest index starts
    first = mr.modes(base, sym, None, iters=8)
    q = base.copy()
    for b in range(B):
        s = int(first["start"][b, 0])
        q[b, (s + 5) % K] = q[b, s]
        q[b, (s + 23) % K] = q[b, s]
    ref = mr.modes(q, sym, None, iters=8)
    out = reward.mode_aggregate(_dev(q, DTYPES[dtype]), sym, with_rt=True)
    d = out["density"].cpu().numpy()
    for b in range(B):
        s = int(first["start"][b, 0])
        trio = sorted([s, (s + 5) % K, (s + 23) % K])
        assert (d[b, trio[0]] == d[b, trio[1]]).all() and (d[b, trio[0]] == d[b, trio[2]]).all()
        gap = mr.top_gap(ref["density"][b])
        assert ref["start"][b, 0] == trio[0] and gap[0] == 0  # the reference's top (rotation) is the tied trio
        assert gap[1] == 0 or gap[1] > 1e-9               # the translation's: the trio again, or a clear winner
    assert np.array_equal(out["start"].cpu().numpy(), ref["start"])
    assert int(_ulp_apart(d, ref["density"]).max()) <= 1 and np.abs(out["mode_RT"].cpu().numpy() - ref["RT"]).max() <= 2e-6
    # a cloud of nothing but copies of one candidate: density and mass exactly 1, start 0, the candidate returned
    same = np.repeat(base[:, 9:10], 12, axis=1)
    for iters in (0, 8):
        out = reward.mode_aggregate(_dev(same, DTYPES[dtype]), sym, iters=iters, with_rt=True)
        assert (out["density"] == 1).all() and (out["mass"] == 1).all() and (out["start"] == 0).all()
        assert np.abs(out["mode_RT"].cpu().numpy() - cr.pose9_to_rt(same[:, 0])).max() <= 2e-6


def test_optional_outputs_and_refused_arguments():
    from genpose_amd import _lib, reward
    from genpose_amd._lib import ptr, stream_ptr
    B, K = 3, 3
    poses = _dev(_clouds(B, K))
    full = reward.mode_aggregate(poses, None, with_rt=True)
    call = lambda b, k, p, hr, ht, iters, o: _lib.lib().gp_mode_aggregate(b, k, 0, ptr(p), None, None, hr, ht, iters, ptr(o["density"]),
                                                                          ptr(o["mode_pose"]), ptr(o["mode_RT"]), ptr(o["mass"]), ptr(o["start"]),
                                                                          stream_ptr())
    h = (float(np.deg2rad(reward.MODE_BW_ROT_DEG)), reward.MODE_BW_TRANS, reward.MODE_ITERS)
    for only in OUTS:  # every output alone: the same bits
        o = {k: (torch.full_like(full[k], -7) if k == only else None) for k in OUTS}
        assert call(B, K, poses, *h, o) == 0
        assert torch.equal(o[only].view(torch.uint8), full[only].view(torch.uint8)), only
    assert reward.mode_aggregate(poses)["mode_RT"] is None
    o = {k: torch.full_like(full[k], -7) for k in OUTS}
    big = torch.zeros(1, 513, 9, device="cuda")
    assert call(1, 513, big, *h, o) == -1
    for hr, ht, it in ((0.0, 0.02, 8), (-0.1, 0.02, 8), (0.17, 0.0, 8), (0.17, -1.0, 8), (float("nan"), 0.02, 8), (0.17, float("inf"), 8),
                       (0.17, 0.02, 65), (0.17, 0.02, -1)):
        assert call(B, K, poses, hr, ht, it, o) == -1
    assert call(B, K, None, *h, o) == -1
    assert call(0, K, poses, *h, o) == 0
    torch.cuda.synchronize()
    assert all((o[k] == -7).all() for k in OUTS)  # nothing was launched


def test_a_captured_launch_replays_on_new_inputs():
    from genpose_amd import reward
    B, K = 5, 50
    first, second = _dev(_clouds(B, K)), _dev(cr.make_clouds(78, B, K, inlier=0.5)[0])
    sym_a, sym_b = _dev(np.array([1, 0, 0, 1, 0], dtype=np.int8)), _dev(np.array([0, 1, 1, 1, 0], dtype=np.int8))
    w_a, w_b = _dev(_top_weight(B, K)), _dev(_top_weight(B, K)[::-1].copy())
    poses, sym, w = first.clone(), sym_a.clone(), w_a.clone()
    reward.mode_aggregate(poses, sym, w, with_rt=True)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = reward.mode_aggregate(poses, sym, w, with_rt=True)
    poses.copy_(second)
    sym.copy_(sym_b)
    w.copy_(w_b)
    g.replay()
    torch.cuda.synchronize()
    want = reward.mode_aggregate(second, sym_b, w_b, with_rt=True)
    _same(out, want, "replay")
    assert not torch.equal(want["mode_pose"], reward.mode_aggregate(first, sym_a, w_a)["mode_pose"])


# ------------------------------------------------------------------------------------------------ the runner
@functools.lru_cache(maxsize=None)
def _energy_agent():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from oracle import genpose_oracle as go
    ea = PoseNet(get_config(posenet_mode="energy"))
    ea.load_state_dict(go.make_state_dict(0, "energy"))
    return ea


@pytest.mark.parametrize("ranker", ["consensus", "energy"])
def test_single_frame_runner_mode_equals_the_pieces_and_mean_is_unchanged(ranker):
    from test_gpu_consensus import KR, _score_agent
    from genpose_amd import reward, rotation, synth
    from genpose_amd.runner import SingleFrameRunner
    ea = _energy_agent() if ranker == "energy" else None
    clouds = torch.from_numpy(synth.make_batch(3, start=40)).float().cuda()
    sym = np.array([1, 0, 1])
    runs = {a: SingleFrameRunner(_score_agent(), ea, ranker=ranker, repeat_num=KR, batch_size=2, aggregate=a) for a in ("mean", "mode")}  # two batches
    out = {}
    for a, run in runs.items():
        torch.manual_seed(5)
        out[a] = run.infer_tensors(clouds, sym=sym) if (a == "mode" or ranker == "consensus") else run.infer_tensors(clouds)
    mean, mode = out["mean"], out["mode"]
    # 'mean': what the runner returned before it had the argument - the ranking's pieces called one after the other
    pred, energy = mean["pred_pose"], mean["energy"]
    if ranker == "consensus":
        assert torch.equal(energy, reward.consensus_energy(pred, sym))
    r = reward.rank_aggregate(pred, energy, ratio=runs["mean"].ratio)
    assert set(mean) == {"pred_pose", "multi_hypothesis_pred_RTs", "energy", "sorted_RTs", "average_sRT"}
    assert torch.equal(mean["sorted_RTs"], rotation.pose9_to_RT(r["sorted_poses"]))
    assert torch.equal(mean["average_sRT"], rotation.quat_trans_to_RT(r["avg_pose"].double()))
    assert torch.equal(mean["multi_hypothesis_pred_RTs"], rotation.pose9_to_RT(pred))
    # 'mode': the same candidates and ranking, then mode_aggregate on the ranking's top max(1, int(K ratio)) per column
    for k in ("pred_pose", "multi_hypothesis_pred_RTs", "energy", "sorted_RTs"):
        assert torch.equal(mode[k], mean[k]), k
    sel = max(1, int(KR * runs["mode"].ratio))
    m = reward.mode_aggregate(pred, sym, reward.selection_weight(r["order"], sel), with_rt=True)
    assert mode["average_sRT"].dtype == torch.float64 and torch.equal(mode["average_sRT"], m["mode_RT"].double())
    assert mode["mode_mass"].shape == (3, 2) and torch.equal(mode["mode_mass"], m["mass"])
    assert (mode["mode_mass"] > 0).all() and (mode["mode_mass"] <= 1).all()
    ref = mr.modes(pred.cpu().numpy(), sym, reward.selection_weight(r["order"], sel).cpu().numpy())
    assert np.abs(mode["average_sRT"].cpu().numpy() - ref["RT"]).max() <= 2e-6
    if ranker == "energy":
        with pytest.raises(ValueError, match="sym"):
            runs["mean"].infer_tensors(clouds, sym=sym)  # still the consensus ranker's argument there
