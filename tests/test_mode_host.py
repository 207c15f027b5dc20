"""CPU (no GPU): the mode-seeking aggregation - gp_mode_aggregate's C ABI (declared, bound, exported, refusing bad arguments before any
launch), its host statement genpose_amd.evaluation.mode_sRT against the independent restatement (tests/mode_reference.py), the property it
exists for (on a 30 + 20 bimodal set the mode sits in the larger cluster where the mean of all candidates belongs to neither), its edge
cases, 'mode' in sort_sRT_by_energy / compute_mAP, and the new ValueErrors."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import consensus_reference as cr
import mode_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_symbol_is_declared_bound_and_exported():
    from genpose_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    m = re.search(r"\bint\s+gp_mode_aggregate\s*\(([^)]*)\)\s*;", hdr)
    assert m, "gp_mode_aggregate is not declared in include/genpose_hip.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    sig = _lib.SIGNATURES["gp_mode_aggregate"]
    assert len(sig) == len(args) == 15
    for decl, ct in zip(args, sig):
        want = "pointer" if "*" in decl or decl.startswith("gp_stream_t") else ("double" if decl.startswith("double") else "int")
        assert want == ("double" if ct is ctypes.c_double else ("int" if ct is ctypes.c_int else "pointer")), (decl, ct)
    assert int(re.search(r"#define\s+GP_MODE_MAX_ITERS\s+(\d+)", hdr).group(1)) == _lib.MODE_MAX_ITERS == 64
    assert _lib.CONSENSUS_MAX_K * 108 <= 64 * 1024  # matrix, translation and flag (100 bytes) and two float32 weights per candidate
    build.build()
    assert hasattr(ctypes.CDLL(_lib.SO_PATH), "gp_mode_aggregate")


def test_bad_arguments_are_refused_without_a_device():
    from genpose_amd import _lib
    f = _lib.lib().gp_mode_aggregate
    cap = _lib.CONSENSUS_MAX_K
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)  # (never dereferenced: every call below returns before a launch)
    # (b, k, is_f64, poses, sym, weight, bw_rot, bw_trans, iters, density, mode_pose, mode_rt, mass, start, stream)
    ok = lambda b=2, k=5, poses=p, hr=0.17, ht=0.02, iters=8: f(b, k, 0, poses, None, None, hr, ht, iters, p, p, p, p, p, None)
    assert ok(k=0) == -1 and ok(k=cap + 1) == -1 and ok(b=-1) == -1
    assert ok(poses=None) == -1
    assert ok(hr=0.0) == -1 and ok(hr=-0.1) == -1 and ok(ht=0.0) == -1 and ok(ht=-1.0) == -1
    assert ok(hr=float("nan")) == -1 and ok(ht=float("inf")) == -1
    assert ok(iters=-1) == -1 and ok(iters=65) == -1
    assert ok(b=0) == 0 and ok(b=0, k=cap, iters=64) == 0 and ok(b=0, iters=0) == 0  # inside the limits: the empty batch launches nothing


def test_reward_wrappers_check_arguments_before_the_device(monkeypatch):
    torch = pytest.importorskip("torch")
    from genpose_amd import _lib, reward

    def no_device():
        raise AssertionError("the device was asked for before the arguments were checked")

    monkeypatch.setattr(_lib, "check_device", no_device)
    z = torch.zeros(2, 5, 9)
    assert (reward.MODE_BW_ROT_DEG, reward.MODE_BW_TRANS, reward.MODE_ITERS) == (10.0, 0.02, 8)
    with pytest.raises(ValueError, match="candidates"):
        reward.mode_aggregate(torch.zeros(2, _lib.CONSENSUS_MAX_K + 1, 9))
    with pytest.raises(ValueError, match=r"\[B,K,9\]"):
        reward.mode_aggregate(torch.zeros(2, 5, 7))
    with pytest.raises(RuntimeError, match="float32 or float64"):
        reward.mode_aggregate(z.half())
    with pytest.raises(ValueError, match="one flag per cloud"):
        reward.mode_aggregate(z, sym=[1, 0, 1])
    with pytest.raises(ValueError, match="one pair per candidate"):
        reward.mode_aggregate(z, weight=torch.ones(2, 5))
    for kw in ({"bw_rot_deg": 0.0}, {"bw_rot_deg": float("nan")}, {"bw_trans": -0.02}, {"bw_trans": float("inf")}):
        with pytest.raises(ValueError, match="bandwidths"):
            reward.mode_aggregate(z, **kw)
    for it in (-1, 65, 2.5):
        with pytest.raises(ValueError, match="iters"):
            reward.mode_aggregate(z, iters=it)
    # selection_weight: the first `sel` ranks of each column, as a 0/1 array
    order = torch.tensor([[[2, 0], [0, 1], [1, 2]]], dtype=torch.int32)
    assert reward.selection_weight(order, 2).tolist() == [[[1.0, 1.0], [0.0, 1.0], [1.0, 0.0]]]
    assert reward.selection_weight(order, 3).eq(1).all()
    for sel in (0, 4):
        with pytest.raises(ValueError, match="sel"):
            reward.selection_weight(order, sel)


def test_single_frame_runner_aggregate_argument():
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.runner import SingleFrameRunner
    sa = PoseNet(get_config(device="cpu", sampler_mode=["heun"], sampling_steps=8))
    assert SingleFrameRunner(sa, ranker="consensus").aggregate == "mean"
    assert SingleFrameRunner(sa, ranker="consensus", aggregate="mode").aggregate == "mode"
    for bad in ("median", None, "Mode"):
        with pytest.raises(ValueError, match="aggregate"):
            SingleFrameRunner(sa, ranker="consensus", aggregate=bad)


# ---------------------------------------------------------------------------------------------- the host statement
def _same_as_reference(poses, sym=None, weight=None, **kw):
    from genpose_amd import evaluation as ev
    want = mr.modes(poses, sym, weight, **kw)
    got, mass, start = ev.mode_sRT(cr.pose9_to_rt(poses), sym, weight=weight, **kw)
    assert got.shape == want["RT"].shape and got.dtype == np.float64
    np.testing.assert_array_equal(start, want["start"])
    np.testing.assert_allclose(got, want["RT"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mass, want["mass"], rtol=0, atol=1e-12)
    return got, mass, start


def test_mode_sRT_equals_the_reference():
    poses, _, _ = cr.make_clouds(21, 5, 23)
    for sym in (None, np.array([0, 1, 0, 1, 1]), np.ones(5, dtype=bool)):
        for iters in (0, 1, 8):
            _same_as_reference(poses, sym, iters=iters)
    _same_as_reference(poses, None, bw_rot_deg=5.0, bw_trans=0.04, iters=3)
    bi = mr.make_bimodal(5, 4, 30, 20)[0]
    _same_as_reference(bi)
    _same_as_reference(bi, np.array([1, 0, 1, 0]))
    # weights (a ranking's top 14 per column, and arbitrary positive ones), a non-finite candidate, a duplicate
    rng = np.random.default_rng(3)
    w = np.zeros((5, 23, 2))
    for b in range(5):
        for c in range(2):
            w[b, rng.permutation(23)[:14], c] = 1.0
    _same_as_reference(poses, np.array([0, 1, 0, 1, 1]), w)
    _same_as_reference(poses, None, w * rng.uniform(0.5, 2.0, w.shape))
    edge = poses.astype(np.float64)
    edge[1, 4] = edge[1, 9]
    edge[2, 7, 3] = np.nan
    edge[3, 2, 8] = np.inf
    _same_as_reference(edge, np.array([0, 1, 0, 1, 1]))
    _same_as_reference(edge, None, w)


def test_bimodal_the_mode_lies_in_the_larger_cluster_and_the_mean_in_neither():
    """30 candidates around pose A, 20 around pose B = A turned 90 deg and shifted 5 cm, at the defaults (10 deg, 2 cm, 8 iterations)."""
    from genpose_amd import evaluation as ev
    n = 8
    poses, (A_R, A_t), _, member = mr.make_bimodal(2025, n, 30, 20)
    sRT = cr.pose9_to_rt(poses)
    mode, mass, start = ev.mode_sRT(sRT)
    avg = ev.average_sRT(sRT)
    for b in range(n):
        inl = member[b] == 0
        centre_R, centre_t = cr.mean_rotation(sRT[b, inl, :3, :3]), sRT[b, inl, :3, 3].mean(axis=0)  # A's cluster as drawn
        e_mode = (cr.angle_deg(mode[b, :3, :3], centre_R), np.linalg.norm(mode[b, :3, 3] - centre_t))
        e_avg = (cr.angle_deg(avg[b, :3, :3], centre_R), np.linalg.norm(avg[b, :3, 3] - centre_t))
        print(f"cloud {b}: mode {e_mode[0]:.2f} deg / {1e3 * e_mode[1]:.1f} mm, mean of all {e_avg[0]:.1f} deg / {1e3 * e_avg[1]:.1f} mm, "
              f"to A itself {cr.angle_deg(mode[b, :3, :3], A_R[b]):.2f} deg, mass {mass[b].round(3).tolist()}")
        assert e_mode[0] < 3.0 and e_mode[1] < 0.01
        assert e_avg[0] > 20.0
        assert (mass[b] > 0.4).all() and (mass[b] < 0.7).all()
        assert inl[start[b]].all()


def test_unimodal_the_mode_agrees_with_the_mean():
    from genpose_amd import evaluation as ev
    poses, _, _ = cr.make_clouds(8, 6, 50, inlier=1.0)  # every candidate within about 5 deg / 1 cm of one pose
    sRT = cr.pose9_to_rt(poses)
    mode, mass, _ = ev.mode_sRT(sRT)
    avg = ev.average_sRT(sRT)
    for b in range(6):
        assert cr.angle_deg(mode[b, :3, :3], avg[b, :3, :3]) < 0.5
        assert np.linalg.norm(mode[b, :3, 3] - avg[b, :3, 3]) < 0.002
    assert (mass > 0.7).all() and (mass <= 1.0).all()


def test_edge_cases_of_the_definition():
    from genpose_amd import evaluation as ev
    poses, _, _ = cr.make_clouds(4, 3, 12, inlier=0.5)
    sRT = cr.pose9_to_rt(poses)
    # iters = 0: the start candidate itself, rotation and translation each from its own start
    for sym in (None, np.array([1, 0, 1])):
        got, _, start = ev.mode_sRT(sRT, sym, iters=0)
        for b in range(3):
            np.testing.assert_array_equal(got[b, :3, :3], sRT[b, start[b, 0], :3, :3])
            np.testing.assert_array_equal(got[b, :3, 3], sRT[b, start[b, 1], :3, 3])
    # all candidates equal: mass exactly 1, start 0, the candidate returned
    same = np.repeat(sRT[:, 5:6], 12, axis=1)
    for sym in (None, np.ones(3)):
        for iters in (0, 8):
            got, mass, start = ev.mode_sRT(same, sym, iters=iters)
            assert (mass == 1.0).all() and (start == 0).all()
            np.testing.assert_allclose(got, same[:, 0], rtol=0, atol=1e-15)
    ref = mr.modes(np.repeat(poses[:, 5:6], 12, axis=1))
    assert (ref["mass"] == 1.0).all() and (ref["start"] == 0).all()
    # a zero weight column: the identity (rotation) / the origin (translation), mass 0, start -1; the other column is not touched
    w = np.ones((3, 12, 2))
    w[1, :, 0] = 0.0
    w[2, :, 1] = 0.0
    got, mass, start = _same_as_reference(poses, None, w)
    np.testing.assert_array_equal(got[1, :3, :3], np.eye(3))
    np.testing.assert_array_equal(got[2, :3, 3], np.zeros(3))
    assert mass[1, 0] == 0 and mass[2, 1] == 0 and start[1, 0] == -1 and start[2, 1] == -1
    assert mass[1, 1] > 0 and mass[2, 0] > 0 and (start[0] >= 0).all()
    plain = ev.mode_sRT(sRT)[0]
    np.testing.assert_array_equal(got[1, :3, 3], plain[1, :3, 3])
    np.testing.assert_array_equal(got[2, :3, :3], plain[2, :3, :3])
    # only non-finite candidates: as no weight at all
    dead = sRT.copy()
    dead[0, :, 0, 0] = np.nan
    got, mass, start = ev.mode_sRT(dead)
    np.testing.assert_array_equal(got[0], np.eye(4))
    assert (mass[0] == 0).all() and (start[0] == -1).all()


def test_mode_sRT_refuses_bad_arguments():
    from genpose_amd import evaluation as ev
    sRT = cr.pose9_to_rt(cr.make_clouds(1, 2, 5)[0])
    assert (ev.MODE_BW_ROT_DEG, ev.MODE_BW_TRANS, ev.MODE_ITERS) == (10.0, 0.02, 8)
    for kw in ({"bw_rot_deg": 0.0}, {"bw_trans": 0.0}, {"bw_rot_deg": float("nan")}, {"bw_trans": float("inf")}, {"iters": -1}, {"iters": 1.5},
               {"weight": np.ones((2, 5))}):
        with pytest.raises(ValueError, match="mode_sRT"):
            ev.mode_sRT(sRT, **kw)
    with pytest.raises(NotImplementedError):
        ev.sort_sRT_by_energy(sRT, np.zeros((2, 5, 2)), None, "energy_ranker", 0.6, "median")


# ---------------------------------------------------------------------------------------------- sort_sRT_by_energy / compute_mAP
def test_sort_sRT_by_energy_mode_is_the_mode_of_the_selection():
    from genpose_amd import evaluation as ev
    poses, _, _ = cr.make_clouds(31, 4, 20, inlier=0.6)
    sRT = cr.pose9_to_rt(poses)
    energy = np.random.default_rng(1).standard_normal((4, 20, 2))
    sym = np.array([0, 1, 1, 0])
    sel_a, avg, se_a = ev.sort_sRT_by_energy(sRT.copy(), energy, None, "energy_ranker", 0.6, "average")
    sel_m, mode, se_m = ev.sort_sRT_by_energy(sRT.copy(), energy, None, "energy_ranker", 0.6, "mode", sym=sym)
    np.testing.assert_array_equal(sel_a, sel_m)
    np.testing.assert_array_equal(se_a, se_m)
    np.testing.assert_array_equal(mode, ev.mode_sRT(sel_m, sym)[0])
    assert mode.shape == avg.shape == (4, 4, 4) and not np.allclose(mode, avg)
    _, cons, _ = ev.sort_sRT_by_energy(sRT.copy(), None, None, "consensus_ranker", 0.6, "mode", sym=sym)
    assert cons.shape == (4, 4, 4) and np.isfinite(cons).all()


def test_compute_mAP_pools_by_the_mode():
    from genpose_amd import evaluation as ev
    from genpose_amd import synth
    results = synth.golden_map_results(77, 12, 10)  # the G10 fixture's inputs
    deg, sh, iou = list(range(0, 46)), [i / 2 for i in range(21)], [i / 100 for i in range(101)]
    seen = []
    orig = ev.sort_sRT_by_energy

    def spy(sRT, energy=None, RT_overlaps=None, ranker="energy_ranker", ratio=1.0, error_mode="average", sym=None):
        seen.append((ranker, error_mode, None if sym is None else np.asarray(sym).copy(), len(sRT)))
        return orig(sRT, energy, RT_overlaps, ranker, ratio, error_mode, sym=sym)

    run = lambda res, **kw: ev.compute_mAP(copy.deepcopy(res), None, deg, sh, iou, iou_pose_thres=0.1, use_matches_for_pose=True, **kw)
    ev.sort_sRT_by_energy = spy
    try:
        for ranker in ("energy_ranker", "consensus_ranker"):
            iou_aps, pose_aps, _, _ = run(results, repeat_num=10, pooling_mode="mode", ratio=0.6, ranker=ranker)
            assert pose_aps.shape == (8, 47, 22) and np.isfinite(pose_aps[1:]).all() and 0 < pose_aps[-1, -1, -1] <= 1
    finally:
        ev.sort_sRT_by_energy = orig
    # the class's symmetry flag reaches the mode under every ranker
    assert seen and all(m == "mode" and s is not None and len(s) == n for _, m, s, n in seen)
    flags = {}
    for i, (_, _, s, n) in enumerate(seen):
        if n:
            flags.setdefault(ev.SYNSET_NAMES[1 + i % 6], set()).update(s.tolist())
    assert all(flags.get(c, {True}) == {True} for c in ("bottle", "bowl", "can"))
    assert all(flags.get(c, {False}) == {False} for c in ("camera", "laptop", "mug"))
    assert any(c in flags for c in ("bottle", "bowl", "can")) and any(c in flags for c in ("camera", "laptop", "mug"))
    # the existing modes and the IoU side are what they were
    avg = run(results, repeat_num=10, ratio=0.6)
    np.testing.assert_array_equal(avg[0], iou_aps)
    # K = 1: the mode of one hypothesis is that hypothesis - the same mAP as its average
    one = copy.deepcopy(results)
    for r in one:
        r["multi_hypothesis_pred_RTs"], r["energy"] = r["multi_hypothesis_pred_RTs"][:, :1], r["energy"][:, :1]
    a, m = run(one, repeat_num=1, pooling_mode="average"), run(one, repeat_num=1, pooling_mode="mode")
    for x, y in zip(a, m):
        np.testing.assert_array_equal(x, y)
    with pytest.raises(NotImplementedError):
        run(results, repeat_num=10, pooling_mode="median")
