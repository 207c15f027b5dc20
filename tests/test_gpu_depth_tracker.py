"""GPU: runner.DepthTracker - mask-free tracking around a FixedStepTracker(init='prior'), on the trained checkpoints (random weights give
poses that point nowhere, so no box finds its object).  Three objects of synth.posed_sequence are splatted into uint16 depth images with the
REAL intrinsics (every cloud point a 3 x 3 pixel patch, nearest wins) over a far background plane; an object's own pixels in frame 0 are
its acquisition mask.  acquire + two track calls equal the pieces called one after the other - the two front ends, the tracker's step,
cloud_extent, the select - bit for bit; an object whose pixels are gone is lost: it keeps its pose, in the DepthTracker and in the
tracker's warm-start slot, its neighbours do not notice, and it is found again when its pixels are back."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SEQ_SEED, N_OBJ, FRAMES = 4, 3, 3  # (sequence 4: the three objects' pixel rectangles lie more than 100 pixels apart, all inside the image)
K_CAND, STEPS, TSEED = 10, 2, 0xD0E5
NAMES = ["obj0", "obj1", "obj2"]
LOST = 2
FAR_MM = 3000


def _agent(mode):
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    a = PoseNet(get_config(posenet_mode=mode, sampler_mode=["ode"]))
    a.load_ckpt(model_dir=os.path.join(HERE, "golden", "trained", f"ckpt_{mode}.pth"), model_path=True, load_model_only=True)
    return a


@functools.lru_cache(maxsize=None)
def _score_agent():
    return _agent("score")


def _tracker():
    from genpose_amd.runner import FixedStepTracker
    return FixedStepTracker(_score_agent(), None, steps=STEPS, repeat_num=K_CAND, ranker="consensus", seed=TSEED, init="prior")


@functools.lru_cache(maxsize=None)
def _frames():
    """-> (depth [F,H,W] uint16, owner [F,H,W] int8: which object a pixel shows, -1 the background)."""
    from genpose_amd import synth
    from genpose_amd.preprocess import REAL_INTRINSICS as KI
    fx, fy, cx, cy = float(KI[0, 0]), float(KI[1, 1]), float(KI[0, 2]), float(KI[1, 2])
    seq = synth.posed_sequence(SEQ_SEED, n_frames=FRAMES, n_obj=N_OBJ)
    H, W = 480, 640
    depth = np.full((FRAMES, H, W), FAR_MM, dtype=np.int64)
    owner = np.full((FRAMES, H, W), -1, dtype=np.int8)
    for f in range(FRAMES):
        splats = []
        for o in range(N_OBJ):
            p = seq["pts"][f, o].astype(np.float64)
            u, v, d = np.rint(fx * p[:, 0] / p[:, 2] + cx).astype(int), np.rint(fy * p[:, 1] / p[:, 2] + cy).astype(int), np.rint(p[:, 2] * 1000).astype(int)
            for du in (-1, 0, 1):
                for dv in (-1, 0, 1):
                    ok = (u + du >= 0) & (u + du < W) & (v + dv >= 0) & (v + dv < H)
                    splats.append((o, (v + dv)[ok], (u + du)[ok], d[ok]))
                    np.minimum.at(depth[f], (splats[-1][1], splats[-1][2]), splats[-1][3])
        for o, vv, uu, d in splats:
            hit = depth[f][vv, uu] == d
            owner[f][vv[hit], uu[hit]] = o
    return depth.astype(np.uint16), owner


def _acquisition():
    depth, owner = _frames()
    masks = np.stack([owner[0] == o for o in range(N_OBJ)], axis=-1)
    rois = []
    for o in range(N_OBJ):
        ys, xs = np.where(masks[:, :, o])
        rois.append([ys.min(), xs.min(), ys.max(), xs.max()])
    return depth[0], masks, np.array(rois, dtype=np.int32)


def _without(depth, owner, o):
    """The frame with object o's pixels (its rectangle and 60 pixels around it, where nothing else is) without a reading."""
    ys, xs = np.where(owner == o)
    out = depth.copy()
    out[max(ys.min() - 60, 0):ys.max() + 61, max(xs.min() - 60, 0):xs.max() + 61] = 0
    return out


KEYS = ("init_x", "pred_pose", "energy", "sorted_RTs", "average_sRT", "points", "count", "valid", "half", "pose")


def _host(d):
    torch.cuda.synchronize()
    return {k: d[k].cpu() for k in KEYS}


@functools.lru_cache(maxsize=None)
def _undisturbed():
    """acquire + two track calls -> (the three host dicts, the tracker's slots after each frame, last_stats and captures after each)."""
    from genpose_amd.runner import DepthTracker
    depth, _ = _frames()
    dt = DepthTracker(_tracker())
    outs, slots, stats = [], [], []
    for f in range(FRAMES):
        out = dt.acquire(*_acquisition(), NAMES) if f == 0 else dt.track(depth[f])
        assert all(out[k].is_cuda for k in KEYS)
        outs.append(_host(out))
        slots.append(dt.tracker.pose_slots(0, N_OBJ).cpu())
        stats.append((dict(dt.tracker.last_stats), dt.tracker.captures))
    return outs, slots, stats


def _same(got, want, tag):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), f"{tag}: {k} differs"


def test_acquire_and_two_tracked_frames_equal_the_pieces_called_one_after_the_other():
    from genpose_amd import reward
    from genpose_amd.preprocess import DepthToClouds
    outs, slots, stats = _undisturbed()
    depth, _ = _frames()
    fe, tr = DepthToClouds(), _tracker()
    d0, masks, rois = _acquisition()
    clouds = fe.device_clouds(d0, masks, rois, TSEED, run=0)
    step = tr.step([(clouds["points"], NAMES, None)])[0]
    half = reward.cloud_extent(clouds["points"], step["average_sRT"], 0, None)
    pose = step["average_sRT"].clone()
    _same(_host({**step, **{k: clouds[k] for k in ("points", "count", "valid")}, "half": half, "pose": pose}), outs[0], "acquire")
    for f in (1, 2):
        clouds = fe.device_clouds_boxes(depth[f], pose, half, TSEED, run=f, inflate=1.15, pad=0.01, min_count=2)
        step = tr.step([(clouds["points"], NAMES, None)])[0]
        pose = torch.where((clouds["valid"] != 0).view(N_OBJ, 1, 1), step["average_sRT"], pose)
        tr.pose_slots(0, N_OBJ).copy_(pose)
        _same(_host({**step, **{k: clouds[k] for k in ("points", "count", "valid")}, "half": half, "pose": pose}), outs[f], f"track {f}")
    # these frames lose nothing, every box holds more pixels than a cloud has rows, and the stored poses are the tracker's own
    for f in range(FRAMES):
        print(f"frame {f}: count {outs[f]['count'].tolist()} valid {outs[f]['valid'].tolist()} half {outs[f]['half'].tolist()}")
        assert outs[f]["valid"].tolist() == [1] * N_OBJ
        assert torch.equal(outs[f]["pose"], outs[f]["average_sRT"]) and torch.equal(slots[f], outs[f]["pose"])
        assert torch.isfinite(outs[f]["pose"]).all() and (outs[f]["half"] > 0).all()
    assert torch.equal(outs[1]["half"], outs[0]["half"]) and torch.equal(outs[2]["half"], outs[0]["half"])  # sizes are fixed at acquisition
    assert not torch.equal(outs[1]["pose"], outs[0]["pose"])


def test_replays_stay_within_the_trackers_bound_and_a_seen_layout_captures_nothing():
    _, _, stats = _undisturbed()
    for st, _ in stats:
        assert st["replays"] <= 3
    assert stats[0][0]["acquired"] == N_OBJ and stats[1][0]["acquired"] == 0 and stats[2][0]["acquired"] == 0
    assert stats[0][1] == stats[1][1] == stats[2][1] == 1  # acquire captured the layout; no track call captured anything


def test_a_lost_object_keeps_its_pose_its_neighbours_do_not_notice_and_it_is_found_again():
    from genpose_amd.runner import DepthTracker
    outs, slots, _ = _undisturbed()
    depth, owner = _frames()
    dt = DepthTracker(_tracker())
    a = _host(dt.acquire(*_acquisition(), NAMES))
    _same(a, outs[0], "acquire")
    b = _host(dt.track(_without(depth[1], owner[1], LOST)))
    slot_b = dt.tracker.pose_slots(0, N_OBJ).cpu()
    others = [o for o in range(N_OBJ) if o != LOST]
    assert b["valid"].tolist() == [int(o != LOST) for o in range(N_OBJ)] and int(b["count"][LOST]) == 0 and (b["points"][LOST] == 0).all()
    assert torch.equal(b["pose"][LOST], a["pose"][LOST]) and torch.equal(slot_b[LOST], slots[0][LOST])  # the frame before, bit for bit
    assert not torch.equal(b["average_sRT"][LOST], a["pose"][LOST])  # (the tracker did produce something for the empty cloud)
    for k in KEYS:
        assert torch.equal(b[k][others], outs[1][k][others]), k
    assert torch.equal(slot_b[others], slots[1][others])
    c = _host(dt.track(depth[2]))
    assert c["valid"].tolist() == [1] * N_OBJ and int(c["count"][LOST]) >= 2  # its pixels are back: the box of the kept pose finds them
    assert torch.equal(c["pose"], c["average_sRT"]) and torch.equal(dt.tracker.pose_slots(0, N_OBJ).cpu(), c["pose"])
    for k in KEYS:
        assert torch.equal(c[k][others], outs[2][k][others]), k
