"""GPU: the depth front end on the device - gp_roi_sample_seeded (csrc/preprocess.hip), preprocess.DepthToClouds.device_clouds and
SingleFrameRunner.infer_depth.  The kernel's rows are, bit for bit, the rows of gp_roi_to_cloud's full cloud that preprocess.seeded_ranks
names (the numpy definition of the draw, held to an independent restatement by tests/test_depth_front_end_cpu.py); a detection's rows do
not depend on what shares its launch; the launch is capturable; the single-frame runner's depth entry point equals its cloud entry point
fed the front end's clouds, and a detection without a usable cloud is carried as a device flag and gets the identity pose."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0xFEED5EED12345678  # (bit 63 set: the whole 64 bits travel)
RUN = 7
CROPS = (8, 13, 100, 256, 257)
N_PTS = (64, 1024)


@functools.lru_cache(maxsize=None)
def _frame():
    from genpose_amd import synth
    return synth.golden_depth_frame(5)


@functools.lru_cache(maxsize=None)
def _full(crop):
    """The parent path's full clouds of the frame at a crop size: (pcl [n, crop^2, 3], count [n], depth_count [n]) on the host."""
    from genpose_amd.preprocess import DepthToClouds
    depth, masks, rois, _ = _frame()
    pcl, cnt, dcnt = DepthToClouds(img_size=crop).full_clouds(depth, masks, rois)
    torch.cuda.synchronize()
    return pcl.cpu(), cnt.cpu().numpy(), dcnt.cpu().numpy()


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _check_against_full(got, pcl, cnt, dcnt, n_pts, seed, run, slot_base):
    from genpose_amd.preprocess import seeded_ranks
    n = len(cnt)
    assert got["points"].shape == (n, n_pts, 3) and got["points"].dtype == torch.float32
    assert got["count"].dtype == torch.int32 and got["depth_count"].dtype == torch.int32 and got["valid"].dtype == torch.uint8
    np.testing.assert_array_equal(got["count"].numpy(), cnt)
    np.testing.assert_array_equal(got["depth_count"].numpy(), dcnt)
    np.testing.assert_array_equal(got["valid"].numpy(), ((cnt > 1) & (dcnt > 1)).astype(np.uint8))
    for i in range(n):
        if cnt[i] > 1 and dcnt[i] > 1:
            ranks = seeded_ranks(int(cnt[i]), n_pts, seed, run, slot_base + i)
            want = pcl[i, torch.from_numpy(ranks)]
            assert torch.equal(got["points"][i], want), f"detection {i}: {int((got['points'][i] != want).any(dim=1).sum())} of {n_pts} rows differ"
        else:
            assert (got["points"][i] == 0).all(), f"detection {i} (count {cnt[i]}, depth_count {dcnt[i]}): rows not zero"


@pytest.mark.parametrize("n_pts", N_PTS)
@pytest.mark.parametrize("crop", CROPS)
def test_rows_are_the_full_clouds_rows_at_the_seeded_ranks(crop, n_pts):
    from genpose_amd.preprocess import DepthToClouds
    depth, masks, rois, _ = _frame()
    pcl, cnt, dcnt = _full(crop)
    fe = DepthToClouds(img_size=crop, n_pts=n_pts)
    got = fe.device_clouds(depth, masks, rois, SEED, RUN, slot_base=3)
    assert all(v.is_cuda for v in got.values())
    _check_against_full(_host(got), pcl, cnt, dcnt, n_pts, SEED, RUN, 3)
    # the frame's skipped detections: the empty mask and the depth hole
    valid = got["valid"].cpu().numpy()
    assert valid[4] == 0 and valid[5] == 0 and cnt[4] == 0 and cnt[5] == 0 and dcnt[4] > 1
    # the same call twice: the same bits; with `out` of the first call: its tensors, written in place
    again = fe.device_clouds(depth, masks, rois, SEED, RUN, slot_base=3, out=got)
    assert all(again[k] is got[k] for k in got)
    _check_against_full(_host(again), pcl, cnt, dcnt, n_pts, SEED, RUN, 3)


def test_every_branch_of_the_draw_is_hit():
    """Crop 8: tiling (1 < c < n) for both cloud sizes; crops 256 / 257: the walk (c > n) for both; c == n: the hand-made mask below."""
    for crop, branch in ((8, "tile"), (256, "walk"), (257, "walk")):
        _, cnt, dcnt = _full(crop)
        ok = (cnt > 1) & (dcnt > 1)
        for n_pts in N_PTS:
            hit = ok & (cnt < n_pts) if branch == "tile" else ok & (cnt > n_pts)
            assert hit.any(), (crop, n_pts, branch, cnt.tolist())
    assert (_full(257)[1] != _full(256)[1]).any()  # (five segments a row instead of four: another table, other counts)


def test_full_mask_of_an_8x8_crop_is_copied_in_raster_order():
    """c == n: 64 valid pixels, 64 output rows -> rank k for row k."""
    from genpose_amd.preprocess import DepthToClouds
    depth = (500 + np.arange(64 * 64).reshape(64, 64) % 97).astype(np.uint16)
    masks = np.ones((64, 64, 1), dtype=bool)
    rois = np.array([[10, 10, 40, 40]], dtype=np.int32)
    fe = DepthToClouds(img_size=8, n_pts=64)
    pcl, cnt, _ = fe.full_clouds(depth, masks, rois)
    got = _host(fe.device_clouds(depth, masks, rois, SEED, RUN))
    assert int(cnt[0]) == 64 and int(got["count"][0]) == 64 and int(got["valid"][0]) == 1
    assert torch.equal(got["points"][0], pcl[0].cpu())


@pytest.mark.parametrize("crop,n_pts", [(256, 1024), (13, 64)])
def test_a_detection_alone_equals_its_row_of_the_frame_and_the_run_moves_the_walk(crop, n_pts):
    from genpose_amd.preprocess import DepthToClouds
    depth, masks, rois, _ = _frame()
    fe = DepthToClouds(img_size=crop, n_pts=n_pts)
    whole = _host(fe.device_clouds(depth, masks, rois, SEED, RUN))
    other = _host(fe.device_clouds(depth, masks, rois, SEED, RUN + 1))
    seeded = _host(fe.device_clouds(depth, masks, rois, SEED + 1, RUN))
    walked = 0
    for i in range(len(rois)):
        alone = _host(fe.device_clouds(depth, masks[:, :, i:i + 1], rois[i:i + 1], SEED, RUN, slot_base=i))
        for k in whole:
            assert torch.equal(alone[k][0], whole[k][i]), (i, k)
        if int(whole["count"][i]) > n_pts:
            walked += 1
            assert not torch.equal(other["points"][i], whole["points"][i]) and not torch.equal(seeded["points"][i], whole["points"][i])
        else:  # tiling and the skipped detections: no draw, nothing moves
            assert torch.equal(other["points"][i], whole["points"][i])
    assert walked >= 1


def _second_frame():
    """Another frame of the same size and detection count: other depth, the detections in reverse order."""
    from genpose_amd import synth
    depth, masks, rois, _ = synth.golden_depth_frame(9)
    return (depth + np.uint16(37) * (depth > 0)).astype(np.uint16), np.ascontiguousarray(masks[:, :, ::-1]), np.ascontiguousarray(rois[::-1])


def _device_inputs(fe, depth, masks, rois, seed, run, slot_base):
    from genpose_amd.preprocess import get_bbox, inverse_crop_map
    H, W = depth.shape
    minv = np.stack([inverse_crop_map(get_bbox(r, H, W), fe.img, H, W) for r in rois]).reshape(len(rois), 6)
    words = np.array([seed & 0xFFFFFFFF, seed >> 32, run, 0, slot_base, 0, 0, 0], dtype=np.uint32).view(np.int32)
    return (torch.from_numpy(depth.view(np.int16)), torch.from_numpy(masks.astype(np.uint8)), torch.from_numpy(minv), torch.from_numpy(words))


def test_the_launch_is_capturable_and_replays_on_overwritten_buffers():
    """No synchronisation, no allocation, no host read in the launch: captured once on frame 1, replayed after depth, masks, minv and the
    seed state were overwritten with frame 2's, it gives frame 2's eager result."""
    from genpose_amd import graphs
    from genpose_amd.preprocess import DepthToClouds
    fe = DepthToClouds(img_size=100, n_pts=64)
    f1 = _frame()[:3]
    f2 = _second_frame()
    bufs = [t.cuda() for t in _device_inputs(fe, *f1, SEED, RUN, 0)]
    out = fe.empty_outputs(len(f1[2]))
    cap = graphs.capture(lambda: fe.launch_seeded(*bufs, out), warmup=True)
    first = {k: v.clone() for k, v in out.items()}
    want1 = fe.device_clouds(*f1, SEED, RUN)
    for k in want1:
        assert torch.equal(first[k], want1[k]), k
    for b, v in zip(bufs, _device_inputs(fe, *f2, SEED + 5, RUN + 2, 16)):
        b.copy_(v)
    for v in out.values():
        v.fill_(1)
    got = cap.replay()
    want2 = fe.device_clouds(*f2, SEED + 5, RUN + 2, slot_base=16)
    torch.cuda.synchronize()
    for k in want2:
        assert torch.equal(got[k], want2[k]), k
    assert not torch.equal(want2["points"], want1["points"]) and int(want2["valid"].sum()) == 4


def test_einval_writes_nothing_and_zero_detections_is_ok():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.preprocess import DepthToClouds
    L = _lib.lib()
    fe = DepthToClouds(img_size=13, n_pts=16)
    depth, masks, minv, seed = (t.cuda() for t in _device_inputs(fe, *_frame()[:3], SEED, RUN, 0))
    H, W, n = depth.shape[0], depth.shape[1], masks.shape[2]
    out = fe.empty_outputs(n)
    for v in out.values():
        v.fill_(7)
    k = (fe.fx, fe.fy, fe.cx, fe.cy)
    o = (ptr(out["points"]), ptr(out["count"]), ptr(out["depth_count"]), ptr(out["valid"]))
    good = (ptr(depth), ptr(masks), ptr(minv))
    s = stream_ptr()
    assert L.gp_roi_sample_seeded(H, W, n, 13, 0, *good, *k, ptr(seed), *o, s) == -1      # no output rows
    assert L.gp_roi_sample_seeded(H, W, n, 513, 16, *good, *k, ptr(seed), *o, s) == -1    # the ballots would not fit
    assert L.gp_roi_sample_seeded(H, W, n, 0, 16, *good, *k, ptr(seed), *o, s) == -1
    assert L.gp_roi_sample_seeded(H, 40000, n, 13, 16, *good, *k, ptr(seed), *o, s) == -1
    assert L.gp_roi_sample_seeded(H, W, -1, 13, 16, *good, *k, ptr(seed), *o, s) == -1
    assert L.gp_roi_sample_seeded(H, W, n, 13, 16, *good, *k, None, *o, s) == -1
    for j in range(3):
        bad = list(good)
        bad[j] = None
        assert L.gp_roi_sample_seeded(H, W, n, 13, 16, *bad, *k, ptr(seed), *o, s) == -1
    for j in range(4):
        bad = list(o)
        bad[j] = None
        assert L.gp_roi_sample_seeded(H, W, n, 13, 16, *good, *k, ptr(seed), *bad, s) == -1
    assert L.gp_roi_sample_seeded(H, W, 0, 13, 16, *good, *k, ptr(seed), *o, s) == 0
    torch.cuda.synchronize()
    assert all((v == 7).all() for v in out.values())
    empty = fe.device_clouds(_frame()[0], np.zeros((H, W, 0), dtype=bool), np.zeros((0, 4), dtype=np.int32), SEED, RUN)
    assert empty["points"].shape == (0, 16, 3) and empty["valid"].shape == (0,)


# ------------------------------------------------------------------ the single-frame runner
STEPS = 2


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


def test_infer_depth_is_infer_tensors_on_the_front_ends_clouds_with_the_identity_for_skipped_detections():
    from genpose_amd.preprocess import DepthToClouds
    from genpose_amd.runner import SingleFrameRunner
    depth, masks, rois, class_ids = _frame()
    sa, ea = _agents()
    runner = SingleFrameRunner(sa, ea, repeat_num=4, T0=0.55)
    torch.manual_seed(123)
    got = runner.infer_depth(depth, masks, rois, class_ids, seed=SEED, frame=RUN)
    assert all(torch.is_tensor(v) and v.is_cuda for v in got.values())
    points = DepthToClouds().device_clouds(depth, masks, rois, SEED, RUN)["points"]
    torch.manual_seed(123)
    want = runner.infer_tensors(points)
    valid = got["valid"].bool().cpu()
    assert valid.tolist() == [True, True, True, True, False, False]
    assert got["cat_id"].tolist() == [int(c) - 1 for c in class_ids]
    eye = torch.eye(4, dtype=got["average_sRT"].dtype)
    for k, w in want.items():
        g = got[k].cpu()
        assert torch.isfinite(g).all(), k
        assert torch.equal(g[valid], w.cpu()[valid]), k
        if k != "average_sRT":
            assert torch.equal(g, w.cpu()), k  # (only the aggregated pose is replaced)
    for i in (4, 5):
        assert torch.equal(got["average_sRT"][i].cpu(), eye)
    assert (points[4:] == 0).all()
