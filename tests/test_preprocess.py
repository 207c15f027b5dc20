"""Depth + mask -> point cloud pre-processing.
CPU: the oracle (oracle/preprocess_oracle.py, oracle/cv2_restated.py) against fixture G11, which was produced by composing the
reference's own get_bbox / get_2d_coord_np / crop_resize_by_warp_affine (oracle/gen_golden.py --g11); the product's host
arithmetic (window, inverse crop map) against the oracle.  GPU: the HIP path against the oracle, bit for bit."""
import functools
import hashlib

import numpy as np
import pytest

from genpose_amd import preprocess as pp
from genpose_amd import synth
from oracle import cv2_restated as cv2r
from oracle import preprocess_oracle as po


def _sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def test_oracle_matches_reference_fixture(golden):
    g = golden("g11_preprocess.npz")
    depth, masks, rois, class_ids = synth.golden_depth_frame()
    K = g["intrinsics"]
    assert np.array_equal(K, po.REAL_INTRINSICS)
    for i in range(len(class_ids)):
        assert tuple(g[f"i{i}_bbox"]) == po.get_bbox(rois[i])
        cloud = po.instance_cloud(depth, masks[:, :, i], rois[i], K)
        if f"i{i}_cloud_sha" not in g:
            assert cloud is None
            continue
        assert cloud.shape[0] == int(g[f"i{i}_n_valid"]) and cloud.dtype == np.float32
        np.testing.assert_array_equal(cloud[:64], g[f"i{i}_cloud_head"])
        np.testing.assert_array_equal(_sha(cloud), g[f"i{i}_cloud_sha"])
    pts, cat, inst = po.frame_clouds(depth, masks, rois, class_ids, K, rng=np.random.RandomState(11))
    np.testing.assert_array_equal(pts, g["points"])
    assert cat == list(g["cat_id"]) and inst == list(g["valid_inst"])
    assert sorted(set(range(len(class_ids))) - set(inst)) == [4, 5]  # the empty mask and the depth hole are skipped


def test_host_window_and_inverse_map_equal_oracle():
    rng = np.random.default_rng(0)
    for _ in range(300):
        y1, x1 = int(rng.integers(0, 470)), int(rng.integers(0, 630))
        roi = [y1, x1, min(479, y1 + int(rng.integers(1, 470))), min(639, x1 + int(rng.integers(1, 630)))]
        win = pp.get_bbox(roi)
        assert win == po.get_bbox(roi)
        rmin, rmax, cmin, cmax = win
        center = np.array([0.5 * (cmin + cmax), 0.5 * (rmin + rmax)])
        scale = min(max(rmax - rmin, cmax - cmin), 640) * 1.0
        ref_inv = cv2r.invertAffineTransform(po.get_affine_transform(center, scale, 256))
        mine = pp.inverse_crop_map(win, 256, 480, 640)
        np.testing.assert_allclose(mine, ref_inv, rtol=0, atol=1e-9)
        # and the sampled source pixels are identical
        sx, sy = cv2r.nearest_source_index(po.get_affine_transform(center, scale, 256), (256, 256))
        j = np.arange(256)
        np.testing.assert_array_equal(sx[0], np.floor(j * scale / 256 + mine[0, 2] + 0.5).astype(np.int64))
        np.testing.assert_array_equal(sy[:, 0], np.floor(j * scale / 256 + mine[1, 2] + 0.5).astype(np.int64))


def test_warp_nearest_border_and_dtype():
    img = np.arange(20, dtype=np.uint16).reshape(4, 5)
    M = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0]])  # dst = src + (2, -1)
    out = cv2r.warpAffine(img, M, (5, 4), flags=cv2r.INTER_NEAREST)
    assert out.dtype == np.uint16 and out.shape == (4, 5)
    exp = np.zeros((4, 5), dtype=np.uint16)
    exp[0:3, 2:5] = img[1:4, 0:3]
    np.testing.assert_array_equal(out, exp)


def test_sample_points_rules():
    pcl = np.arange(15, dtype=np.float32).reshape(5, 3)
    np.testing.assert_array_equal(po.sample_points(pcl, 12)[:, 0] // 3, np.arange(12) % 5)
    assert po.sample_points(pcl, 5) is pcl
    sub = po.sample_points(pcl, 3, np.random.RandomState(0))
    np.testing.assert_array_equal(sub, pcl[np.random.RandomState(0).permutation(5)[:3]])


@pytest.mark.gpu
def test_hip_clouds_bit_exact_vs_oracle():
    import torch
    for seed in (5, 6):
        depth, masks, rois, class_ids = synth.golden_depth_frame(seed)
        d2c = pp.DepthToClouds(pp.REAL_INTRINSICS)
        pcl, count, dcount = d2c.full_clouds(depth, masks, rois)
        torch.cuda.synchronize()
        for i in range(len(class_ids)):
            ref = po.instance_cloud(depth, masks[:, :, i], rois[i], po.REAL_INTRINSICS)
            c = int(count[i])
            if ref is None:
                assert c <= 1 or int(dcount[i]) <= 1
                continue
            assert c == ref.shape[0]
            np.testing.assert_array_equal(pcl[i, :c].cpu().numpy(), ref)  # float32, bit for bit, same point order
        got = d2c(depth, masks, rois, class_ids, rng=np.random.RandomState(11))
        pts, cat, inst = po.frame_clouds(depth, masks, rois, class_ids, po.REAL_INTRINSICS, rng=np.random.RandomState(11))
        np.testing.assert_array_equal(got["points"].cpu().numpy(), pts)
        assert got["cat_id"] == cat and got["valid_inst"] == inst


# Crop sizes beside the runners' 256.  The kernel gives each of its 16 waves ceil(img / 16) crop rows and walks a row 64 columns at a time:
# 8 has fewer rows than waves (eight waves own nothing); 13 and 100 leave the last wave (13: the last three) an empty range and, at 100, the
# one before it a short one; 200 divides neither by 16 rows nor by 64 columns; 257 ends every row with a pass of one lane.
CROP_SIZES = (8, 13, 100, 200, 257)


def _fixed_point_source(minv, s):
    """The source pixel of every crop pixel as csrc/preprocess.hip computes it from the product's inverse map (roi_pixel: OpenCV's 10-bit
    fixed point) -> (sx [s,s], sy [s,s]) int64, before the bounds test."""
    j = np.arange(s, dtype=np.float64)
    X0 = np.rint((minv[0, 1] * j + minv[0, 2]) * 1024.0).astype(np.int64) + 512
    Y0 = np.rint((minv[1, 1] * j + minv[1, 2]) * 1024.0).astype(np.int64) + 512
    ax, ay = np.rint(minv[0, 0] * j * 1024.0).astype(np.int64), np.rint(minv[1, 0] * j * 1024.0).astype(np.int64)
    return np.clip((X0[:, None] + ax[None, :]) >> 10, -32768, 32767), np.clip((Y0[:, None] + ay[None, :]) >> 10, -32768, 32767)


@pytest.mark.parametrize("s", CROP_SIZES)
def test_host_window_and_inverse_map_equal_oracle_at_other_crop_sizes(s):
    """test_host_window_and_inverse_map_equal_oracle at the crop sizes of the GPU test below: the product's closed-form inverse map, put
    through the kernel's fixed-point arithmetic, selects exactly the source pixels the oracle's warp selects - which is what makes bit
    for bit a fair demand of the device at these sizes."""
    rng = np.random.default_rng(s)
    for _ in range(200):
        y1, x1 = int(rng.integers(0, 470)), int(rng.integers(0, 630))
        roi = [y1, x1, min(479, y1 + int(rng.integers(1, 470))), min(639, x1 + int(rng.integers(1, 630)))]
        win = pp.get_bbox(roi)
        assert win == po.get_bbox(roi)
        rmin, rmax, cmin, cmax = win
        center = np.array([0.5 * (cmin + cmax), 0.5 * (rmin + rmax)])
        scale = min(max(rmax - rmin, cmax - cmin), 640) * 1.0
        M = po.get_affine_transform(center, scale, s)
        mine = pp.inverse_crop_map(win, s, 480, 640)
        np.testing.assert_allclose(mine, cv2r.invertAffineTransform(M), rtol=0, atol=1e-9)
        sx, sy = cv2r.nearest_source_index(M, (s, s))
        gx, gy = _fixed_point_source(mine, s)
        np.testing.assert_array_equal(gx, sx)
        np.testing.assert_array_equal(gy, sy)


@functools.lru_cache(maxsize=None)
def _frame5():
    return synth.golden_depth_frame(5)  # (shared by the tests below, none of which writes to it)


@functools.lru_cache(maxsize=None)
def _oracle_instances(s):
    """Per instance of frame 5 at crop size s: (cloud or None, valid masked pixels, crop pixels with a depth reading), the oracle's."""
    depth, masks, rois, class_ids = _frame5()
    out = []
    for i in range(len(class_ids)):
        rmin, rmax, cmin, cmax = po.get_bbox(rois[i])
        center = np.array([0.5 * (cmin + cmax), 0.5 * (rmin + rmax)])
        scale = min(max(rmax - rmin, cmax - cmin), 640) * 1.0
        roi_depth = po.crop_resize_nearest(depth, center, scale, s)
        roi_mask = po.crop_resize_nearest(np.logical_and(masks[:, :, i], depth > 0).astype(np.float32), center, scale, s)
        cloud = po.instance_cloud(depth, masks[:, :, i], rois[i], po.REAL_INTRINSICS, img_size=s)
        if cloud is not None:
            cloud.setflags(write=False)
        out.append((cloud, int(((roi_mask > 0) & (roi_depth > 0)).sum()), int((roi_depth > 0).sum())))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", (64, 1024))
@pytest.mark.parametrize("s", CROP_SIZES)
def test_hip_clouds_bit_exact_at_other_crop_sizes(s, n):
    depth, masks, rois, class_ids = _frame5()
    d2c = pp.DepthToClouds(pp.REAL_INTRINSICS, n_pts=n, img_size=s)
    pcl, count, dcount = d2c.full_clouds(depth, masks, rois)
    assert pcl.shape == (len(class_ids), s * s, 3)
    count, dcount = count.cpu().numpy(), dcount.cpu().numpy()
    kept = []
    for i, (ref, c_ref, d_ref) in enumerate(_oracle_instances(s)):
        assert (int(count[i]), int(dcount[i])) == (c_ref, d_ref), i
        assert (ref is None) == (c_ref <= 1 or d_ref <= 1)
        if ref is not None:
            assert ref.shape[0] == c_ref
            np.testing.assert_array_equal(pcl[i, :c_ref].cpu().numpy(), ref)  # float32, bit for bit, same point order
            kept.append(i)
    got = d2c(depth, masks, rois, class_ids, rng=np.random.RandomState(11))
    pts, cat, inst = po.frame_clouds(depth, masks, rois, class_ids, po.REAL_INTRINSICS, n_pts=n, rng=np.random.RandomState(11), img_size=s)
    assert got["points"].shape == (len(kept), n, 3) and inst == kept
    np.testing.assert_array_equal(got["points"].cpu().numpy(), pts)
    assert got["cat_id"] == cat and got["valid_inst"] == inst


@pytest.mark.gpu
@pytest.mark.parametrize("s", (256, 100))
def test_hip_one_instance_alone_equals_its_row_of_the_frame(s):
    """masks [H,W,1] (mask stride 1) for the large, the small and a border instance, and a frame without detections: each gives what the
    six-instance call gives for that instance."""
    import torch
    depth, masks, rois, class_ids = _frame5()
    d2c = pp.DepthToClouds(pp.REAL_INTRINSICS, n_pts=64, img_size=s)
    pcl, count, dcount = d2c.full_clouds(depth, masks, rois)
    for i in (0, 1, 2, 3):  # large, small, touching the top border, touching the bottom right corner
        p1, c1, d1 = d2c.full_clouds(depth, masks[:, :, i:i + 1], rois[i:i + 1])
        c = int(count[i])
        assert p1.shape == (1, s * s, 3) and int(c1[0]) == c and int(d1[0]) == int(dcount[i])
        assert torch.equal(p1[0, :c], pcl[i, :c])
        got = d2c(depth, masks[:, :, i:i + 1], rois[i:i + 1], class_ids[i:i + 1], rng=np.random.RandomState(7))
        if c <= 1 or int(dcount[i]) <= 1:
            assert got["points"].shape == (0, 64, 3) and got["valid_inst"] == []
            continue
        want = po.sample_points(pcl[i, :c].cpu().numpy(), 64, np.random.RandomState(7))
        np.testing.assert_array_equal(got["points"].cpu().numpy()[0], want)
        assert got["cat_id"] == [int(class_ids[i]) - 1] and got["valid_inst"] == [0]
    p0, c0, d0 = d2c.full_clouds(depth, masks[:, :, :0], rois[:0])
    assert p0.shape == (0, s * s, 3) and c0.shape == (0,) and d0.shape == (0,)
    got = d2c(depth, masks[:, :, :0], rois[:0], class_ids[:0])
    assert got["points"].shape == (0, 64, 3) and got["cat_id"] == [] and got["valid_inst"] == []


@pytest.mark.gpu
def test_hip_cloud_sample_every_branch():
    """gp_cloud_sample itself: an empty instance (its rows stay as they were), one point, one short of npts, exactly npts (a plain copy), more
    than npts - with ids, negative and too-large entries among them (clamped to [0, count - 1]), and with ids = NULL (the first npts rows)."""
    import torch
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    npts, cap = 64, 100
    counts = np.array([0, 1, npts - 1, npts, cap], dtype=np.int32)
    rng = np.random.default_rng(0)
    pcl = rng.standard_normal((5, cap, 3)).astype(np.float32)
    ids = np.stack([rng.permutation(cap)[:npts] for _ in range(5)]).astype(np.int32)
    ids[:, 3], ids[:, 10], ids[:, 20], ids[:, 63] = -1, cap, -2 ** 31, 2 ** 31 - 1
    ids[:, 0], ids[:, 1] = 0, cap - 1
    d_pcl, d_cnt, d_ids = torch.from_numpy(pcl).cuda(), torch.from_numpy(counts).cuda(), torch.from_numpy(ids).cuda()
    for use_ids in (True, False):
        out = torch.full((5, npts, 3), -77.0, device="cuda")
        _lib.call("gp_cloud_sample", 5, cap, npts, ptr(d_pcl), ptr(d_cnt), ptr(d_ids) if use_ids else None, ptr(out), stream_ptr())
        out = out.cpu().numpy()
        assert (out[0] == -77.0).all()
        for i in (1, 2, 3):
            np.testing.assert_array_equal(out[i], po.sample_points(pcl[i, :counts[i]], npts), err_msg=f"count {counts[i]}")
            np.testing.assert_array_equal(out[i], pcl[i, np.arange(npts) % counts[i]])
        rows = np.clip(ids[4].astype(np.int64), 0, cap - 1) if use_ids else np.arange(npts)
        np.testing.assert_array_equal(out[4], pcl[4, rows])


@pytest.mark.gpu
def test_hip_clouds_feed_the_runner():
    """Pre-processing output goes straight into the agents: clouds stay on the device."""
    import torch
    from genpose_amd.config import get_config
    from genpose_amd.posenet_agent import PoseNet
    from genpose_amd.weights_synth import make_state_dict
    depth, masks, rois, class_ids = synth.golden_depth_frame()
    got = pp.DepthToClouds(pp.REAL_INTRINSICS)(depth, masks, rois, class_ids, rng=np.random.RandomState(1))
    agent = PoseNet(get_config(posenet_mode="score", sampler_mode=["pc"], sampling_steps=8))
    agent.load_state_dict(make_state_dict(0, "score"))
    pts = got["points"]
    pred = agent.pred_func({"pts": pts, "pts_center": pts.mean(dim=1)}, repeat_num=4, save_path=None)
    assert pred.shape == (len(got["valid_inst"]), 4, 9) and torch.isfinite(pred).all()
