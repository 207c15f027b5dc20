"""CPU: the host side of the mask-free front end (gp_cloud_extent, gp_box_sample, gp_box_sample_max_segments; reward.cloud_extent,
preprocess.DepthToClouds.device_clouds_boxes, runner.DepthTracker) - the three symbols declared and bound with the header's arity, every
stated argument error of the Python wrappers, and the numpy restatements of tests/box_front_end_reference.py held to something other than
themselves: the float32 inside test to a float64 evaluation of the geometry, the order statistic to hand-made arrays."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import box_front_end_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (591.0125, 590.16775, 322.525, 244.11084)


def _header_args(name):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genpose_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/genpose_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    return [] if args == ["void"] else args


@pytest.mark.parametrize("name", ["gp_cloud_extent", "gp_box_sample", "gp_box_sample_max_segments"])
def test_symbol_is_declared_and_bound_with_the_headers_arity(name):
    from genpose_amd import _lib
    args = _header_args(name)
    sig = _lib.SIGNATURES[name]
    assert len(sig) == len(args), (name, len(sig), args)
    for a, c in zip(args, sig):  # pointers and the stream are void pointers, ints ints, floats floats
        want = _lib.P if ("*" in a or a.startswith("gp_stream_t")) else {"int": ctypes.c_int, "float": ctypes.c_float}[a.split()[0]]
        assert c is want, (name, a, c)


def test_header_limit_matches_the_binding():
    from genpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "genpose_hip.h")).read()
    assert int(re.search(r"#define GP_EXTENT_MAX_N (\d+)", hdr).group(1)) == _lib.EXTENT_MAX_N >= 4096


def test_cloud_extent_refuses_every_stated_argument_error():
    from genpose_amd import _lib, reward
    pts, rt = torch.zeros(2, 8, 3), torch.eye(4).repeat(2, 1, 1)
    bad = [dict(pts=torch.zeros(2, 8, 4)), dict(pts=torch.zeros(8, 3)), dict(pts=pts.double()), dict(rt=torch.eye(4).repeat(3, 1, 1)),
           dict(rt=rt.double()), dict(rt=torch.zeros(2, 3, 4)), dict(pts=torch.zeros(2, 0, 3)), dict(pts=torch.zeros(1, _lib.EXTENT_MAX_N + 1, 3), rt=rt[:1]),
           dict(trim=-1), dict(trim=8), dict(trim=1.5), dict(sym=torch.zeros(3)), dict(sym=[1])]
    for kw in bad:
        args = dict(pts=pts, rt=rt, trim=0, sym=None)
        args.update(kw)
        with pytest.raises(ValueError):
            reward.cloud_extent(**args)
    with pytest.raises(ValueError, match="GPU"):  # well-formed host tensors: there is no CPU fallback
        reward.cloud_extent(pts, rt)


def test_device_clouds_boxes_refuses_every_stated_argument_error():
    from genpose_amd.preprocess import check_box_inputs
    depth = np.zeros((48, 64), dtype=np.uint16)
    rt, half = np.tile(np.eye(4, dtype=np.float32), (2, 1, 1)), np.full((2, 3), 0.1, dtype=np.float32)
    good = dict(depth=depth, rt=rt, half=half, frame_of=None, inflate=1.15, pad=0.01, min_count=2)
    d, r, h, f, F, H, W, n = check_box_inputs(**good)
    assert (F, H, W, n) == (1, 48, 64, 2) and f is None and r.dtype == torch.float32
    assert check_box_inputs(**{**good, "depth": np.zeros((3, 48, 64), np.uint16), "frame_of": [0, 2]})[4] == 3
    bad = [dict(depth=np.zeros((48, 64), np.float32)), dict(depth=torch.zeros(48, 64, dtype=torch.int32)), dict(depth=np.zeros((0, 48, 64), np.uint16)),
           dict(depth=np.zeros((48,), np.uint16)), dict(depth=np.zeros((1, 1, 48, 64), np.uint16)),
           dict(rt=rt[0]), dict(rt=np.zeros((2, 3, 4), np.float32)), dict(rt=torch.zeros(2, 4, 4, dtype=torch.float64)), dict(half=half[:1]),
           dict(half=np.zeros((2, 2), np.float32)), dict(frame_of=[0]), dict(frame_of=np.zeros(2, np.float32)), dict(inflate=0.0), dict(inflate=-1.0),
           dict(inflate=float("nan")), dict(inflate=float("inf")), dict(pad=-0.01), dict(pad=float("nan")), dict(pad=float("inf")), dict(min_count=-1),
           dict(min_count=2.5)]
    for kw in bad:
        with pytest.raises((ValueError, RuntimeError)):
            check_box_inputs(**{**good, **kw})


def test_depth_tracker_refuses_every_stated_argument_error():
    from genpose_amd.runner import DepthTracker

    class Tracker:  # (the constructor looks at the tracker's mode alone)
        init, max_objects, seed = "prior", 8, 0
    for kw in (dict(trim=-1), dict(trim=1.5), dict(inflate=0.0), dict(inflate=float("nan")), dict(pad=-1.0), dict(min_count=-1)):
        with pytest.raises(ValueError):
            DepthTracker(Tracker(), front_end=object(), **kw)
    gt = Tracker()
    gt.init = "gt"
    with pytest.raises(ValueError, match="prior"):
        DepthTracker(gt, front_end=object())
    with pytest.raises(RuntimeError, match="acquire"):
        DepthTracker(Tracker(), front_end=object()).track(np.zeros((48, 64), np.uint16))


def test_the_restated_inside_test_agrees_with_float64_geometry():
    """Every case of the GPU test: where a pixel's float64 point lies more than 1e-4 m from every face of the box, the float32 restatement
    decides as the float64 geometry does - and such pixels exist on both sides."""
    im = ref.images()
    fx, fy, cx, cy = K
    for name, image, rt, half, inflate, pad in ref.cases(K):
        depth = im[image]
        H, W = depth.shape
        d = depth.astype(np.float64)
        sx, sy = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
        p = np.stack([(sx - cx) * d / fx / 1000, (sy - cy) * d / fy / 1000, d / 1000], axis=-1)
        R, t = rt[:3, :3].astype(np.float64), rt[:3, 3].astype(np.float64)
        q = (p - t) @ R  # q_j = sum_i u_i R[i][j]
        hh = half.astype(np.float64) * inflate + pad
        margin = np.abs(np.abs(q) - hh).min(axis=-1)
        inside64 = (depth > 0) & np.all(np.abs(q) <= hh, axis=-1)
        clear = (depth > 0) & (margin > 1e-4)
        got = ref.inside_mask(depth, K, rt, half, inflate, pad)
        assert clear.any(), name
        np.testing.assert_array_equal(got[clear], inside64[clear], err_msg=name)
        assert not got[depth == 0].any()


def test_extent_reference_on_hand_made_arrays():
    a = np.array([[3, 1, 0], [1, 1, 0], [3, 2, 0], [2, 1, 0], [3, 1, 0]], dtype=np.float32)  # ties and duplicates, a constant column
    assert ref.order_statistic(a, 0).tolist() == [3, 2, 0]
    assert ref.order_statistic(a, 1).tolist() == [3, 1, 0]
    assert ref.order_statistic(a, 2).tolist() == [3, 1, 0]
    assert ref.order_statistic(a, 3).tolist() == [2, 1, 0]
    assert ref.order_statistic(a, 4).tolist() == [1, 1, 0]
    # through the object frame: identity pose at t, signs do not matter, the symmetric form measures the radius in the x-z plane
    t = np.array([0.5, -0.25, 1.0], dtype=np.float32)
    q = np.array([[0.5, -0.125, 0.0], [-0.25, 0.125, 0.0], [0.0, 0.0, -0.75], [0.375, 0.0, 0.5]], dtype=np.float32)  # (exact in float32)
    rt = ref.pose(np.eye(3, dtype=np.float32), t)
    assert ref.extent_reference(q + t, rt, 0).tolist() == [0.5, 0.125, 0.75]
    assert ref.extent_reference(q + t, rt, 1).tolist() == [0.375, 0.125, 0.5]
    assert ref.extent_reference(q + t, rt, 3).tolist() == [0.0, 0.0, 0.0]
    assert ref.extent_reference(q + t, rt, 0, sym=True).tolist() == [0.75, 0.125, 0.75]
    assert ref.extent_reference(q + t, rt, 1, sym=True).tolist() == [0.625, 0.125, 0.625]  # (0.375, 0.5: a 3-4-5 triangle)
    # a quarter turn about z maps the camera's x to the object's -y... the extents swap columns
    Rz = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], dtype=np.float32)
    assert ref.extent_reference(q @ Rz.T + t, ref.pose(Rz, t), 0).tolist() == [0.5, 0.125, 0.75]


def test_the_cases_hit_every_branch_of_the_draw():
    """Device-free twin of the GPU test's branch check: the reference's counts put the cases on every branch for 64 and 1024 points."""
    im = ref.images()
    c = {name: int(ref.inside_mask(im[image], K, rt, half, inflate, pad).sum()) for name, image, rt, half, inflate, pad in ref.cases(K)}
    for n in (64, 1024):
        assert any(v > n for v in c.values()) and any(1 < v < n for v in c.values()) and c[f"plane_{n}"] == n
    assert all(c[k] <= 1 for k in ("millimetre", "hole", "behind", "off_image")) and c["millimetre"] == 1
    assert c["whole_frame"] > 250_000 and c["corner_reaches_in"] > 64 and c["near_large"] > 100_000
