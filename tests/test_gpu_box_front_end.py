"""GPU: the mask-free front end - gp_cloud_extent and gp_box_sample (csrc/preprocess.hip), reward.cloud_extent and
preprocess.DepthToClouds.device_clouds_boxes.  Every comparison is bit for bit, against the numpy float32 restatements of
tests/box_front_end_reference.py (held to float64 geometry and hand-made arrays by tests/test_box_front_end_host.py).

The boxes (box_front_end_reference.cases) sit on objects 0-3 of synth.golden_depth_frame(5) under seeded rotations, one a 45-degree turn
about the optical axis, and on hand-made images; with 64 and 1024 points they reach every branch of the draw - c > n (the seeded walk),
1 < c < n (tiling), c == n (an axis-aligned box on a plane), c <= 1 (one pixel, a depth hole, behind the camera, off the image) - and the
rectangle's edge cases: a box centred off the image whose corner reaches in, one on the image border, one 0.1 m from the camera with a
large projection, one with a corner behind the near plane (the whole image), one holding the whole frame (4 800 segments) and a 97 x 131
image.  The reference counts over the WHOLE image, the kernel over the rectangle: equal counts are the rectangle's superset check."""
import functools

import numpy as np
import pytest
import torch

import box_front_end_reference as ref

pytestmark = pytest.mark.gpu

SEED = 0xFEED5EED12345678
RUN = 7
SLOT0 = 3
N_PTS = (64, 1024)
K = (591.0125, 590.16775, 322.525, 244.11084)  # REAL_INTRINSICS


@functools.lru_cache(maxsize=None)
def _images():
    return ref.images()


@functools.lru_cache(maxsize=None)
def _groups():
    """The cases that can share a launch: (image, inflate, pad) -> [(name, rt, half)], in the order of the case list."""
    g = {}
    for name, image, rt, half, inflate, pad in ref.cases(K):
        g.setdefault((image, inflate, pad), []).append((name, rt, half))
    return g


@functools.lru_cache(maxsize=None)
def _expected(n_pts):
    """name -> (points [n_pts,3], count, valid) by the whole-image definition, drawn as its slot in its group's launch."""
    im, out = _images(), {}
    for (image, inflate, pad), members in _groups().items():
        for i, (name, rt, half) in enumerate(members):
            out[name] = ref.box_sample(im[image], K, rt, half, inflate, pad, 2, n_pts, SEED, RUN, SLOT0 + i)
    return out


def _fe(n_pts):
    from genpose_amd.preprocess import DepthToClouds
    return DepthToClouds(n_pts=n_pts)


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _seed_words(run=RUN, slot0=SLOT0):
    w = np.array([SEED & 0xFFFFFFFF, SEED >> 32, run, 0, slot0, 0, 0, 0], dtype=np.uint32)
    return torch.from_numpy(w.view(np.int32)).cuda()


def _raw(depth, rt, half, n_pts, inflate=1.0, pad=0.0, min_count=2, frame_of=None, draw=None, seed=None, out=None, nobj=None, **over):
    """gp_box_sample itself on device tensors -> (rc, out dict)."""
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    depth = depth if depth.dim() == 3 else depth.unsqueeze(0)
    F, H, W = depth.shape
    n = rt.shape[0] if nobj is None else nobj
    seed = _seed_words() if seed is None else seed
    if out is None:
        out = {"points": torch.empty(n, n_pts, 3, device="cuda"), "count": torch.zeros(n, dtype=torch.int32, device="cuda"),
               "valid": torch.zeros(n, dtype=torch.uint8, device="cuda")}
    a = dict(h=H, w=W, nframes=F, nobj=n, npts=n_pts, p_depth=ptr(depth), p_frame_of=ptr(frame_of), p_rt=ptr(rt), p_half=ptr(half), inflate=inflate,
             pad=pad, min_count=min_count, fx=K[0], fy=K[1], cx=K[2], cy=K[3], p_seed=ptr(seed), p_draw=ptr(draw), p_points=ptr(out["points"]),
             p_count=ptr(out["count"]), p_valid=ptr(out["valid"]), s=stream_ptr())
    assert set(over) <= set(a), over
    a.update(over)
    return _lib.lib().gp_box_sample(*a.values()), out


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _depth_dev(image):
    return torch.from_numpy(_images()[image].view(np.int16)).cuda()


def _stack(members):
    return np.stack([m[1] for m in members]), np.stack([m[2] for m in members])


@pytest.mark.parametrize("n_pts", N_PTS)
def test_rows_counts_and_flags_equal_the_whole_image_definition(n_pts):
    fe, want = _fe(n_pts), _expected(n_pts)
    for (image, inflate, pad), members in _groups().items():
        rt, half = _stack(members)
        got = fe.device_clouds_boxes(_images()[image], *_dev(rt, half), SEED, RUN, inflate=inflate, pad=pad, slot_base=SLOT0)
        assert all(v.is_cuda for v in got.values())
        got = _host(got)
        assert got["points"].shape == (len(members), n_pts, 3) and got["count"].dtype == torch.int32 and got["valid"].dtype == torch.uint8
        for i, (name, _, _) in enumerate(members):
            pts, c, valid = want[name]
            print(f"{name}: count {int(got['count'][i])} (whole image {c}), valid {int(got['valid'][i])}")
            assert int(got["count"][i]) == c, (name, "the rectangle is no superset" if int(got["count"][i]) < c else "count")
            assert int(got["valid"][i]) == valid, name
            assert np.array_equal(got["points"][i].numpy().view(np.uint32), pts.view(np.uint32)), \
                f"{name}: {int((got['points'][i].numpy() != pts).any(axis=1).sum())} of {n_pts} rows differ"


def test_every_branch_really_occurs():
    for n in N_PTS:
        want = _expected(n)
        c = {k: v[1] for k, v in want.items()}
        assert any(v > n for v in c.values()) and any(1 < v < n for v in c.values()) and c[f"plane_{n}"] == n and want[f"plane_{n}"][2] == 1
        for k in ("millimetre", "hole", "behind", "off_image"):
            assert c[k] <= 1 and want[k][2] == 0, k
        assert c["millimetre"] == 1  # (a pixel inside, and still no cloud)
    c = {k: v[1] for k, v in _expected(1024).items()}
    assert c["obj2_medium"] > 64 and c["obj2_medium"] < 1024  # one box on both branches
    assert c["whole_frame"] == int((_images()["frame"] > 0).sum()) and c["near_plane_corner"] > 1024 and c["near_large"] > 1024
    assert c["corner_reaches_in"] > 1024 and c["obj3_border"] > 1024 and c["small_image"] > 1024
    im = _images()["frame"]
    m = ref.inside_mask(im, K, *[(rt, half, inflate, pad) for name, image, rt, half, inflate, pad in ref.cases(K) if name == "obj3_border"][0])
    assert m[:, -1].any() and m[-1, :].any()  # the border box has inside pixels in the last column and the last row


def test_a_rectangle_above_the_segment_cap_is_refused_whole():
    from genpose_amd import _lib
    cap = _lib.lib().gp_box_sample_max_segments()
    assert 4800 <= cap < 720 * 20
    depth = torch.full((720, 1280), 800, dtype=torch.int16, device="cuda")
    rt = np.stack([ref.pose(np.eye(3, dtype=np.float32), [0, 0, 1.0]), ref.pose(np.eye(3, dtype=np.float32), ref.centre_of(700, 300, 0.8, K))])
    half = np.array([[5, 5, 5], [0.02, 0.02, 0.02]], dtype=np.float32)
    rc, got = _raw(depth, *_dev(rt, half), 64)
    got = _host(got)
    assert rc == 0 and got["count"][0] == -1 and got["valid"][0] == 0 and (got["points"][0] == 0).all()
    pts, c, valid = ref.box_sample(np.full((720, 1280), 800, np.uint16), K, rt[1], half[1], 1.0, 0.0, 2, 64, SEED, RUN, SLOT0 + 1)
    assert valid == 1 and int(got["count"][1]) == c and int(got["valid"][1]) == 1 and np.array_equal(got["points"][1].numpy(), pts)


def test_non_finite_boxes_and_frames_out_of_range_are_invalid_objects_and_leave_their_neighbours_alone():
    n_pts, image = 64, "frame"
    members = _groups()[(image, 1.0, 0.0)]
    good = [m for m in members if m[0] in ("obj0_turn45", "obj1_tiny")]
    rt0, half0 = _stack(good)
    depth = _depth_dev(image)
    base = _host(_raw(depth, *_dev(rt0, half0), n_pts, draw=_dev(np.array([[RUN, 10], [RUN, 11]], dtype=np.uint32).view(np.int32))[0])[1])
    bad_rt, bad_half = [], []
    for k, v in ((("rt", 0, 0), np.nan), (("rt", 1, 3), np.inf), (("rt", 3, 3), np.nan), (("half", 1), np.nan), (("half", 0), np.inf), (("half", 2), -0.05),
                 (("half", 1), 0.0)):
        r, h = rt0[0].copy(), half0[0].copy()
        if k[0] == "rt":
            r[k[1], k[2]] = v
        else:
            h[k[1]] = v
        bad_rt.append(r)
        bad_half.append(h)
    nb = len(bad_rt)
    # good 0, the bad ones, good 1, good 0 on a frame out of range (twice)
    rt = np.stack([rt0[0]] + bad_rt + [rt0[1], rt0[0], rt0[0]])
    half = np.stack([half0[0]] + bad_half + [half0[1], half0[0], half0[0]])
    frame_of = np.array([0] * (nb + 2) + [-1, 1], dtype=np.int32)
    draw = np.array([[RUN, 10]] + [[RUN, 20 + i] for i in range(nb)] + [[RUN, 11], [RUN, 30], [RUN, 31]], dtype=np.uint32).view(np.int32)
    rc, got = _raw(depth, *_dev(rt, half), n_pts, frame_of=_dev(frame_of)[0], draw=_dev(draw)[0])
    got = _host(got)
    assert rc == 0
    for k in base:
        assert torch.equal(got[k][0], base[k][0]) and torch.equal(got[k][nb + 1], base[k][1]), k
    assert int(base["valid"][0]) == 1 and int(base["valid"][1]) == 1
    im = _images()[image]
    for i in range(nb):
        c = int(ref.inside_mask(im, K, bad_rt[i], bad_half[i], 1.0, 0.0).sum())
        assert int(got["valid"][1 + i]) == 0 and (got["points"][1 + i] == 0).all() and int(got["count"][1 + i]) == c, (i, c)
    for i in (nb + 2, nb + 3):
        assert int(got["valid"][i]) == 0 and int(got["count"][i]) == 0 and (got["points"][i] == 0).all()


@pytest.mark.parametrize("n_pts", N_PTS)
def test_alone_in_company_in_any_order_and_across_frames(n_pts):
    """An object's outputs are a function of its own box, frame and (run, slot): alone, in company, in another order, and with two frames
    in one launch under frame_of."""
    members = _groups()[("frame", 1.0, 0.0)]
    rt, half = _stack(members)
    n = len(members)
    depth = _depth_dev("frame")
    draw = np.array([[RUN, SLOT0 + i] for i in range(n)], dtype=np.uint32)
    company = _host(_raw(depth, *_dev(rt, half), n_pts, draw=_dev(draw.view(np.int32))[0])[1])
    want = _expected(n_pts)
    for i, (name, _, _) in enumerate(members):  # (the draw table and the seed words give the same draw)
        assert int(company["count"][i]) == want[name][1] and np.array_equal(company["points"][i].numpy(), want[name][0]), name
    for i in range(n):
        alone = _host(_raw(depth, *_dev(rt[i:i + 1], half[i:i + 1]), n_pts, seed=_seed_words(slot0=SLOT0 + i))[1])
        for k in company:
            assert torch.equal(alone[k][0], company[k][i]), (members[i][0], k)
    perm = np.random.default_rng(5).permutation(n)
    shuffled = _host(_raw(depth, *_dev(rt[perm], half[perm]), n_pts, draw=_dev(draw[perm].view(np.int32))[0])[1])
    for k in company:
        assert torch.equal(shuffled[k], company[k][torch.from_numpy(perm)]), k
    # two frames of one size: the frame and the near image, their boxes interleaved
    near = _groups()[("near", 1.0, 0.0)]
    rt_n, half_n = _stack(near)
    near_alone = _host(_raw(_depth_dev("near"), *_dev(rt_n, half_n), n_pts, draw=_dev(np.array([[RUN + 1, 40 + i] for i in range(len(near))], dtype=np.uint32).view(np.int32))[0])[1])
    both = torch.stack([depth, _depth_dev("near")])
    rt2, half2 = np.concatenate([rt_n[:1], rt, rt_n[1:]]), np.concatenate([half_n[:1], half, half_n[1:]])
    frame_of = np.array([1] + [0] * n + [1] * (len(near) - 1), dtype=np.int32)
    draw2 = np.concatenate([[[RUN + 1, 40]], draw, [[RUN + 1, 40 + i] for i in range(1, len(near))]]).astype(np.uint32)
    joint = _host(_raw(both, *_dev(rt2, half2), n_pts, frame_of=_dev(frame_of)[0], draw=_dev(draw2.view(np.int32))[0])[1])
    for k in company:
        assert torch.equal(joint[k][1:1 + n], company[k]), k
        assert torch.equal(joint[k][0], near_alone[k][0]) and torch.equal(joint[k][1 + n:], near_alone[k][1:]), k


def test_host_inputs_device_inputs_out_reuse_and_min_count():
    n_pts = 64
    fe = _fe(n_pts)
    members = _groups()[("frame", 1.0, 0.0)]
    rt, half = _stack(members)
    im = _images()["frame"]
    a = fe.device_clouds_boxes(im, rt, half, SEED, RUN, inflate=1.0, pad=0.0, slot_base=SLOT0)  # host arrays
    b = fe.device_clouds_boxes(_depth_dev("frame"), *_dev(rt, half), SEED, RUN, inflate=1.0, pad=0.0, slot_base=SLOT0)  # device tensors
    ha, hb = _host(a), _host(b)
    for k in ha:
        assert torch.equal(ha[k], hb[k]), k
    # many frames as one host array, frame_of; written into the first call's tensors
    two = np.stack([_images()["plane"], im])
    c = fe.device_clouds_boxes(two, rt, half, SEED, RUN, frame_of=np.ones(len(rt), dtype=np.int64), inflate=1.0, pad=0.0, slot_base=SLOT0, out=a)
    assert all(c[k] is a[k] for k in a)
    hc = _host(c)
    for k in ha:
        assert torch.equal(hc[k], hb[k]), k
    # min_count above a box's count: that object alone turns invalid
    names = [m[0] for m in members]
    i, cnt = names.index("obj3_border"), int(hb["count"][names.index("obj3_border")])
    d = _host(fe.device_clouds_boxes(im, rt, half, SEED, RUN, inflate=1.0, pad=0.0, slot_base=SLOT0, min_count=cnt + 1))
    e = _host(fe.device_clouds_boxes(im, rt, half, SEED, RUN, inflate=1.0, pad=0.0, slot_base=SLOT0, min_count=cnt))
    assert int(d["valid"][i]) == 0 and (d["points"][i] == 0).all() and int(d["count"][i]) == cnt and int(e["valid"][i]) == 1
    assert torch.equal(e["points"][i], hb["points"][i])  # (at the bar exactly: still a cloud, the same one)
    keep = torch.tensor([j for j in range(len(names)) if hb["count"][j] > cnt or hb["valid"][j] == 0])  # (what the higher bar does not reach)
    assert torch.equal(d["points"][keep], hb["points"][keep])
    # no object: no launch, empty tensors
    z = fe.device_clouds_boxes(im, np.zeros((0, 4, 4), np.float32), np.zeros((0, 3), np.float32), SEED, RUN)
    assert z["points"].shape == (0, n_pts, 3) and z["count"].shape == (0,)


def test_the_launch_is_capturable_and_replays_on_overwritten_buffers():
    n_pts = 1024
    members = _groups()[("frame", 1.0, 0.0)]
    rt, half = _stack(members)
    n = len(members)
    depth, rt_d, half_d = _depth_dev("near").clone(), *_dev(rt[::-1], half[::-1])
    seed = _seed_words()
    rc, out = _raw(depth, rt_d, half_d, n_pts, seed=seed)  # the first call, outside capture
    assert rc == 0
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            rc, _ = _raw(depth, rt_d, half_d, n_pts, seed=seed, out=out)
    assert rc == 0
    depth.copy_(_depth_dev("frame"))
    rt_d.copy_(_dev(rt)[0])
    half_d.copy_(_dev(half)[0])
    for v in out.values():
        v.fill_(7)
    g.replay()
    got, want = _host(out), _expected(n_pts)
    for i, (name, _, _) in enumerate(members):
        assert int(got["count"][i]) == want[name][1] and int(got["valid"][i]) == want[name][2] and np.array_equal(got["points"][i].numpy(), want[name][0]), name


def test_argument_errors_write_nothing_and_no_object_is_fine():
    n_pts = 64
    members = _groups()[("frame", 1.0, 0.0)][:2]
    rt, half = _dev(*_stack(members))
    depth = _depth_dev("frame")
    out = {"points": torch.full((2, n_pts, 3), 7.0, device="cuda"), "count": torch.full((2,), 7, dtype=torch.int32, device="cuda"),
           "valid": torch.full((2,), 7, dtype=torch.uint8, device="cuda")}
    nan, inf = float("nan"), float("inf")
    bad = [dict(h=0), dict(w=0), dict(h=32768), dict(w=32768), dict(nframes=0), dict(nobj=-1), dict(npts=0), dict(inflate=0.0), dict(inflate=-1.0),
           dict(inflate=nan), dict(inflate=inf), dict(pad=-0.001), dict(pad=nan), dict(pad=inf), dict(min_count=-1), dict(p_depth=None), dict(p_rt=None),
           dict(p_half=None), dict(p_seed=None), dict(p_points=None), dict(p_count=None), dict(p_valid=None)]
    for kw in bad:
        rc, _ = _raw(depth, rt, half, n_pts, out=out, **kw)
        assert rc == -1, kw
    torch.cuda.synchronize()
    assert (out["points"] == 7).all() and (out["count"] == 7).all() and (out["valid"] == 7).all()
    rc, _ = _raw(depth, rt, half, n_pts, out=out, nobj=0)
    torch.cuda.synchronize()
    assert rc == 0 and (out["points"] == 7).all()


# ------------------------------------------------------------------ gp_cloud_extent
def _clouds(b, n, seed):
    rng = np.random.default_rng([n, b, seed])
    rt = np.stack([ref.pose(ref.rotation(rng), rng.uniform(-0.3, 0.3, 3) + [0, 0, 0.8]) for _ in range(b)])
    pts = (rng.uniform(-0.1, 0.1, (b, n, 3)) + rt[:, None, :3, 3]).astype(np.float32)
    return pts, rt


def _extent(pts, rt, trim, sym=None):
    from genpose_amd import reward
    out = reward.cloud_extent(*_dev(pts, rt), trim=trim, sym=sym)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check_extent(pts, rt, trims, tag):
    b, n = pts.shape[:2]
    for trim in sorted({t for t in trims if 0 <= t < n}):
        for sym in (None, [i % 2 == 0 for i in range(b)], [True] * b):
            got = _extent(pts, rt, trim, sym)
            want = np.stack([ref.extent_reference(pts[i], rt[i], trim, bool(sym[i]) if sym else False) for i in range(b)])
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (tag, n, b, trim, sym, got, want)
            assert (got == np.abs(got)).all()


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1500])
def test_cloud_extent_is_the_exact_order_statistic(n, b):
    pts, rt = _clouds(b, n, 0)
    _check_extent(pts, rt, (0, 1, 5, n - 1), "random")


def test_cloud_extent_with_duplicates_and_exact_ties():
    from genpose_amd import synth
    rng = np.random.default_rng(77)
    few, rt = _clouds(2, 300, 1)
    tiled = few[:, np.arange(1024) % 300]  # every point three or four times
    _check_extent(tiled, rt, (0, 1, 2, 3, 4, 5, 1023), "tiled")
    g = synth.golden_clouds()
    grid = g[3:4]  # an exact 32 x 32 grid on a plane
    for R in (np.eye(3, dtype=np.float32), ref.rotation(rng, about_z=90.0), ref.rotation(rng)):
        rt = ref.pose(R, grid[0].mean(0))[None]
        _check_extent(grid, rt, (0, 1, 5, 31, 32, 1023), "grid")
    q = ref.object_frame(grid[0], ref.pose(np.eye(3, dtype=np.float32), grid[0].mean(0)))
    assert len(np.unique(np.abs(q[:, 0]))) <= 32  # (the ties are there)
    allc = np.concatenate([g, tiled[:1]])
    rts = np.stack([ref.pose(ref.rotation(rng), c.mean(0)) for c in allc])
    _check_extent(allc, rts, (0, 10), "golden")


def test_a_cloud_alone_measures_what_it_measures_in_a_batch_and_nothing_is_written_on_an_error():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    pts, rt = _clouds(3, 1024, 2)
    sym = [True, False, True]
    batch = _extent(pts, rt, 5, sym)
    for i in range(3):
        assert np.array_equal(_extent(pts[i:i + 1], rt[i:i + 1], 5, sym[i:i + 1]), batch[i:i + 1])
    p, r = _dev(pts, rt)
    out = torch.full((3, 3), 7.0, device="cuda")
    L = _lib.lib()
    for b, n, pp, rr, trim, oo in ((-1, 1024, p, r, 0, out), (3, 0, p, r, 0, out), (3, _lib.EXTENT_MAX_N + 1, p, r, 0, out), (3, 1024, p, r, -1, out),
                                   (3, 1024, p, r, 1024, out), (3, 1024, None, r, 0, out), (3, 1024, p, None, 0, out), (3, 1024, p, r, 0, None)):
        assert L.gp_cloud_extent(b, n, ptr(pp), ptr(rr), trim, None, ptr(oo), stream_ptr()) == -1
    assert L.gp_cloud_extent(0, 1024, ptr(p), ptr(r), 0, None, ptr(out), stream_ptr()) == 0
    torch.cuda.synchronize()
    assert (out == 7).all()
    nanp = pts.copy()
    nanp[0, 5] = np.nan
    nanp[1, 7] = np.inf
    got = _extent(nanp, rt, 0)  # neither a fault nor a hang; the finite cloud is untouched
    assert np.array_equal(got[2], _extent(pts, rt, 0)[2])


def test_the_box_of_a_clouds_extent_holds_the_cloud():
    """Closure: object 0's cloud from the mask front end, a pose at its mean under a seeded rotation, half = its extent (trim 0); the box of
    exactly that size (inflate 1, pad 0) then counts at least the cloud's distinct pixels and its full cloud holds every one of them - which
    holds because both kernels evaluate ONE object-frame expression."""
    from genpose_amd import reward, synth
    from genpose_amd.preprocess import DepthToClouds
    depth, masks, rois, _ = synth.golden_depth_frame(5)
    fe = DepthToClouds(n_pts=1024)
    cloud = fe.device_clouds(depth, masks[:, :, :1], rois[:1], SEED, RUN)["points"]
    pts = cloud[0].cpu().numpy()
    rt = ref.pose(ref.rotation(np.random.default_rng(9)), pts.mean(0))
    half = reward.cloud_extent(cloud, _dev(rt[None])[0])
    box = _host(fe.device_clouds_boxes(depth, _dev(rt[None])[0], half, SEED, RUN, inflate=1.0, pad=0.0))
    half_h = half.cpu().numpy()[0]
    assert np.array_equal(half_h, ref.extent_reference(pts, rt, 0))
    distinct = np.unique(pts, axis=0)
    full = ref.full_cloud(depth, K, rt, half_h, 1.0, 0.0)
    # (the crop up-samples the object's window, so some of the cloud's 1024 rows show one source pixel twice: fewer distinct points than rows)
    assert int(box["count"][0]) == len(full) >= len(distinct) > 512 and int(box["valid"][0]) == 1
    assert set(map(bytes, distinct)) <= set(map(bytes, full))
