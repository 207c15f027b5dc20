"""GPU: the depth front end over MANY frames in one launch - gp_roi_sample_frames (csrc/preprocess.hip), preprocess.DepthToClouds
.launch_frames / device_clouds_frames / detect and SingleFrameRunner.infer_depth_frames.  The yardstick is the per-frame launch
(gp_roi_sample_seeded through device_clouds, itself held to gp_roi_to_cloud's rows and the numpy definition of the draw by
tests/test_gpu_depth_front_end.py): a detection's four outputs are bit for bit what that launch writes for it, whatever shares the batched
launch and in whatever order; host and device inputs agree; the launch is capturable; the runner's batched depth entry point equals its
cloud entry point fed the batched front end's clouds; detect keeps what __call__ keeps."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0xFEED5EED12345678  # (bit 63 set: the whole 64 bits travel)
RUN = 7
SLOT_BASE = 3
CONFIGS = [(8, 64), (100, 64), (256, 64), (256, 1024)]  # (crop, points)
KEYS = ("points", "count", "depth_count", "valid")
SECOND_CHANNELS = [0, 2, 5]  # of the second frame: its depth hole, a border object, its large object


@functools.lru_cache(maxsize=None)
def _first_frame():
    from genpose_amd import synth
    return synth.golden_depth_frame(5)


@functools.lru_cache(maxsize=None)
def _second_frame():
    """Another frame of the same size and detection count: other depth, the detections in reverse order (with their class ids)."""
    from genpose_amd import synth
    depth, masks, rois, cls = synth.golden_depth_frame(9)
    return ((depth + np.uint16(37) * (depth > 0)).astype(np.uint16), np.ascontiguousarray(masks[:, :, ::-1]), np.ascontiguousarray(rois[::-1]),
            np.ascontiguousarray(cls[::-1]))


def _restrict(frame, ch):
    return (frame[0], np.ascontiguousarray(frame[1][:, :, ch]), np.ascontiguousarray(frame[2][ch])) + tuple(np.ascontiguousarray(x[ch]) for x in frame[3:])


@functools.lru_cache(maxsize=None)
def _frames():
    """Frame 5 (6 detections: large, small, at the border, the empty mask, the depth hole), a frame without detections, three channels of the second frame."""
    d0, m0, r0, _ = _first_frame()
    empty = (_second_frame()[0], np.zeros(m0.shape[:2] + (0,), dtype=bool), np.zeros((0, 4), dtype=np.int32))
    return ((d0, m0, r0), empty, _restrict(_second_frame()[:3], SECOND_CHANNELS))


N_F = (6, 0, 3)
FRAME = [0] * 6 + [2] * 3
INST = [0, 1, 2, 3, 4, 5, 0, 1, 2]


def _host(d):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _fe(crop, n_pts):
    from genpose_amd.preprocess import DepthToClouds
    return DepthToClouds(img_size=crop, n_pts=n_pts)


@functools.lru_cache(maxsize=None)
def _per_frame(crop, n_pts):
    """The yardstick, computed once: every frame through the per-frame launch, run RUN + f, slots SLOT_BASE + i -> host dicts."""
    return tuple(_host(_fe(crop, n_pts).device_clouds(*fr, SEED, RUN + f, slot_base=SLOT_BASE)) for f, fr in enumerate(_frames()))


@functools.lru_cache(maxsize=None)
def _batched(crop, n_pts):
    got = _fe(crop, n_pts).device_clouds_frames(list(_frames()), SEED, first_run=RUN, slot_base=SLOT_BASE)
    assert all(v.is_cuda for v in got.values())
    return _host(got)


def _assert_blocks_equal_the_per_frame_launches(got, crop, n_pts):
    want = _per_frame(crop, n_pts)
    assert got["points"].shape == (9, n_pts, 3) and got["points"].dtype == torch.float32
    assert got["count"].dtype == torch.int32 and got["depth_count"].dtype == torch.int32 and got["valid"].dtype == torch.uint8
    assert got["frame"].dtype == torch.int64 and got["frame"].tolist() == FRAME
    assert got["inst"].dtype == torch.int64 and got["inst"].tolist() == INST
    lo = 0
    for f, n_f in enumerate(N_F):
        for k in KEYS:
            assert want[f][k].shape[0] == n_f
            assert torch.equal(got[k][lo:lo + n_f], want[f][k]), (f, k)
        lo += n_f


@pytest.mark.parametrize("crop,n_pts", CONFIGS)
def test_every_frames_block_equals_the_per_frame_launch(crop, n_pts):
    fe, frames = _fe(crop, n_pts), list(_frames())
    got = _batched(crop, n_pts)
    _assert_blocks_equal_the_per_frame_launches(got, crop, n_pts)
    # one frame: the whole dict is device_clouds'
    one = _host(fe.device_clouds_frames(frames[:1], SEED, first_run=RUN, slot_base=SLOT_BASE))
    for k in KEYS:
        assert torch.equal(one[k], _per_frame(crop, n_pts)[0][k]), k
    assert one["frame"].tolist() == [0] * 6 and one["inst"].tolist() == list(range(6))
    # the same call with `out` of an earlier one: its tensors, written in place, the same bits
    first = fe.device_clouds_frames(frames, SEED, first_run=RUN, slot_base=SLOT_BASE)
    for v in first.values():
        v.fill_(1)
    again = fe.device_clouds_frames(frames, SEED, first_run=RUN, slot_base=SLOT_BASE, out=first)
    assert all(again[k] is first[k] for k in first) and sorted(again) == sorted(first)
    _assert_blocks_equal_the_per_frame_launches(_host(again), crop, n_pts)


def test_every_branch_of_the_draw_is_in_the_launches():
    """Crop 8: tiling (1 < c < n); crops 100 and 256: the walk (c > n); crop 256 with 1024 points: both in one launch; the empty mask and
    the depth hole (detections 4 and 5 of frame 0, and detection 0 of frame 2) in every launch - no branch is silently absent."""
    for (crop, n_pts), tile, walk in zip(CONFIGS, (True, False, False, True), (False, True, True, True)):
        got = _batched(crop, n_pts)
        cnt, dcnt, ok = got["count"].numpy(), got["depth_count"].numpy(), got["valid"].numpy().astype(bool)
        assert (ok == ((cnt > 1) & (dcnt > 1))).all()
        if tile:
            assert (ok & (cnt < n_pts)).any(), (crop, n_pts, cnt.tolist())
        if walk:
            assert (ok & (cnt > n_pts)).any(), (crop, n_pts, cnt.tolist())
        for i in (4, 5, 6):
            assert not ok[i] and cnt[i] == 0 and (got["points"][i] == 0).all(), (crop, n_pts, i)
        assert dcnt[4] > 1 and ok[[0, 2, 3, 7, 8]].all()


@pytest.mark.parametrize("crop,n_pts", [(100, 64), (256, 1024)])
def test_order_and_company_do_not_matter(crop, n_pts):
    fe, frames = _fe(crop, n_pts), list(_frames())
    base = _batched(crop, n_pts)
    # the frames in reverse order, every frame keeping its run
    rev = _host(fe.device_clouds_frames(frames[::-1], SEED, slot_base=SLOT_BASE, runs=[RUN + 2, RUN + 1, RUN]))
    assert rev["frame"].tolist() == [0] * 3 + [2] * 6 and rev["inst"].tolist() == [0, 1, 2, 0, 1, 2, 3, 4, 5]
    where = {(2 - f, i): k for k, (f, i) in enumerate(zip(rev["frame"].tolist(), rev["inst"].tolist()))}
    for k, (f, i) in enumerate(zip(FRAME, INST)):
        for name in KEYS:
            assert torch.equal(rev[name][where[(f, i)]], base[name][k]), (f, i, name)
    # two walked detections of frame 0 swap their slots: their rows move, nothing else does
    cnt = base["count"].numpy()
    a, b = [i for i in range(6) if cnt[i] > n_pts][:2]
    slots = [SLOT_BASE + i for i in INST]
    slots[a], slots[b] = slots[b], slots[a]
    sw = _host(fe.device_clouds_frames(frames, SEED, first_run=RUN, slots=slots))
    for name in ("count", "depth_count", "valid", "frame", "inst"):
        assert torch.equal(sw[name], base[name]), name
    for k in range(9):
        assert torch.equal(sw["points"][k], base["points"][k]) == (k not in (a, b)), k
    # ... to the rows the per-frame launch gives the detection under the other's slot
    d0, m0, r0 = frames[0]
    for k, other in ((a, b), (b, a)):
        alone = _host(fe.device_clouds(d0, m0[:, :, k:k + 1], r0[k:k + 1], SEED, RUN, slot_base=SLOT_BASE + other))
        assert torch.equal(sw["points"][k], alone["points"][0]), k


@pytest.mark.parametrize("crop,n_pts", [(100, 64), (256, 1024)])
def test_host_inputs_and_device_inputs_give_identical_outputs(crop, n_pts):
    fe, frames = _fe(crop, n_pts), list(_frames())
    base = _batched(crop, n_pts)
    depth = torch.from_numpy(np.stack([fr[0] for fr in frames]).view(np.int16)).cuda()  # [F,H,W] on the device: used as it is
    masks = [torch.from_numpy(frames[0][1].astype(np.uint8)).cuda(), torch.from_numpy(frames[1][1]).cuda(), torch.from_numpy(frames[2][1]).cuda()]  # (uint8 and bool)
    dev = [(depth[f], masks[f], frames[f][2]) for f in range(3)]
    got = _host(fe.device_clouds_frames(dev, SEED, first_run=RUN, slot_base=SLOT_BASE))
    for k in base:
        assert torch.equal(got[k], base[k]), k
    # device images that are NOT one block (gathered by device copies), in the other 16-bit dtype
    apart = [(torch.from_numpy(fr[0].copy()).cuda(), masks[f], fr[2]) for f, fr in enumerate(frames)]
    got = _host(fe.device_clouds_frames(apart, SEED, first_run=RUN, slot_base=SLOT_BASE))
    for k in base:
        assert torch.equal(got[k], base[k]), k
    # a ragged sequence of calls grows the staging and leaves the bits alone
    small = _host(fe.device_clouds_frames(frames[2:], SEED, first_run=RUN + 2, slot_base=SLOT_BASE))
    for k in KEYS:
        assert torch.equal(small[k], base[k][6:]), k
    got = _host(fe.device_clouds_frames(frames + frames[:1], SEED, first_run=RUN, slot_base=SLOT_BASE))
    for k in KEYS:
        assert torch.equal(got[k][:9], base[k]), k
    assert got["frame"].tolist() == FRAME + [3] * 6
    with pytest.raises(ValueError):
        fe.device_clouds_frames([dev[0], frames[2]], SEED)  # (host and device images mixed)


def _device_inputs(fe, frames, seed, first_run, slot_base):
    """launch_frames' seven input tensors for a list of host frames, on the host."""
    from genpose_amd.preprocess import frame_tables
    t = frame_tables(frames, fe.img, first_run=first_run, slot_base=slot_base)
    depth = torch.from_numpy(np.stack([fr[0] for fr in frames]).view(np.int16))
    masks = torch.from_numpy(np.concatenate([fr[1].astype(np.uint8).reshape(-1) for fr in frames]))
    assert masks.numel() == t["mask_bytes"]
    words = np.array([seed & 0xFFFFFFFF, seed >> 32, 0xDEAD, 0, 0xBEEF, 0, 0, 0], dtype=np.uint32).view(np.int32)  # (words 2 and 4 must not matter)
    return (depth, masks, torch.from_numpy(t["mask_off"]), torch.from_numpy(t["det"]), torch.from_numpy(t["draw"].view(np.int32)),
            torch.from_numpy(t["minv"]), torch.from_numpy(words))


def test_the_launch_is_capturable_and_replays_on_overwritten_buffers():
    """No synchronisation, no allocation, no host read in the launch: captured once on frame set A, replayed after every input buffer -
    depth, masks, the four tables and the seed - was overwritten with set B's (the same 9 detections split 3 + 6 instead of 6 + 3, so other
    mask offsets and another frame per detection), it gives B's eager result."""
    from genpose_amd import graphs
    fe = _fe(100, 64)
    f5, f9 = _first_frame()[:3], _second_frame()[:3]
    A = [f5, _restrict(f9, SECOND_CHANNELS)]
    B = [_restrict(f5, [1, 3, 4]), f9]
    bufs = [t.cuda() for t in _device_inputs(fe, A, SEED, RUN, 0)]
    out = fe.empty_outputs(9)
    cap = graphs.capture(lambda: fe.launch_frames(*bufs, out), warmup=True)
    first = {k: v.clone() for k, v in out.items()}
    want_a = fe.device_clouds_frames(A, SEED, first_run=RUN)
    for k in KEYS:
        assert torch.equal(first[k], want_a[k]), k
    for b, v in zip(bufs, _device_inputs(fe, B, SEED + 5, RUN + 2, 16)):
        assert b.shape == v.shape
        b.copy_(v)
    for v in out.values():
        v.fill_(1)
    got = cap.replay()
    want_b = fe.device_clouds_frames(B, SEED + 5, first_run=RUN + 2, slot_base=16)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(got[k], want_b[k]), k
    assert not torch.equal(want_b["points"], want_a["points"]) and want_b["frame"].tolist() == [0] * 3 + [1] * 6


def test_einval_writes_nothing_and_zero_detections_is_ok():
    from genpose_amd import _lib
    from genpose_amd._lib import ptr, stream_ptr
    L = _lib.lib()
    fe = _fe(13, 16)
    frames = list(_frames())
    depth, masks, mask_off, det, draw, minv, seed = (t.cuda() for t in _device_inputs(fe, frames, SEED, RUN, 0))
    F, H, W = depth.shape
    n, nb = det.shape[0], masks.numel()
    out = fe.empty_outputs(n)
    for v in out.values():
        v.fill_(7)
    k = (fe.fx, fe.fy, fe.cx, fe.cy)
    o = [ptr(out["points"]), ptr(out["count"]), ptr(out["depth_count"]), ptr(out["valid"])]
    tabs = [ptr(mask_off), ptr(det), ptr(draw), ptr(minv)]
    s = stream_ptr()

    def call(h=H, w=W, nframes=F, ndet=n, img=13, npts=16, d=ptr(depth), m=ptr(masks), mask_bytes=nb, tabs=tabs, seed_p=ptr(seed), o=o):
        return L.gp_roi_sample_frames(h, w, nframes, ndet, img, npts, d, m, mask_bytes, *tabs, *k, seed_p, *o, s)
    assert call(npts=0) == -1       # no output rows
    assert call(img=513) == -1      # the ballots would not fit
    assert call(img=0) == -1
    assert call(w=40000) == -1 and call(h=32768) == -1 and call(h=0) == -1 and call(w=0) == -1
    assert call(ndet=-1) == -1
    assert call(nframes=0) == -1 and call(nframes=-2) == -1  # detections of no frame
    assert call(mask_bytes=-1) == -1
    assert call(d=None) == -1 and call(m=None) == -1 and call(seed_p=None) == -1
    for j in range(4):
        bad = list(tabs)
        bad[j] = None
        assert call(tabs=bad) == -1
        bad = list(o)
        bad[j] = None
        assert call(o=bad) == -1
    assert call(ndet=0) == 0 and call(ndet=0, nframes=0) == 0
    torch.cuda.synchronize()
    assert all((v == 7).all() for v in out.values())
    # no detection at all: the empty dict, no launch
    empty = fe.device_clouds_frames([frames[1], frames[1]], SEED)
    assert empty["points"].shape == (0, 16, 3) and empty["valid"].shape == (0,) and empty["frame"].shape == (0,) and empty["inst"].dtype == torch.int64
    assert fe.device_clouds_frames([], SEED)["points"].shape == (0, 16, 3)


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


@pytest.mark.parametrize("batch_size", [256, 4])
def test_infer_depth_frames_is_infer_tensors_on_the_batched_front_ends_clouds(batch_size):
    """batch_size 4: the 9 detections span three network batches (4 + 4 + 1)."""
    from genpose_amd.preprocess import DepthToClouds
    from genpose_amd.runner import SingleFrameRunner
    cls = (_first_frame()[3], np.zeros(0, dtype=np.int32), _second_frame()[3][SECOND_CHANNELS])
    frames = [fr + (c,) for fr, c in zip(_frames(), cls)]
    sa, ea = _agents()
    runner = SingleFrameRunner(sa, ea, repeat_num=4, T0=0.55, batch_size=batch_size)
    torch.manual_seed(123)
    got = runner.infer_depth_frames(frames, seed=SEED, first_frame=RUN)
    assert all(torch.is_tensor(v) and v.is_cuda for v in got.values())
    fe = DepthToClouds().device_clouds_frames(list(_frames()), SEED, first_run=RUN)
    torch.manual_seed(123)
    want = runner.infer_tensors(fe["points"])
    valid = got["valid"].bool().cpu()
    assert valid.tolist() == [True, True, True, True, False, False, False, True, True]
    assert got["cat_id"].tolist() == [int(c) - 1 for c in np.concatenate(cls)]
    assert got["frame"].tolist() == FRAME and got["inst"].tolist() == INST
    for k in ("valid", "count", "depth_count"):
        assert torch.equal(got[k], fe[k]), k
    eye = torch.eye(4, dtype=got["average_sRT"].dtype)
    for k, w in want.items():
        g = got[k].cpu()
        assert g.shape[0] == 9 and torch.isfinite(g).all(), k
        assert torch.equal(g[valid], w.cpu()[valid]), k
        if k != "average_sRT":
            assert torch.equal(g, w.cpu()), k  # (only the aggregated pose is replaced)
    for i in (4, 5, 6):
        assert torch.equal(got["average_sRT"][i].cpu(), eye)
        assert (fe["points"][i] == 0).all()


def test_detect_keeps_what_call_keeps_and_its_clouds_are_the_seeded_rows():
    from genpose_amd.preprocess import DepthToClouds, seeded_ranks
    fe = DepthToClouds()
    frames = [_first_frame(), _second_frame()]
    keys = ["scene_1/0000", "scene_1/0001"]
    by_chunk = {}
    for chunk in (64, 1):
        results = [{"pred_class_ids": fr[3]} for fr in frames]
        d = by_chunk[chunk] = fe.detect([fr[:3] for fr in frames], keys, results, [fr[3] for fr in frames], seed=SEED, first_run=RUN, chunk=chunk)
        assert list(d) == keys
        for f, fr in enumerate(frames):
            e = d[keys[f]]
            ref = fe(*fr, rng=np.random.default_rng(0))
            assert e["result"] is results[f] and e["result"]["pred_RTs"].shape == (6, 4, 4)
            assert e["cat_id"] == ref["cat_id"] and e["valid_inst"] == ref["valid_inst"] and len(e["valid_pts"]) == len(ref["valid_inst"]) == 4
            pcl, cnt, _ = fe.full_clouds(*fr[:3])
            pcl, cnt = pcl.cpu(), cnt.cpu().numpy()
            for pts, i in zip(e["valid_pts"], e["valid_inst"]):
                assert pts.dtype == np.float32 and pts.shape == (1024, 3)
                want = pcl[i, torch.from_numpy(seeded_ranks(int(cnt[i]), 1024, SEED, RUN + f, i))]
                assert np.array_equal(pts, want.numpy()), (chunk, f, i)
    for key in keys:  # one launch over both frames and a launch per frame: the same clouds
        for p, q in zip(by_chunk[64][key]["valid_pts"], by_chunk[1][key]["valid_pts"]):
            assert np.array_equal(p, q)
