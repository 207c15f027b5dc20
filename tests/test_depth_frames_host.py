"""CPU (no GPU): the host side of the many-frame depth front end (gp_roi_sample_frames) - preprocess.frame_tables (the launch's tables
from a list of frames), preprocess.check_frame_tables (the refusal of entries the kernel would have to guard against),
preprocess.assemble_detect_result (host arrays -> the reference's detect_result dict) and the entry point's ABI."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, IMG = 48, 64, 16


def _frame(n, seed):
    rng = np.random.default_rng(seed)
    depth = rng.integers(0, 2000, (H, W)).astype(np.uint16)
    masks = rng.random((H, W, n)) < 0.5
    y1, x1 = rng.integers(0, H - 12, n), rng.integers(0, W - 12, n)
    rois = np.stack([y1, x1, y1 + rng.integers(2, 12, n), x1 + rng.integers(2, 12, n)], axis=1).astype(np.int32).reshape(n, 4)
    return depth, masks, rois


def _frames():
    return [_frame(6, 0), _frame(0, 1), _frame(3, 2)]


def test_tables_of_three_frames_with_6_0_and_3_detections():
    from genpose_amd.preprocess import frame_tables, get_bbox, inverse_crop_map
    frames = _frames()
    t = frame_tables(frames, IMG, first_run=7, slot_base=3)
    assert (t["H"], t["W"], t["nframes"], t["ndet"], t["mask_bytes"]) == (H, W, 3, 9, H * W * 9)
    assert t["mask_off"].dtype == np.int64 and t["mask_off"].tolist() == [0, H * W * 6, H * W * 6]  # the running sum of H * W * n_f
    assert t["det"].dtype == np.int32 and t["det"].shape == (9, 3)
    assert t["det"][:, 0].tolist() == [0] * 6 + [2] * 3
    assert t["det"][:, 1].tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 2]
    assert t["det"][:, 2].tolist() == [6] * 6 + [3] * 3
    assert t["frame"].dtype == np.int64 and t["frame"].tolist() == [0] * 6 + [2] * 3
    assert t["inst"].dtype == np.int64 and t["inst"].tolist() == [0, 1, 2, 3, 4, 5, 0, 1, 2]
    assert t["draw"].dtype == np.uint32 and t["draw"].shape == (9, 2)
    assert t["draw"][:, 0].tolist() == [7] * 6 + [9] * 3        # run = first_run + frame index
    assert t["draw"][:, 1].tolist() == [3, 4, 5, 6, 7, 8, 3, 4, 5]  # slot = slot_base + instance within its frame
    assert t["minv"].dtype == np.float64 and t["minv"].shape == (9, 6)
    k = 0
    for _, _, rois in frames:
        for r in rois:
            np.testing.assert_array_equal(t["minv"][k], inverse_crop_map(get_bbox(r, H, W), IMG, H, W).reshape(6))
            k += 1
    assert k == 9


@pytest.mark.parametrize("hw", [(480, 640), (48, 64), (1000, 300)])
def test_crop_maps_of_many_boxes_at_once_equal_the_per_detection_functions(hw):
    """inverse_crop_maps takes the array path from 16 boxes on: boxes that leave the image on every side, that are wider than the 440 cap,
    inverted ones and float ones (truncated towards zero) - equal bit for bit, and the table builder uses it."""
    from genpose_amd.preprocess import frame_tables, get_bbox, inverse_crop_map, inverse_crop_maps
    h, w = hw
    rng = np.random.default_rng(h)
    a = rng.integers(-60, max(h, w) + 60, (3000, 2))
    b = a + rng.integers(-5, 700, (3000, 2))
    rois = np.stack([a[:, 0], a[:, 1], b[:, 0], b[:, 1]], axis=1)
    for boxes in (rois, rois + rng.random(rois.shape) - 0.5, rois[:15], rois[:16]):
        want = np.stack([inverse_crop_map(get_bbox(r, h, w), 100, h, w).reshape(6) for r in boxes])
        got = inverse_crop_maps(boxes, 100, h, w)
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert inverse_crop_maps(np.zeros((0, 4)), 100, h, w).shape == (0, 6)
    frames = [(np.zeros((h, w), np.uint16), np.zeros((h, w, 10), bool), rois[10 * f:10 * f + 10].astype(np.int32)) for f in range(3)]
    np.testing.assert_array_equal(frame_tables(frames, 100)["minv"], inverse_crop_maps(rois[:30], 100, h, w))


def test_explicit_runs_and_slots_replace_the_defaults():
    from genpose_amd.preprocess import frame_tables
    frames = _frames()
    slots = [40, 41, 42, 43, 44, 45, 10, 12, 11]
    t = frame_tables(frames, IMG, first_run=7, slot_base=3, runs=[5, 1, 2 ** 32 + 8], slots=slots)
    assert t["draw"][:, 0].tolist() == [5] * 6 + [8] * 3  # (the low 32 bits travel)
    assert t["draw"][:, 1].tolist() == slots
    base = frame_tables(frames, IMG, first_run=7, slot_base=3)
    for k in ("mask_off", "det", "minv", "frame", "inst"):
        np.testing.assert_array_equal(t[k], base[k])
    with pytest.raises(ValueError):
        frame_tables(frames, IMG, runs=[1, 2])          # one run per frame
    with pytest.raises(ValueError):
        frame_tables(frames, IMG, slots=list(range(8)))  # one slot per detection


def test_no_frames_and_no_detections():
    from genpose_amd.preprocess import check_frame_tables, frame_tables
    t = check_frame_tables(frame_tables([], IMG))
    assert t["nframes"] == 0 and t["ndet"] == 0 and t["det"].shape == (0, 3) and t["mask_bytes"] == 0
    t = check_frame_tables(frame_tables([_frame(0, 3), _frame(0, 4)], IMG))
    assert t["nframes"] == 2 and t["ndet"] == 0 and t["mask_off"].tolist() == [0, 0] and t["minv"].shape == (0, 6)


def test_device_free_inputs_may_be_tensors():
    from genpose_amd.preprocess import frame_tables
    frames = _frames()
    as_t = [(torch.from_numpy(d.view(np.int16)), torch.from_numpy(m), r) for d, m, r in frames]
    a, b = frame_tables(frames, IMG), frame_tables(as_t, IMG)
    for k in ("mask_off", "det", "draw", "minv", "frame", "inst"):
        np.testing.assert_array_equal(a[k], b[k])


def test_every_stated_error_case_raises():
    from genpose_amd.preprocess import MAX_IMG_SEEDED, frame_tables
    f0, f1 = _frame(2, 0), _frame(1, 1)
    with pytest.raises(ValueError):  # frames of different H x W
        frame_tables([f0, (np.zeros((H + 1, W), np.uint16), np.zeros((H + 1, W, 1), bool), f1[2])], IMG)
    with pytest.raises(ValueError):  # a mask block whose channel count differs from len(rois)
        frame_tables([f0, (f1[0], np.zeros((H, W, 2), bool), f1[2])], IMG)
    with pytest.raises(ValueError):  # (and a block of another size than the depth image: mask_off assumes H * W * n_f)
        frame_tables([f0, (f1[0], np.zeros((H, W - 1, 1), bool), f1[2])], IMG)
    with pytest.raises(ValueError):
        frame_tables([f0], MAX_IMG_SEEDED + 1)
    frame_tables([f0], MAX_IMG_SEEDED)
    with pytest.raises(RuntimeError):  # depth that is not uint16, as device_clouds
        frame_tables([f0, (f1[0].astype(np.float32), f1[1], f1[2])], IMG)
    with pytest.raises(RuntimeError):
        frame_tables([(torch.zeros(H, W, dtype=torch.int32), f0[1], f0[2])], IMG)


def test_out_of_range_table_entries_are_refused_before_any_launch():
    """What the kernel guards against (such a detection gets no cloud there) never reaches it from the Python layer."""
    from genpose_amd.preprocess import check_frame_tables, frame_tables
    good = frame_tables(_frames(), IMG)
    assert check_frame_tables(good) is good

    def broken(**edit):
        t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in good.items()}
        for k, (idx, val) in edit.items():
            if idx is None:
                t[k] = val
            else:
                t[k][idx] = val
        return t
    for bad in (broken(det=((0, 0), 3)), broken(det=((0, 0), -1)),    # frame outside [0, nframes)
                broken(det=((7, 1), 3)), broken(det=((7, 1), -1)),    # channel outside [0, n_f)
                broken(det=((2, 2), 0)), broken(det=((2, 2), -4)),    # n_f <= 0
                broken(det=((8, 2), 4)),                              # a block that ends beyond the packed masks
                broken(mask_off=(2, H * W * 7)), broken(mask_off=(0, -1)),
                broken(mask_bytes=(None, H * W * 9 - 1)),
                broken(nframes=(None, 2)), broken(ndet=(None, 8))):
        with pytest.raises(ValueError):
            check_frame_tables(bad)


# ------------------------------------------------------------------ detect_result assembly
def _hand_made():
    keys = ["scene_1/0000", "scene_1/0001", "scene_2/0000"]
    class_ids = [np.array([1, 6, 3]), np.array([], dtype=np.int32), np.array([2, 5])]
    results = [{"gt_class_ids": np.array([1, 6]), "pred_class_ids": c, "pred_scores": np.ones(len(c))} for c in class_ids]
    frame = np.array([0, 0, 0, 2, 2])
    inst = np.array([0, 1, 2, 0, 1])
    valid = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
    points = np.arange(5 * 8 * 3, dtype=np.float32).reshape(5, 8, 3)
    return keys, results, class_ids, frame, inst, valid, points


def test_detect_result_keeps_exactly_the_valid_instances():
    from genpose_amd.preprocess import assemble_detect_result
    keys, results, class_ids, frame, inst, valid, points = _hand_made()
    d = assemble_detect_result(keys, results, class_ids, frame, inst, valid, points)
    assert list(d) == keys
    for f, key in enumerate(keys):
        assert sorted(d[key]) == ["cat_id", "result", "valid_inst", "valid_pts"]
        assert d[key]["result"] is results[f]
    e = d[keys[0]]
    assert e["valid_inst"] == [0, 2] and e["cat_id"] == [0, 2]  # cat_id = class_id - 1
    assert len(e["valid_pts"]) == 2
    np.testing.assert_array_equal(e["valid_pts"][0], points[0])
    np.testing.assert_array_equal(e["valid_pts"][1], points[2])
    assert all(p.dtype == np.float32 and p.shape == (8, 3) for p in e["valid_pts"])
    for key in keys[1:]:  # a frame without detections, and one with nothing kept: the key with empty lists
        assert d[key]["valid_pts"] == [] and d[key]["cat_id"] == [] and d[key]["valid_inst"] == []
    # the reference's placeholders: one identity / unit size per detection, kept or not
    assert results[0]["pred_RTs"].shape == (3, 4, 4) and results[1]["pred_RTs"].shape == (0, 4, 4) and results[2]["pred_scales"].shape == (2, 3)
    np.testing.assert_array_equal(results[0]["pred_RTs"][1], np.identity(4))
    with pytest.raises(ValueError):
        assemble_detect_result(keys[:2], results, class_ids, frame, inst, valid, points)
    with pytest.raises(ValueError):
        assemble_detect_result(keys, results, class_ids, frame, inst, valid[:4], points)


def test_detection_results_constructs_from_the_dict_and_batches_the_clouds():
    from genpose_amd import evaluation
    from genpose_amd.preprocess import assemble_detect_result
    keys, results, class_ids, frame, inst, valid, points = _hand_made()
    valid = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    d = assemble_detect_result(keys, results, class_ids, frame, inst, valid, points)
    K = 5
    store = evaluation.DetectionResults(d, K)
    assert results[0]["multi_hypothesis_pred_RTs"].shape == (3, K, 4, 4) and results[2]["energy"].shape == (2, K, 2)
    names = ("bottle", "bowl", "camera", "can", "laptop", "mug")
    got = {}
    for cat in store.by_category:
        for sl, pts in store.batches(cat, 2):
            assert pts.dtype == np.float32 and pts.shape == (sl.stop - sl.start, 8, 3)
            got[cat] = pts
    assert sorted(got) == sorted([names[0], names[2], names[1]])  # class ids 1, 3 (frame 0) and 2 (frame 2)
    np.testing.assert_array_equal(got[names[0]][0], points[0])
    np.testing.assert_array_equal(got[names[2]][0], points[2])
    np.testing.assert_array_equal(got[names[1]][0], points[3])
    store.write(names[1], slice(0, 1), np.full((1, K, 4, 4), 2.0), np.full((1, K, 2), 3.0))
    assert (results[2]["multi_hypothesis_pred_RTs"][0] == 2.0).all() and (results[2]["energy"][0] == 3.0).all()
    assert (results[2]["energy"][1] == 0.0).all()


# ------------------------------------------------------------------ ABI
def test_roi_sample_frames_is_declared_and_bound_with_the_headers_arity():
    import ctypes
    from genpose_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "genpose_hip.h")).read(), flags=re.S)
    args = [a.strip() for a in re.search(r"\bint\s+gp_roi_sample_frames\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")]
    sig = _lib.SIGNATURES["gp_roi_sample_frames"]
    assert len(sig) == len(args) == 23
    for a, c in zip(args, sig):
        want = ctypes.c_void_p if ("*" in a or a.startswith("gp_stream_t")) else {"int": ctypes.c_int, "float": ctypes.c_float,
                                                                                 "int64_t": ctypes.c_int64}[a.split()[0]]
        assert c is want, (a, c)
    # the sibling's arguments, in its order, around the frame tables
    sib = [a.strip() for a in re.search(r"\bint\s+gp_roi_sample_seeded\s*\(([^)]*)\)\s*;", hdr).group(1).split(",")]
    assert [a for a in args if a in sib] == [a for a in sib if a in args] and len([a for a in args if a in sib]) == len(sib) - 1  # (ninst -> ndet)
