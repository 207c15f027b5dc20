"""Depth image + Mask-RCNN detections -> per-instance 1024-point clouds on the GPU.

Replaces the per-frame body of detect_mrcnn_genpose (runners/evaluation_single.py:140-216): for every detection the square
crop window of get_bbox (utils/sgpa_utils.py:214-242), the 256 x 256 nearest-neighbour crops of depth / mask / pixel
coordinates (utils/datasets_utils.py:82-136), depth_to_pcl and sample_points.  Input formats are the reference's: `depth`
uint16 millimetres [H,W] (load_depth, sgpa_utils.py:194-211), `masks` bool [H,W,n], `rois` [n,4] (y1,x1,y2,x2), `class_ids` [n].
Output: the `valid_pts` / `cat_id` / `valid_inst` entries of the reference's per-image record (evaluation_single.py:241-253),
with the clouds left on the device for the pose agents.
"""
import numpy as np
import torch

from . import _lib
from ._lib import ptr, stream_ptr
from .graphs import UploadRing
from .lru import ShapeCache

REAL_INTRINSICS = np.array([[591.0125, 0, 322.525], [0, 590.16775, 244.11084], [0, 0, 1]], dtype=np.float32)   # evaluation_single.py:54
CAMERA_INTRINSICS = np.array([[577.5, 0, 319.5], [0, 577.5, 239.5], [0, 0, 1]], dtype=np.float32)            # evaluation_single.py:50


def get_bbox(bbox, img_h=480, img_w=640):
    """Square crop window (rmin, rmax, cmin, cmax): side = the next multiple of 40 above the box (<= 440), centred on the
    box and shifted back inside the image."""
    y1, x1, y2, x2 = [int(v) for v in bbox]
    half = int(min((max(y2 - y1, x2 - x1) // 40 + 1) * 40, 440) / 2)
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - half, cy + half, cx - half, cx + half
    if rmin < 0:
        rmin, rmax = 0, rmax - rmin
    if cmin < 0:
        cmin, cmax = 0, cmax - cmin
    if rmax > img_h:
        rmin, rmax = rmin - (rmax - img_h), img_h
    if cmax > img_w:
        cmin, cmax = cmin - (cmax - img_w), img_w
    return rmin, rmax, cmin, cmax


def inverse_crop_map(window, img_size, im_h, im_w):
    """Destination -> source map of crop_resize_by_warp_affine for a get_bbox window: get_affine_transform (rot = 0) maps the
    window centre to the crop centre with gain img_size / scale, scale = min(window side, max(H, W)); its inverse is
    source = dest * scale / img_size + (centre - scale / 2).  [2,3] float64."""
    rmin, rmax, cmin, cmax = window
    scale = float(min(max(rmax - rmin, cmax - cmin), max(im_h, im_w)))
    g = scale / float(img_size)
    cx, cy = 0.5 * (cmin + cmax), 0.5 * (rmin + rmax)
    return np.array([[g, 0.0, cx - 0.5 * scale], [0.0, g, cy - 0.5 * scale]], dtype=np.float64)


# ------------------------------------------------------------------ the seeded draw of the device front end (csrc/philox.h restated)
FEISTEL_ROUNDS = 8
PRIOR_STEP = (1 << 29) - 1   # gp_philox::PRIOR_STEP: the reserved step; the tracker's prior is its stream 0, this draw its stream 1
FRONT_END_STREAM = 1
MAX_IMG_SEEDED = 512         # gp_roi_sample_seeded keeps a crop's ballots in LDS


def _philox_word0(c0, c1, c2, c3, k0, k1):
    """Output word 0 of Philox4x32-10 (Salmon et al., SC'11); counter and key words: uint32 arrays of one shape."""
    m0, m1, sh, lo32 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(32), np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        for _ in range(10):
            p0, p1 = m0 * c0.astype(np.uint64), m1 * c2.astype(np.uint64)
            c0, c1, c2, c3 = ((p1 >> sh).astype(np.uint32) ^ c1 ^ k0, (p1 & lo32).astype(np.uint32),
                              (p0 >> sh).astype(np.uint32) ^ c3 ^ k1, (p0 & lo32).astype(np.uint32))
            k0, k1 = k0 + np.uint32(0x9E3779B9), k1 + np.uint32(0xBB67AE85)
    return c0


def seeded_ranks(count, n_pts, seed, run, slot):
    """Which valid pixels (ranks in raster order of the crop, as full_clouds orders them) a detection's n_pts output rows take under
    DepthToClouds.device_clouds: the host-side DEFINITION of gp_roi_sample_seeded's draw -> int64 [n_pts]; with arrays for seed, run or
    slot (broadcast to [S]) -> [S, n_pts], row s the draw of (seed[s], run[s], slot[s]).
        count < n_pts: k % count (sample_points' tiling)     count == n_pts: k     count > n_pts: sigma(k)
    sigma is a keyed bijection of [0, count), so the ranks are distinct without a sort: cycle walking over an alternating Feistel network
    on b = max(2, bit_length(count - 1)) bits, state x = a << hb | v with ha = b // 2, hb = b - ha, started at x = k.  One application is
    FEISTEL_ROUNDS rounds - even r: a ^= F(v, r) & (2^ha - 1), odd r: v ^= F(a, r) & (2^hb - 1) - and it is applied until x < count.
    F(u, r) = word 0 of the Philox4x32-10 block with key (seed lo, seed hi) and counter (u, (slot & 0xFFFFFF) | r << 24, run,
    PRIOR_STEP << 3 | 1 << 2 | 0): a function of (seed, run = frame index, slot = the detection's global slot) alone.
    NO random-number parity with numpy's permutation (what DepthToClouds.__call__ draws on the host) is claimed."""
    c, n = int(count), int(n_pts)
    if c < 1 or n < 1:
        raise ValueError(f"seeded_ranks(count={count}, n_pts={n_pts}): at least one valid pixel and one output row")
    scalar = np.ndim(seed) == 0 and np.ndim(run) == 0 and np.ndim(slot) == 0
    seed, run, slot = np.broadcast_arrays(np.atleast_1d(np.asarray(seed, dtype=np.uint64)), np.atleast_1d(np.asarray(run, dtype=np.uint64)),
                                          np.atleast_1d(np.asarray(slot, dtype=np.uint64)))
    S = seed.shape[0]
    k = np.arange(n, dtype=np.int64)
    if c <= n:
        x = np.broadcast_to(k % c if c < n else k, (S, n)).copy()
        return x[0] if scalar else x
    u32 = lambda v: (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    rep = lambda v: np.repeat(v, n)  # one entry per (draw, output row), draw-major
    k0, k1, c2, sl = rep(u32(seed)), rep(u32(seed >> np.uint64(32))), rep(u32(run)), rep(u32(slot) & np.uint32(0xFFFFFF))
    b = max(2, (c - 1).bit_length())
    ha = b // 2
    hb = b - ha
    ma, mb, sh = np.uint32((1 << ha) - 1), np.uint32((1 << hb) - 1), np.uint32(hb)
    c3 = np.uint32(PRIOR_STEP << 3 | FRONT_END_STREAM << 2)
    x = np.tile(k.astype(np.uint32), S)
    todo = np.arange(S * n)
    while todo.size:
        a, v = x[todo] >> sh, x[todo] & mb
        tk0, tk1, tc2, tsl, tc3 = k0[todo], k1[todo], c2[todo], sl[todo], np.full(todo.size, c3, dtype=np.uint32)
        for r in range(FEISTEL_ROUNDS):
            c1 = tsl | np.uint32(r << 24)
            if r % 2 == 0:
                a = a ^ (_philox_word0(v, c1, tc2, tc3, tk0, tk1) & ma)
            else:
                v = v ^ (_philox_word0(a, c1, tc2, tc3, tk0, tk1) & mb)
        x[todo] = a << sh | v
        todo = todo[x[todo] >= c]
    x = x.astype(np.int64).reshape(S, n)
    return x[0] if scalar else x


# ------------------------------------------------------------------ many frames in one launch (gp_roi_sample_frames): the host tables
def _depth_hw(depth, f):
    """(H, W) of a depth image - a host array or a tensor on any device - after device_clouds' dtype check; nothing is copied."""
    if isinstance(depth, torch.Tensor):
        ok = depth.dtype in (torch.uint16, torch.int16)
    else:
        depth = np.asarray(depth)
        ok = depth.dtype.kind in "ui" and depth.dtype.itemsize == 2
    if not ok:
        raise RuntimeError(f"frame {f}: depth must be uint16 millimetres")
    shape = tuple(depth.shape)
    if len(shape) != 2:
        raise ValueError(f"frame {f}: depth must be [H, W], got {shape}")
    return int(shape[0]), int(shape[1])


def inverse_crop_maps(rois, img_size, im_h, im_w):
    """inverse_crop_map(get_bbox(roi, im_h, im_w), img_size, im_h, im_w).reshape(6) for every row of rois [n,4] at once -> [n,6] float64,
    the same integer and float64 operations in the same order (equal bit for bit; tests/test_depth_frames_host.py): a batch of 258
    detections costs 1.5 ms through the per-detection functions."""
    if len(rois) < 16:  # (a frame or two: the per-detection functions are quicker than some forty array operations)
        return np.array([inverse_crop_map(get_bbox(b, im_h, im_w), img_size, im_h, im_w) for b in rois], dtype=np.float64).reshape(len(rois), 6)
    r = np.trunc(np.asarray(rois, dtype=np.float64)).astype(np.int64).reshape(-1, 4)  # (int(v): towards zero)
    y1, x1, y2, x2 = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    half = np.minimum((np.maximum(y2 - y1, x2 - x1) // 40 + 1) * 40, 440) // 2  # (a multiple of 40 halved: exact)
    cy, cx = (y1 + y2) // 2, (x1 + x2) // 2
    rmin, rmax, cmin, cmax = cy - half, cy + half, cx - half, cx + half
    rmax, rmin = np.where(rmin < 0, rmax - rmin, rmax), np.maximum(rmin, 0)
    cmax, cmin = np.where(cmin < 0, cmax - cmin, cmax), np.maximum(cmin, 0)
    rmin, rmax = np.where(rmax > im_h, rmin - (rmax - im_h), rmin), np.minimum(rmax, im_h)
    cmin, cmax = np.where(cmax > im_w, cmin - (cmax - im_w), cmin), np.minimum(cmax, im_w)
    scale = np.minimum(np.maximum(rmax - rmin, cmax - cmin), max(im_h, im_w)).astype(np.float64)
    out = np.zeros((len(r), 6), dtype=np.float64)
    out[:, 0] = out[:, 4] = scale / float(img_size)
    out[:, 2] = 0.5 * (cmin + cmax) - 0.5 * scale
    out[:, 5] = 0.5 * (rmin + rmax) - 0.5 * scale
    return out


def frame_tables(frames, img_size, first_run=0, slot_base=0, runs=None, slots=None):
    """The tables of gp_roi_sample_frames (include/genpose_hip.h) for a list of frames (depth [H,W] uint16, masks [H,W,n_f], rois [n_f,4],
    ...) of ONE image size; device-free: host arrays out, the images are only asked for their shapes and dtypes.  The n = sum n_f detections
    are in frame order, instance order inside a frame.  -> dict
        H, W, nframes, ndet, mask_bytes (= sum H * W * n_f: the packed mask buffer)
        mask_off [F] int64      byte offset of each frame's [H,W,n_f] uint8 block in that buffer (the running sum of H * W * n_f)
        det      [n,3] int32    frame index, mask channel inside the frame's block, n_f
        draw     [n,2] uint32   (run, slot) of the detection's draw: run = first_run + frame index, slot = slot_base + instance, so that
                                frame f's block of the launch equals device_clouds(*frame, seed, run=first_run + f, slot_base=slot_base);
                                runs [F] (one per FRAME) / slots [n] (one per DETECTION, in frame order) replace them
        minv     [n,6] float64  inverse_crop_map(get_bbox(roi)) per detection
        frame, inst [n] int64   which frame, which instance of it
    ValueError: frames of different H x W, a mask block that is not [H,W,len(rois)], img_size > MAX_IMG_SEEDED, runs / slots of the wrong
    length; RuntimeError: depth that is not uint16 (as device_clouds)."""
    if img_size > MAX_IMG_SEEDED:
        raise ValueError(f"frame_tables: img_size {img_size} > {MAX_IMG_SEEDED} (the kernel keeps the crop's ballots in LDS); use __call__")
    F = len(frames)
    H = W = total = 0
    # (plain lists, converted once at the end: array calls per frame were most of a 43-frame table's cost)
    mask_off, frame, inst, chans, rois = [], [], [], [], []
    for f, fr in enumerate(frames):
        h, w = _depth_hw(fr[0], f)
        if f == 0:
            H, W = h, w
        elif (h, w) != (H, W):
            raise ValueError(f"frame {f} is {h} x {w}, frame 0 is {H} x {W}: one launch serves one image size (group the frames by size)")
        mshape = tuple(fr[1].shape) if hasattr(fr[1], "shape") else np.shape(fr[1])
        nf = int(mshape[2]) if len(mshape) == 3 else 0
        if nf != len(fr[2]):
            raise ValueError(f"frame {f}: {nf} masks for {len(fr[2])} rois")
        if nf and tuple(mshape[:2]) != (H, W):
            raise ValueError(f"frame {f}: masks {mshape} for a {H} x {W} depth image")
        mask_off.append(total)
        total += H * W * nf
        if nf:
            frame += [f] * nf
            inst += range(nf)
            chans += [nf] * nf
            rois.append(np.asarray(fr[2]).reshape(nf, 4))
    n = len(frame)
    if runs is None:
        runs = [int(first_run) + f for f in range(F)]
    elif np.shape(runs) != (F,):
        raise ValueError(f"runs: one per frame ([{F}]), got {np.shape(runs)}")
    if slots is None:
        slots = [int(slot_base) + i for i in inst]
    elif np.shape(slots) != (n,):
        raise ValueError(f"slots: one per detection ([{n}]), got {np.shape(slots)}")
    draw = np.array([(int(runs[f]) & 0xFFFFFFFF, int(s) & 0xFFFFFFFF) for f, s in zip(frame, slots)], dtype=np.uint32).reshape(n, 2)
    return {"H": H, "W": W, "nframes": F, "ndet": n, "mask_bytes": total, "mask_off": np.array(mask_off, dtype=np.int64).reshape(F),
            "det": np.array([frame, inst, chans], dtype=np.int32).reshape(3, n).T.copy(), "draw": draw,
            "minv": inverse_crop_maps(np.concatenate(rois) if rois else np.zeros((0, 4)), img_size, H, W), "frame": np.array(frame, dtype=np.int64).reshape(n),
            "inst": np.array(inst, dtype=np.int64).reshape(n)}


def check_frame_tables(t):
    """Refuses, before any launch, tables whose entries the kernel would have to guard against (there such a detection silently gets no
    cloud): a frame outside [0, nframes), n_f <= 0, a channel outside [0, n_f), a block outside the packed mask buffer.  ValueError."""
    F, n, H, W = t["nframes"], t["ndet"], t["H"], t["W"]
    det, off = np.asarray(t["det"]).reshape(-1, 3), np.asarray(t["mask_off"]).reshape(-1)
    if len(det) != n or len(off) != F or np.asarray(t["draw"]).shape != (n, 2) or np.asarray(t["minv"]).shape != (n, 6):
        raise ValueError(f"frame tables: {n} detections of {F} frames, got det {det.shape}, mask_off {off.shape}")
    if n == 0:
        return t
    if F <= 0 or not (1 <= H <= 32767 and 1 <= W <= 32767):
        raise ValueError(f"frame tables: {n} detections of {F} frames of {H} x {W}")
    f, ch, nf = det[:, 0].astype(np.int64), det[:, 1].astype(np.int64), det[:, 2].astype(np.int64)
    bad = (f < 0) | (f >= F) | (nf <= 0) | (ch < 0) | (ch >= nf)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"frame tables: detection {i} names frame {f[i]} of {F}, channel {ch[i]} of {nf[i]}")
    o = off[f]
    bad = (o < 0) | (o + H * W * nf > int(t["mask_bytes"]))
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"frame tables: detection {i}'s mask block [{o[i]}, {o[i] + H * W * nf[i]}) leaves the {t['mask_bytes']} packed bytes")
    return t


def _as_tensor(x):
    """A host array as a (contiguous) tensor; a tensor, on any device, as it is."""
    return x if torch.is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x))


def _check_frame(depth, masks, rois):
    """One frame's inputs as tensors -> (depth, masks, n).  RuntimeError: depth that is not uint16; ValueError: not one mask per roi."""
    depth, masks = _as_tensor(depth), _as_tensor(masks)
    if depth.dtype not in (torch.uint16, torch.int16):
        raise RuntimeError("depth must be uint16 millimetres")
    n = masks.shape[2] if masks.dim() == 3 else 0
    if n != len(rois):
        raise ValueError(f"{n} masks for {len(rois)} rois")
    return depth, masks, n


def _check_out(out, fields):
    """The `out` dict of a launch_* method: every (name, shape, dtype) of `fields` a device tensor of that shape and dtype.  ValueError."""
    for name, shape, dtype in fields:
        if tuple(out[name].shape) != shape or out[name].dtype != dtype or out[name].device.type != "cuda":
            raise ValueError(f"out[{name!r}]: a device tensor {shape} {dtype}, got {tuple(out[name].shape)} {out[name].dtype} on {out[name].device}")


def _seed_fill(seed, run=0, slot_base=0):
    """The fill of a pinned int32 [8] block with the front ends' seed state: the low 32 bits of run and slot_base travel (word 5 stays 0)."""
    words = _lib.seed_words(seed, int(run) % (1 << 32), int(slot_base) & 0xFFFFFFFF)
    return lambda h: h.copy_(torch.from_numpy(words.view(np.int32)))


def check_box_inputs(depth, rt, half, frame_of, inflate, pad, min_count):
    """device_clouds_boxes' argument rules, device-free: -> (depth, rt, half, frame_of as tensors where they were arrays, F, H, W, n).
    ValueError / RuntimeError (depth that is not uint16, as device_clouds) before anything touches a device."""
    depth = _as_tensor(depth)
    if depth.dim() == 3:
        if depth.shape[0] < 1:
            raise ValueError("device_clouds_boxes: at least one frame")
        H, W = _depth_hw(depth[0], 0)
    else:
        H, W = _depth_hw(depth, 0)
    F = depth.shape[0] if depth.dim() == 3 else 1
    as_f32 = lambda t: (t if torch.is_tensor(t) else torch.as_tensor(np.ascontiguousarray(t, dtype=np.float32)))
    rt, half = as_f32(rt), as_f32(half)
    n = rt.shape[0] if rt.dim() == 3 else -1
    if n < 0 or tuple(rt.shape) != (n, 4, 4) or tuple(half.shape) != (n, 3) or rt.dtype != torch.float32 or half.dtype != torch.float32:
        raise ValueError(f"device_clouds_boxes: rt float32 [n,4,4] and half float32 [n,3], got {rt.dtype} {tuple(rt.shape)} and {half.dtype} {tuple(half.shape)}")
    if frame_of is not None:
        frame_of = _as_tensor(frame_of)
        if tuple(frame_of.shape) != (n,) or frame_of.dtype.is_floating_point:
            raise ValueError(f"device_clouds_boxes: frame_of holds one frame index per object ([{n}]), got {frame_of.dtype} {tuple(frame_of.shape)}")
    if not (np.isfinite(inflate) and inflate > 0 and np.isfinite(pad) and pad >= 0):
        raise ValueError(f"device_clouds_boxes: inflate finite > 0 and pad finite >= 0, got {inflate} and {pad}")
    if int(min_count) != min_count or min_count < 0:
        raise ValueError(f"device_clouds_boxes: min_count an integer >= 0, got {min_count}")
    return depth, rt, half, frame_of, F, H, W, n


def assemble_detect_result(keys, results, class_ids, frame, inst, valid, points):
    """Host arrays of a batched front end -> the reference's `detect_result` dict (evaluation_single.py:241-253):
    keys[f] -> {'result': results[f], 'valid_pts': [n_pts,3] float32 per kept instance, 'cat_id': class_id - 1 per kept instance,
    'valid_inst': the kept instance indices}, kept = valid != 0, in instance order.  frame / inst / valid [n], points [n,n_pts,3]: the
    detections in frame order; class_ids[f]: frame f's [n_f].  A frame with nothing kept has its key with empty lists.  results[f] gets the
    reference's placeholders pred_RTs (identities) and pred_scales (ones) where it has none (:162-163, :238-239)."""
    if not (len(keys) == len(results) == len(class_ids)):
        raise ValueError(f"{len(keys)} keys, {len(results)} results, {len(class_ids)} class_ids: one of each per frame")
    frame, inst, valid = np.asarray(frame).reshape(-1), np.asarray(inst).reshape(-1), np.asarray(valid).reshape(-1)
    points = np.asarray(points, dtype=np.float32)
    if not (len(frame) == len(inst) == len(valid) == len(points)):
        raise ValueError(f"frame {frame.shape}, inst {inst.shape}, valid {valid.shape}, points {points.shape}: one row per detection")
    out = {}
    for f, key in enumerate(keys):
        n_f = len(class_ids[f])
        res = results[f]
        res.setdefault("pred_RTs", np.tile(np.identity(4, dtype=float), (n_f, 1, 1)))
        res.setdefault("pred_scales", np.ones((n_f, 3), dtype=float))
        out[key] = {"result": res, "valid_pts": [], "cat_id": [], "valid_inst": []}
    for i in np.flatnonzero(valid != 0):
        f, k = int(frame[i]), int(inst[i])
        e = out[keys[f]]
        e["valid_pts"].append(points[i])
        e["cat_id"].append(int(class_ids[f][k]) - 1)
        e["valid_inst"].append(k)
    return out


def _as_one_block(ts, H, W):
    """Device images [H,W] that already are the consecutive slices of one contiguous tensor -> that [F,H,W] tensor, no copy; else None."""
    t0 = ts[0]
    step = H * W * t0.element_size()
    for f, t in enumerate(ts):
        if not (t.is_contiguous() and t.dtype == t0.dtype and t.device == t0.device and t.data_ptr() == t0.data_ptr() + f * step
                and t.untyped_storage().data_ptr() == t0.untyped_storage().data_ptr()):
            return None
    return t0.as_strided((len(ts), H, W), (H * W, W, 1))


class DepthToClouds:
    RING = 4  # pinned blocks in rotation (device_clouds): the host rewrites one only after the copy issued four calls earlier has completed
    FRAMES_RING = 2  # device_clouds_frames' blocks hold many frames each: two in rotation (a third call waits for the first one's copy)

    def __init__(self, intrinsics=REAL_INTRINSICS, n_pts=1024, img_size=256, device="cuda"):
        _lib.check_device()
        K = np.asarray(intrinsics, dtype=np.float32).reshape(-1)
        self.fx, self.fy, self.cx, self.cy = float(K[0]), float(K[4]), float(K[2]), float(K[5])
        self.n_pts, self.img, self.dev = n_pts, img_size, torch.device(device)
        self._staging = ShapeCache(8)  # device_clouds: (H, W, n), device_clouds_boxes: ("boxes", F, H, W) -> _stage's entry
        self._staging_frames = ShapeCache(4)  # device_clouds_frames: (H, W) -> the same, its buffers sized by capacity

    def _stage(self, cache, key, depth):
        """-> (the staging entry of `key`: device buffers by name (_reserve) and the ring their pinned blocks rotate in, that ring), the ring
        advanced: once per call of a front end."""
        st = cache.get(key)
        if st is None:
            st = cache[key] = {"ring": UploadRing(depth)}
        st["ring"].advance()
        return st, st["ring"]

    def _reserve(self, st, name, need, tail, dtype):
        """st[name]: a device buffer [capacity, *tail] with capacity >= need - sized by capacity, it only grows (by half at least), so a
        ragged sequence of batches does not reallocate on every call; its pinned blocks go with it."""
        cap = st[name].shape[0] if name in st else 0
        if cap < need:
            st["ring"].drop(name)  # (each block after the last copy out of it has completed)
            st[name] = torch.empty((max(need, cap + cap // 2),) + tail, dtype=dtype, device=self.dev)
        return st[name]

    def _out_fields(self, n, depth_count=True):
        """What _check_out holds an `out` dict to: empty_outputs(n)'s tensors, or (depth_count=False) empty_outputs_boxes(n)'s."""
        f = [("points", (n, self.n_pts, 3), torch.float32), ("count", (n,), torch.int32), ("depth_count", (n,), torch.int32),
             ("valid", (n,), torch.uint8)]
        return f if depth_count else f[:2] + f[3:]

    def full_clouds(self, depth, masks, rois):
        """All valid points of every detection, raster order of the crop: (pcl [n,img*img,3] f32, count [n], depth_count [n])."""
        depth, masks, n = _check_frame(depth, masks, rois)
        H, W = depth.shape
        depth = depth.to(self.dev).contiguous()
        masks = masks.to(self.dev).to(torch.uint8).contiguous()
        minv = np.stack([inverse_crop_map(get_bbox(r, H, W), self.img, H, W) for r in rois]).reshape(n, 6) if n else np.zeros((0, 6))
        minv = torch.from_numpy(minv).to(self.dev)
        cap = self.img * self.img
        pcl = torch.empty(n, cap, 3, device=self.dev)
        count = torch.zeros(n, dtype=torch.int32, device=self.dev)
        dcount = torch.zeros(n, dtype=torch.int32, device=self.dev)
        if n == 0:  # a frame without detections: the empty tensors have no address to hand to the entry point (NULL is GP_EINVAL there)
            return pcl, count, dcount
        _lib.call("gp_roi_to_cloud", H, W, n, self.img, ptr(depth), ptr(masks), ptr(minv), self.fx, self.fy, self.cx, self.cy, ptr(pcl),
                  ptr(count), ptr(dcount), stream_ptr())
        return pcl, count, dcount

    def __call__(self, depth, masks, rois, class_ids, rng=np.random):
        """-> dict(points [k,n_pts,3] device f32, cat_id [k] list, valid_inst [k] list) for the k instances the reference keeps."""
        pcl, count, dcount = self.full_clouds(depth, masks, rois)
        c, d = count.cpu().numpy(), dcount.cpu().numpy()
        keep = [i for i in range(len(c)) if d[i] > 1 and c[i] > 1]  # evaluation_single.py:201-208
        if not keep:
            return {"points": torch.zeros(0, self.n_pts, 3, device=self.dev), "cat_id": [], "valid_inst": []}
        ids = np.zeros((len(keep), self.n_pts), dtype=np.int32)
        for k, i in enumerate(keep):  # same draw order as the reference's per-instance np.random.permutation
            if c[i] > self.n_pts:
                ids[k] = rng.permutation(int(c[i]))[: self.n_pts]
        sel = torch.as_tensor(keep, device=self.dev)
        pcl_k, cnt_k = pcl[sel].contiguous(), count[sel].contiguous()
        ids_t = torch.from_numpy(ids).to(self.dev)
        out = torch.empty(len(keep), self.n_pts, 3, device=self.dev)
        _lib.call("gp_cloud_sample", len(keep), pcl.shape[1], self.n_pts, ptr(pcl_k), ptr(cnt_k), ptr(ids_t), ptr(out), stream_ptr())
        return {"points": out, "cat_id": [int(class_ids[i]) - 1 for i in keep], "valid_inst": keep}

    # ------------------------------------------------------------------ the device front end (ours): no host round trip
    def empty_outputs(self, n):
        """The output dict of device_clouds for n detections (pass it as `out` and the call allocates nothing)."""
        return {"points": torch.empty(n, self.n_pts, 3, device=self.dev), "count": torch.zeros(n, dtype=torch.int32, device=self.dev),
                "depth_count": torch.zeros(n, dtype=torch.int32, device=self.dev), "valid": torch.zeros(n, dtype=torch.uint8, device=self.dev)}

    def launch_seeded(self, depth, masks, minv, seed_state, out):
        """gp_roi_sample_seeded on device tensors alone: depth [H,W] uint16 / int16, masks [H,W,n] uint8, minv [n,6] f64, seed_state [8]
        int32 (csrc/philox.h's seed state; word 4 = the slot of detection 0), out as empty_outputs(n).  One launch, nothing else: capturable."""
        H, W = depth.shape
        n = masks.shape[2]
        _check_out(out, self._out_fields(n))
        if masks.dtype != torch.uint8 or depth.dtype not in (torch.uint16, torch.int16) or minv.dtype != torch.float64 or tuple(minv.shape) != (n, 6) \
                or seed_state.dtype != torch.int32 or seed_state.numel() != 8:
            raise ValueError("launch_seeded: depth uint16 [H,W], masks uint8 [H,W,n], minv float64 [n,6], seed_state int32 [8]")
        if n == 0:
            return out
        _lib.call("gp_roi_sample_seeded", H, W, n, self.img, self.n_pts, ptr(depth), ptr(masks), ptr(minv), self.fx, self.fy, self.cx, self.cy,
                  ptr(seed_state), ptr(out["points"]), ptr(out["count"]), ptr(out["depth_count"]), ptr(out["valid"]), stream_ptr())
        return out

    def device_clouds(self, depth, masks, rois, seed, run, slot_base=0, out=None):
        """Depth + masks -> dict(points [n,n_pts,3] f32, count [n] i32, depth_count [n] i32, valid [n] u8), ALL n detections, all on the
        device, in one launch (gp_roi_sample_seeded): no count is read back, nothing is drawn on the host, no [n,img*img,3] buffer exists.
        valid = count > 1 and depth_count > 1 - the detections __call__ keeps; the others' rows are zero.  Where a detection has more than
        n_pts valid pixels the kernel draws n_pts distinct ones itself, as a function of (seed, run = the frame index, slot_base + i) alone:
        points[i] == full_clouds(...)[0][i, seeded_ranks(count[i], n_pts, seed, run, slot_base + i)] bit for bit.  The draw claims NO
        random-number parity with __call__'s numpy permutation (nor with the reference's).
        minv (from rois, on the host as in full_clouds) and the seed words go up through pinned blocks in stream order; depth / masks may be
        host arrays (copied through pinned blocks into static device buffers) or device tensors (uint16 / uint8: used as they are).  out: empty_outputs(n) of an
        earlier call - then nothing is allocated."""
        depth, masks, n = _check_frame(depth, masks, rois)
        H, W = depth.shape
        if self.img > MAX_IMG_SEEDED:
            raise ValueError(f"device_clouds: img_size {self.img} > {MAX_IMG_SEEDED} (the kernel keeps the crop's ballots in LDS); use __call__")
        if out is None:
            out = self.empty_outputs(n)
        if n == 0:
            return out
        st, ring = self._stage(self._staging, (H, W, n), self.RING)
        # host images go up through pinned blocks like everything else: a non-blocking copy out of pageable memory (and, for bool masks, out
        # of the temporary of the dtype conversion, freed on return) leaves the runtime reading host memory the caller may already have freed
        if depth.device.type != "cuda":
            depth16 = depth.view(torch.int16)
            depth = ring.send("depth", self._reserve(st, "depth", H, (W,), torch.int16), lambda h: h.copy_(depth16))
        if masks.device.type != "cuda":
            masks_h = masks
            masks = ring.send("masks", self._reserve(st, "masks", H, (W, n), torch.uint8), lambda h: h.copy_(masks_h))  # (bool -> uint8: 0 / 1, on the host)
        elif masks.dtype != torch.uint8:
            masks = self._reserve(st, "masks", H, (W, n), torch.uint8).copy_(masks)
        minv_h = np.stack([inverse_crop_map(get_bbox(r, H, W), self.img, H, W) for r in rois]).reshape(n, 6)
        minv = ring.send("minv", self._reserve(st, "minv", n, (6,), torch.float64), lambda h: h.copy_(torch.from_numpy(minv_h)))
        seed_state = ring.send("seed", self._reserve(st, "seed", 8, (), torch.int32), _seed_fill(seed, run, slot_base))
        return self.launch_seeded(depth.contiguous(), masks.contiguous(), minv, seed_state, out)

    # ------------------------------------------------------------------ mask-free (ours): clouds from depth and oriented boxes
    def empty_outputs_boxes(self, n):
        """The output dict of device_clouds_boxes for n objects (pass it as `out` and the call allocates nothing)."""
        return {"points": torch.empty(n, self.n_pts, 3, device=self.dev), "count": torch.zeros(n, dtype=torch.int32, device=self.dev),
                "valid": torch.zeros(n, dtype=torch.uint8, device=self.dev)}

    def launch_boxes(self, depth, frame_of, rt, half, inflate, pad, min_count, seed_state, out):
        """gp_box_sample on device tensors alone: depth [F,H,W] uint16 / int16, frame_of [n] int32 or None (frame 0), rt [n,4,4] f32, half
        [n,3] f32, seed_state [8] int32 (word 2 = run, word 4 = the slot of object 0), out as empty_outputs_boxes(n).  One launch, nothing
        else: capturable after a first call outside the capture."""
        if depth.dim() != 3 or depth.dtype not in (torch.uint16, torch.int16):
            raise ValueError(f"launch_boxes: depth uint16 [F,H,W], got {depth.dtype} {tuple(depth.shape)}")
        F, H, W = depth.shape
        n = rt.shape[0]
        if tuple(rt.shape) != (n, 4, 4) or rt.dtype != torch.float32 or tuple(half.shape) != (n, 3) or half.dtype != torch.float32:
            raise ValueError(f"launch_boxes: rt float32 [n,4,4] and half float32 [n,3], got {rt.dtype} {tuple(rt.shape)} and {half.dtype} {tuple(half.shape)}")
        if frame_of is not None and (tuple(frame_of.shape) != (n,) or frame_of.dtype != torch.int32):
            raise ValueError(f"launch_boxes: frame_of int32 [{n}], got {frame_of.dtype} {tuple(frame_of.shape)}")
        if seed_state.dtype != torch.int32 or seed_state.numel() != 8:
            raise ValueError("launch_boxes: seed_state int32 [8]")
        if not (1 <= H <= 32767 and 1 <= W <= 32767 and F >= 1):
            raise ValueError(f"launch_boxes: {F} frames of {H} x {W}; at least one, sides in 1..32767")
        if not (np.isfinite(inflate) and inflate > 0 and np.isfinite(pad) and pad >= 0):
            raise ValueError(f"launch_boxes: inflate finite > 0 and pad finite >= 0, got {inflate} and {pad}")
        if int(min_count) != min_count or min_count < 0:
            raise ValueError(f"launch_boxes: min_count an integer >= 0, got {min_count}")
        _check_out(out, self._out_fields(n, depth_count=False))
        if any(t is not None and t.device.type != "cuda" for t in (depth, frame_of, rt, half, seed_state)):
            raise ValueError("launch_boxes: device tensors only")
        if n == 0:
            return out
        _lib.call("gp_box_sample", H, W, F, n, self.n_pts, ptr(depth), ptr(frame_of), ptr(rt), ptr(half), float(inflate), float(pad), int(min_count),
                  self.fx, self.fy, self.cx, self.cy, ptr(seed_state), None, ptr(out["points"]), ptr(out["count"]), ptr(out["valid"]), stream_ptr())
        return out

    def device_clouds_boxes(self, depth, rt, half, seed, run=0, *, frame_of=None, inflate=1.15, pad=0.01, min_count=2, slot_base=0, out=None):
        """Depth + one oriented box per object -> dict(points [n,n_pts,3] f32, count [n] i32, valid [n] u8) on the device, one launch
        (gp_box_sample), NO mask and nothing read back: what a tracker that already holds the objects' poses needs in place of a
        segmentation.  Ours - the reference has no counterpart (its tracking loop reads ground-truth masks) and no parity is claimed; the
        clouds are the frame's NATIVE pixels, not the 256 x 256 crop-and-resize of device_clouds.
        rt [n,4,4] f32: object -> camera poses (average_sRT's layout); half [n,3] f32: half-extents in the object frame (reward.cloud_extent);
        object i's box is |q_j| <= half[i][j] * inflate + pad, q = R^T (p - t) in the float32 order of include/genpose_hip.h.  count = the
        pixels with depth whose point lies inside (-1: the box's pixel rectangle has more 64-pixel segments than gp_box_sample_max_segments);
        valid = count >= max(2, min_count) with finite rt and a box of positive size; the others' rows are zero.  More than n_pts inside:
        the n_pts rows are drawn as in device_clouds - points[i] == (the inside pixels in raster order)[seeded_ranks(count[i], n_pts, seed,
        run, slot_base + i)].
        depth: [H,W] or [F,H,W] uint16 millimetres, a host array (copied through a pinned block into a static device buffer) or a device
        tensor (used as it is); frame_of [n] (optional): each object's frame, default frame 0.  rt, half, frame_of: device tensors are used
        as they are, host arrays are uploaded.  out: empty_outputs_boxes(n) of an earlier call - then nothing is allocated."""
        depth, rt, half, frame_of, F, H, W, n = check_box_inputs(depth, rt, half, frame_of, inflate, pad, min_count)
        if out is None:
            out = self.empty_outputs_boxes(n)
        if n == 0:
            return out
        st, ring = self._stage(self._staging, ("boxes", F, H, W), self.RING)
        if depth.device.type != "cuda":
            depth16 = depth.view(torch.int16).reshape(F, H, W)
            depth = ring.send("depth", self._reserve(st, "depth", F, (H, W), torch.int16), lambda h: h.copy_(depth16))
        else:
            depth = depth.contiguous().view(F, H, W)
        rt, half = rt.to(self.dev).contiguous(), half.to(self.dev).contiguous()
        if frame_of is not None:
            frame_of = frame_of.to(device=self.dev, dtype=torch.int32).contiguous()
        seed_state = ring.send("seed", self._reserve(st, "seed", 8, (), torch.int32), _seed_fill(seed, run, slot_base))
        return self.launch_boxes(depth, frame_of, rt, half, inflate, pad, min_count, seed_state, out)

    # ------------------------------------------------------------------ many frames in one launch
    def empty_outputs_frames(self, n):
        """The output dict of device_clouds_frames for n detections: empty_outputs(n) plus frame and inst [n] int64."""
        out = self.empty_outputs(n)
        out["frame"], out["inst"] = torch.zeros(2, n, dtype=torch.int64, device=self.dev)  # (one block: one copy fills both)
        return out

    def launch_frames(self, depth, masks, mask_off, det, draw, minv, seed_state, out):
        """gp_roi_sample_frames on device tensors alone: depth [F,H,W] uint16 / int16, masks [bytes] uint8 (the frames' [H,W,n_f] blocks one
        after the other), mask_off [F] int64, det [n,3] int32, draw [n,2] int32 (the uint32 words), minv [n,6] float64 - frame_tables' arrays -
        seed_state [8] int32 (words 0, 1 alone are read), out as empty_outputs(n) (frame / inst, if present, are not touched).  One launch,
        nothing else: capturable.  The table ENTRIES are not looked at here (that would be a read-back; check_frame_tables does it on the
        host): the kernel gives an out-of-range entry no cloud."""
        if depth.dim() != 3 or det.dim() != 2:
            raise ValueError("launch_frames: depth [F,H,W], det [n,3]")
        F, H, W = depth.shape
        n = det.shape[0]
        _check_out(out, self._out_fields(n))
        if depth.dtype not in (torch.uint16, torch.int16) or masks.dtype != torch.uint8 or masks.dim() != 1 or mask_off.dtype != torch.int64 \
                or tuple(mask_off.shape) != (F,) or det.dtype != torch.int32 or tuple(det.shape) != (n, 3) or draw.dtype != torch.int32 \
                or tuple(draw.shape) != (n, 2) or minv.dtype != torch.float64 or tuple(minv.shape) != (n, 6) or seed_state.dtype != torch.int32 \
                or seed_state.numel() != 8:
            raise ValueError("launch_frames: depth uint16 [F,H,W], masks uint8 [bytes], mask_off int64 [F], det int32 [n,3], draw int32 [n,2], "
                             "minv float64 [n,6], seed_state int32 [8]")
        if any(t.device.type != "cuda" for t in (depth, masks, mask_off, det, draw, minv, seed_state)):
            raise ValueError("launch_frames: device tensors only")
        if n == 0:
            return out
        _lib.call("gp_roi_sample_frames", H, W, F, n, self.img, self.n_pts, ptr(depth), ptr(masks), masks.numel(), ptr(mask_off), ptr(det), ptr(draw),
                  ptr(minv), self.fx, self.fy, self.cx, self.cy, ptr(seed_state), ptr(out["points"]), ptr(out["count"]), ptr(out["depth_count"]),
                  ptr(out["valid"]), stream_ptr())
        return out

    def _clouds_frames(self, frames, seed, first_run, slot_base, runs, slots, out):
        """device_clouds_frames -> (its dict, the host tables)."""
        frames = [tuple(fr[:3]) for fr in frames]
        t = check_frame_tables(frame_tables(frames, self.img, first_run, slot_base, runs, slots))
        F, n, H, W = t["nframes"], t["ndet"], t["H"], t["W"]
        if out is None:
            out = self.empty_outputs_frames(n)
        if n == 0:
            return out, t
        st, ring = self._stage(self._staging_frames, (H, W), self.FRAMES_RING)
        # ---- depth: device images that are one block already are used as they are; others are gathered by device copies; host images go up
        # through one pinned block, the frames side by side
        depths = [_as_tensor(fr[0]) for fr in frames]
        on_dev = [d.device.type == "cuda" for d in depths]
        depth = _as_one_block(depths, H, W) if all(on_dev) else None
        if depth is None:
            buf = self._reserve(st, "depth", F, (H, W), torch.int16)
            i16 = [d.view(torch.int16) if d.dtype == torch.uint16 else d for d in depths]
            if all(on_dev):
                for f in range(F):
                    buf[f].copy_(i16[f])
            elif not any(on_dev):
                def fill_depth(h):
                    for f in range(F):
                        h[f].copy_(i16[f])
                ring.send("depth", buf, fill_depth, rows=F)
            else:
                raise ValueError("device_clouds_frames: the frames' depth images are all host arrays or all device tensors")
            depth = buf[:F]
        # ---- masks: packed at mask_off - on the host into one pinned block (bool -> 0 / 1 there), from the device by one copy per frame
        blocks = [(f, int(t["mask_off"][f]), _as_tensor(fr[1])) for f, fr in enumerate(frames) if len(fr[2])]
        on_dev = [m.device.type == "cuda" for _, _, m in blocks]
        nbytes = t["mask_bytes"]
        if len(blocks) == 1 and on_dev[0] and blocks[0][2].dtype == torch.uint8 and blocks[0][2].is_contiguous():
            masks = blocks[0][2].view(-1)  # (one frame's uint8 block on the device: as it is)
        else:
            buf = self._reserve(st, "masks", nbytes, (), torch.uint8)
            if all(on_dev):
                for f, off, m in blocks:
                    buf[off:off + m.numel()].view(m.shape).copy_(m)
            elif not any(on_dev):
                def fill_masks(h):
                    for f, off, m in blocks:
                        h[off:off + m.numel()].view(m.shape).copy_(m)
                ring.send("masks", buf, fill_masks, rows=nbytes)
            else:
                raise ValueError("device_clouds_frames: the frames' masks are all host arrays or all device tensors")
            masks = buf[:nbytes]
        # ---- the tables and the seed: ONE pinned block, one copy - int64 mask_off [F] | float64 minv [n,6] | int64 frame, inst [2,n] |
        # int32 det [n,3] | uint32 draw [n,2] | the 8 seed words (run and slot words unused: they come from draw)
        parts = [("mask_off", t["mask_off"]), ("minv", t["minv"]), ("fi", np.stack([t["frame"], t["inst"]])), ("det", t["det"]),
                 ("draw", t["draw"]), ("seed", _lib.seed_words(seed))]
        total = sum(a.nbytes for _, a in parts)
        buf = self._reserve(st, "tables", total, (), torch.uint8)

        def fill_tables(h):
            hn, o = h.numpy(), 0
            for _, a in parts:
                hn[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
                o += a.nbytes
        ring.send("tables", buf, fill_tables, rows=total)
        as_torch = {"int64": torch.int64, "float64": torch.float64, "int32": torch.int32, "uint32": torch.int32}
        dev, o = {}, 0
        for name, a in parts:  # (8-byte entries first: every view starts at a multiple of its item size)
            dev[name] = buf[o:o + a.nbytes].view(as_torch[a.dtype.name]).view(a.shape)
            o += a.nbytes
        self.launch_frames(depth, masks, dev["mask_off"], dev["det"], dev["draw"], dev["minv"], dev["seed"], out)
        # (the staging is the next call's: the indices leave it - in one copy where the two tensors are empty_outputs_frames' one block)
        fr_o, in_o = out.get("frame"), out.get("inst")
        if fr_o is None or in_o is None:
            out["frame"], out["inst"] = dev["fi"].clone()
        elif fr_o.is_contiguous() and in_o.is_contiguous() and in_o.data_ptr() == fr_o.data_ptr() + 8 * n \
                and in_o.untyped_storage().data_ptr() == fr_o.untyped_storage().data_ptr():
            fr_o.as_strided((2, n), (n, 1)).copy_(dev["fi"])
        else:
            fr_o.copy_(dev["fi"][0])
            in_o.copy_(dev["fi"][1])
        return out, t

    def device_clouds_frames(self, frames, seed, first_run=0, slot_base=0, runs=None, slots=None, out=None):
        """device_clouds over MANY frames in ONE launch (gp_roi_sample_frames).  frames: a sequence of (depth [H,W] uint16, masks [H,W,n_f],
        rois [n_f,4]) of one image size (this object's intrinsics and crop size serve them all; n_f may be 0).  -> device_clouds' dict over
        all n = sum n_f detections in frame order - points [n,n_pts,3], count, depth_count, valid [n] - plus frame and inst [n] int64 (which
        frame, which instance of it), all on the device, nothing read back.  Detection (f, i) draws as (seed, run = first_run + f,
        slot = slot_base + i): frame f's block equals device_clouds(*frames[f], seed, run=first_run + f, slot_base=slot_base) bit for bit,
        whatever shares the launch and in whatever order; runs [F] / slots [n] replace the defaults (frame_tables).
        Host depth, masks and the tables go up through pinned blocks in stream order (three copies for the whole batch); device depth images
        that are consecutive slices of one [F,H,W] tensor are used as they are, others and per-frame device masks are gathered by device
        copies.  The staging is sized by capacity and only grows.  out: empty_outputs_frames(n) of an earlier call - then nothing is
        allocated for the outputs.  No detection at all: the empty dict, no launch."""
        return self._clouds_frames(frames, seed, first_run, slot_base, runs, slots, out)[0]

    def detect(self, frames, keys, results, class_ids, seed=0, first_run=0, chunk=64):
        """The reference's `detect_result` dict (what detect_mrcnn_genpose pickles, evaluation_single.py:241-253: key -> {'result',
        'valid_pts', 'cat_id', 'valid_inst'}) for a list of frames (depth, masks, rois), built from batched launches of at most `chunk`
        frames with ONE read-back per chunk (the clouds and their valid flags in one copy).  keys[f], results[f] (the per-image record
        carried along as 'result'), class_ids[f] [n_f] belong to frames[f]; frame f draws as run first_run + f.  The kept instances are
        exactly those __call__ keeps; SingleFrameRunner.evaluate and evaluation.DetectionResults take the dict as it is."""
        if not (len(frames) == len(keys) == len(results) == len(class_ids)):
            raise ValueError(f"{len(frames)} frames, {len(keys)} keys, {len(results)} results, {len(class_ids)} class_ids: one of each per frame")
        if chunk < 1:
            raise ValueError(f"detect(chunk={chunk}): at least one frame per launch")
        out = {}
        for c0 in range(0, len(frames), chunk):
            sl = slice(c0, c0 + chunk)
            fe, t = self._clouds_frames(frames[sl], seed, first_run + c0, 0, None, None, None)
            n = t["ndet"]
            # (valid travels as one more column of the float rows: one device -> host copy, one synchronisation per chunk)
            both = torch.cat([fe["points"].reshape(n, -1), fe["valid"].float().unsqueeze(1)], dim=1).cpu().numpy() if n else np.zeros((0, 3 * self.n_pts + 1), np.float32)
            out.update(assemble_detect_result(keys[sl], results[sl], class_ids[sl], t["frame"], t["inst"], both[:, -1],
                                              both[:, :-1].reshape(n, self.n_pts, 3)))
        return out
