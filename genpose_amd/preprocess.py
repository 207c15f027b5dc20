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


class DepthToClouds:
    RING = 4  # pinned blocks in rotation (device_clouds): the host rewrites one only after the copy issued four calls earlier has completed

    def __init__(self, intrinsics=REAL_INTRINSICS, n_pts=1024, img_size=256, device="cuda"):
        _lib.check_device()
        K = np.asarray(intrinsics, dtype=np.float32).reshape(-1)
        self.fx, self.fy, self.cx, self.cy = float(K[0]), float(K[4]), float(K[2]), float(K[5])
        self.n_pts, self.img, self.dev = n_pts, img_size, torch.device(device)
        self._staging = {}  # device_clouds: (H, W, n) -> static device inputs and their pinned blocks

    def full_clouds(self, depth, masks, rois):
        """All valid points of every detection, raster order of the crop: (pcl [n,img*img,3] f32, count [n], depth_count [n])."""
        depth = torch.as_tensor(np.ascontiguousarray(depth)) if not torch.is_tensor(depth) else depth
        if depth.dtype not in (torch.uint16, torch.int16):
            raise RuntimeError("depth must be uint16 millimetres")
        H, W = depth.shape
        masks = torch.as_tensor(np.ascontiguousarray(masks)) if not torch.is_tensor(masks) else masks
        n = masks.shape[2] if masks.dim() == 3 else 0
        if n != len(rois):
            raise ValueError(f"{n} masks for {len(rois)} rois")
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
        for name, shape, dtype in (("points", (n, self.n_pts, 3), torch.float32), ("count", (n,), torch.int32),
                                   ("depth_count", (n,), torch.int32), ("valid", (n,), torch.uint8)):
            if tuple(out[name].shape) != shape or out[name].dtype != dtype or out[name].device.type != "cuda":
                raise ValueError(f"out[{name!r}]: a device tensor {shape} {dtype}, got {tuple(out[name].shape)} {out[name].dtype} on {out[name].device}")
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
        from .graphs import PinnedBlock
        depth = torch.as_tensor(np.ascontiguousarray(depth)) if not torch.is_tensor(depth) else depth
        if depth.dtype not in (torch.uint16, torch.int16):
            raise RuntimeError("depth must be uint16 millimetres")
        H, W = depth.shape
        masks = torch.as_tensor(np.ascontiguousarray(masks)) if not torch.is_tensor(masks) else masks
        n = masks.shape[2] if masks.dim() == 3 else 0
        if n != len(rois):
            raise ValueError(f"{n} masks for {len(rois)} rois")
        if self.img > MAX_IMG_SEEDED:
            raise ValueError(f"device_clouds: img_size {self.img} > {MAX_IMG_SEEDED} (the kernel keeps the crop's ballots in LDS); use __call__")
        if out is None:
            out = self.empty_outputs(n)
        if n == 0:
            return out
        st = self._staging.get((H, W, n))
        if st is None:
            if len(self._staging) >= 8:
                self._staging.pop(next(iter(self._staging)))
            st = self._staging[(H, W, n)] = {
                "depth": torch.empty(H, W, dtype=torch.int16, device=self.dev), "masks": torch.empty(H, W, n, dtype=torch.uint8, device=self.dev),
                "minv": torch.empty(n, 6, dtype=torch.float64, device=self.dev), "seed": torch.zeros(8, dtype=torch.int32, device=self.dev),
                "pin_minv": [PinnedBlock((n, 6), torch.float64) for _ in range(self.RING)],
                "pin_seed": [PinnedBlock((8,), torch.int32) for _ in range(self.RING)], "ring": 0}
        slot = st["ring"] = (st["ring"] + 1) % self.RING
        # host images go up through pinned blocks like everything else: a non-blocking copy out of pageable memory (and, for bool masks, out
        # of the temporary of the dtype conversion, freed on return) leaves the runtime reading host memory the caller may already have freed
        if depth.device.type != "cuda":
            if "pin_depth" not in st:
                st["pin_depth"] = [PinnedBlock((H, W), torch.int16) for _ in range(self.RING)]
            depth16 = depth.view(torch.int16)
            depth = st["pin_depth"][slot].send(st["depth"], lambda h: h.copy_(depth16))
        if masks.device.type != "cuda":
            if "pin_masks" not in st:
                st["pin_masks"] = [PinnedBlock((H, W, n), torch.uint8) for _ in range(self.RING)]
            masks_h = masks
            masks = st["pin_masks"][slot].send(st["masks"], lambda h: h.copy_(masks_h))  # (bool -> uint8: 0 / 1, on the host)
        elif masks.dtype != torch.uint8:
            st["masks"].copy_(masks)
            masks = st["masks"]
        minv_h = np.stack([inverse_crop_map(get_bbox(r, H, W), self.img, H, W) for r in rois]).reshape(n, 6)
        seed = int(seed) % (1 << 64)
        words = np.array([seed & 0xFFFFFFFF, seed >> 32, int(run) & 0xFFFFFFFF, 0, int(slot_base) & 0xFFFFFFFF, 0, 0, 0], dtype=np.uint32)
        st["pin_minv"][slot].send(st["minv"], lambda h: h.copy_(torch.from_numpy(minv_h)))
        st["pin_seed"][slot].send(st["seed"], lambda h: h.copy_(torch.from_numpy(words.view(np.int32))))
        return self.launch_seeded(depth.contiguous(), masks.contiguous(), st["minv"], st["seed"], out)
