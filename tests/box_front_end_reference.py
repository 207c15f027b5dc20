"""numpy float32 restatements of the mask-free front end (include/genpose_hip.h: gp_cloud_extent, gp_box_sample): the object-frame
expression with one rounding per operation in the header's order, the WHOLE-IMAGE inside mask (no rectangle: that is the kernel's
accelerator, and agreeing with this is what shows the rectangle to be a superset), the full cloud in raster order, the sampled rows
through preprocess.seeded_ranks (the one host definition of the draw) and the order statistic through np.sort.  No device."""
import numpy as np

from genpose_amd.preprocess import seeded_ranks

F32 = np.float32


def object_frame(p, rt):
    """p [...,3] float32, rt [4,4] float32 -> q [...,3] float32: u = p - t, q_j = ((u_0 R[0][j]) + (u_1 R[1][j])) + (u_2 R[2][j])."""
    p, rt = np.asarray(p, dtype=F32), np.asarray(rt, dtype=F32)
    with np.errstate(all="ignore"):
        u = [p[..., i] - rt[i, 3] for i in range(3)]
        return np.stack([((u[0] * rt[0, j]) + (u[1] * rt[1, j])) + (u[2] * rt[2, j]) for j in range(3)], axis=-1).astype(F32)


def back_project(depth, K):
    """depth [H,W] uint16, K = (fx, fy, cx, cy) -> points [H,W,3] float32, gp_roi_to_cloud's expressions."""
    fx, fy, cx, cy = (F32(v) for v in K)
    H, W = depth.shape
    d = depth.astype(F32)
    sx, sy = np.arange(W, dtype=F32)[None, :], np.arange(H, dtype=F32)[:, None]
    x = ((sx - cx) * d / fx) / F32(1000)
    y = ((sy - cy) * d / fy) / F32(1000)
    return np.stack([x, y, d / F32(1000)], axis=-1).astype(F32)


def inflated(half, inflate, pad):
    with np.errstate(all="ignore"):
        return (np.asarray(half, dtype=F32) * F32(inflate) + F32(pad)).astype(F32)


def inside_mask(depth, K, rt, half, inflate, pad):
    """The inside pixels of the whole image [H,W] bool: depth > 0 and |q_j| <= hh_j for all j (a NaN compares false)."""
    hh = inflated(half, inflate, pad)
    q = object_frame(back_project(depth, K), rt)
    with np.errstate(all="ignore"):
        return (depth > 0) & np.all(np.abs(q) <= hh, axis=-1)


def full_cloud(depth, K, rt, half, inflate, pad):
    """The inside pixels' points in the image's raster order [c,3] float32."""
    return back_project(depth, K)[inside_mask(depth, K, rt, half, inflate, pad)]


def box_sample(depth, K, rt, half, inflate, pad, min_count, n_pts, seed, run, slot):
    """One object -> (points [n_pts,3] float32, count, valid) by the whole-image definition."""
    rt, hh = np.asarray(rt, dtype=F32), inflated(half, inflate, pad)
    cloud = full_cloud(depth, K, rt, half, inflate, pad)
    c = len(cloud)
    valid = bool(c >= max(2, int(min_count)) and np.isfinite(rt).all() and np.isfinite(hh).all() and (hh > 0).all())
    if not valid:
        return np.zeros((n_pts, 3), dtype=F32), c, 0
    return cloud[seeded_ranks(c, n_pts, seed, run, slot)], c, 1


def extent_reference(pts, rt, trim=0, sym=False):
    """pts [n,3], rt [4,4] -> half [3] float32: the (trim + 1)-th largest |q_j| (sym: of sqrt(q_0 q_0 + q_2 q_2) in columns 0 and 2)."""
    q = object_frame(pts, rt)
    a = np.abs(q)
    if sym:
        r = np.sqrt((q[:, 0] * q[:, 0]) + (q[:, 2] * q[:, 2])).astype(F32)
        a = np.stack([r, a[:, 1], r], axis=-1)
    return order_statistic(a, trim)


def order_statistic(a, trim):
    """a [n,3] -> the (trim + 1)-th largest of every column (duplicates count as often as they occur)."""
    a = np.asarray(a, dtype=F32)
    return np.sort(a, axis=0)[a.shape[0] - 1 - int(trim)].astype(F32)


def rotation(rng, about_z=None):
    """A float32 rotation matrix: seeded random (QR of a normal matrix, det +1), or a turn of about_z degrees about the optical axis."""
    if about_z is not None:
        c, s = np.cos(np.radians(about_z)), np.sin(np.radians(about_z))
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64).astype(F32)
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.astype(F32)


def pose(R, t):
    rt = np.eye(4, dtype=F32)
    rt[:3, :3], rt[:3, 3] = R, t
    return rt


# ------------------------------------------------------------------ the cases of tests/test_gpu_box_front_end.py (built once, device-free)
def images():
    """name -> depth [H,W] uint16: the synthetic frame and the hand-made images."""
    from genpose_amd import synth
    rng = np.random.default_rng(11)
    small = rng.integers(400, 600, size=(97, 131)).astype(np.uint16)
    small[rng.random(small.shape) < 0.05] = 0
    return {"frame": synth.golden_depth_frame(5)[0], "near": np.full((480, 640), 100, dtype=np.uint16), "plane": np.full((480, 640), 500, dtype=np.uint16),
            "small": small}


def centre_of(px, py, z, K):
    """The camera-frame point (float64 geometry, rounded once) that projects to pixel (px, py) at depth z metres."""
    fx, fy, cx, cy = (float(v) for v in K)
    return np.array([(px - cx) * z / fx, (py - cy) * z / fy, z], dtype=np.float64).astype(F32)


def cases(K):
    """[(name, image, rt [4,4], half [3], inflate, pad)]: boxes on objects 0-3 of the frame under seeded rotations (one a 45-degree turn
    about the optical axis) sized to tile and to walk at 64 and 1024 points, the c == n planes, the c <= 1 boxes and the rectangle's edge
    cases (module docstring of the GPU test)."""
    rng = np.random.default_rng(2024)
    fx, fy = float(K[0]), float(K[1])
    I3 = np.eye(3, dtype=F32)
    out = []
    add = lambda name, image, R, t, half, inflate=1.0, pad=0.0: out.append((name, image, pose(R, t), np.asarray(half, dtype=F32), inflate, pad))
    # the frame's objects: (row, col) centres and depths of synth.golden_depth_frame
    add("obj0_random", "frame", rotation(rng), centre_of(320, 240, 0.615, K), (0.05, 0.05, 0.05), 1.15, 0.01)
    add("obj0_turn45", "frame", rotation(rng, about_z=45.0), centre_of(320, 240, 0.615, K), (0.06, 0.03, 0.05))
    add("obj1_tiny", "frame", rotation(rng), centre_of(520, 100, 0.655, K), (0.02, 0.02, 0.02))
    add("obj2_medium", "frame", rotation(rng), centre_of(40, 30, 0.695, K), (0.015, 0.015, 0.015), 1.0, 0.001)
    add("obj3_border", "frame", rotation(rng), centre_of(610, 455, 0.735, K), (0.06, 0.06, 0.06))
    add("millimetre", "frame", rotation(rng), centre_of(320, 240, 0.630, K), (0.0002, 0.0002, 0.0002))  # (one pixel: the object's apex)
    add("hole", "frame", rotation(rng), centre_of(200, 200, 0.8, K), (0.015, 0.015, 0.015))
    add("behind", "frame", rotation(rng), np.array([0.0, 0.0, -0.5], dtype=F32), (0.1, 0.1, 0.1))
    add("off_image", "frame", rotation(rng), centre_of(-300, 100, 0.7, K), (0.03, 0.03, 0.03))
    add("corner_reaches_in", "frame", rotation(rng), centre_of(-20, 240, 1.07, K), (0.08, 0.08, 0.08))
    add("whole_frame", "frame", rotation(rng), np.array([0.0, 0.0, 1.0], dtype=F32), (5.0, 5.0, 5.0))
    add("near_large", "near", I3, np.array([0.0, 0.0, 0.1], dtype=F32), (0.03, 0.03, 0.02))
    add("near_plane_corner", "near", rotation(rng, about_z=20.0), np.array([0.0, 0.0, 0.1], dtype=F32), (0.03, 0.03, 0.06))
    for n in (64, 1024):  # c == n: an axis-aligned box over sqrt(n) x sqrt(n) pixels of a plane, its faces half a pixel from the next pixel
        s = int(round(n ** 0.5))
        add(f"plane_{n}", "plane", I3, centre_of(100 + (s - 1) / 2.0, 60 + (s - 1) / 2.0, 0.5, K), (0.5 * s * 0.5 / fx, 0.5 * s * 0.5 / fy, 0.01))
    add("small_image", "small", rotation(rng), centre_of(65, 48, 0.5, K), (0.05, 0.05, 0.05))
    return out
