"""Float64 numpy restatement of the mode-seeking aggregation (include/genpose_hip.h, section D: gp_mode_aggregate), written from the
definition and independently of genpose_amd.evaluation, and a seeded generator of bimodal test clouds.

Per cloud, the rotation (column 0) and the translation (column 1) independently:
  R_i, t_i, "finite" and the distances are consensus_reference's: dR_ij = 2 asin(min(1, |R_i - R_j|_F / (2 sqrt 2))), for a cloud symmetric
  about y 2 asin(min(1, |y_i - y_j| / 2)); dT_ij = |t_i - t_j|;
  w_j = the weight where it is > 0 and j is finite, else 0 (no weight: 1);  W = sum w_j;  kappa(d) = exp(-d^2 / (2 h^2));
  density_i = sum_j w_j kappa(d_ij) / W (j = i included; -inf for a non-finite i; 0 where W == 0);
  start = the lowest index with w_i > 0 of the highest density (-1 where W == 0);
  `iters` mean-shift steps from the start candidate with u_j = w_j kappa(d(centre, x_j)):  t <- sum u_j t_j / sum u_j;
  R <- quaternion_to_matrix of the top eigenvector (w >= 0) of sum u_j q_j q_j^T / sum u_j, q_j = pytorch3d's matrix_to_quaternion(R_j);
  symmetric: y <- normalize(sum u_j y_j), and with iters > 0 the rotation is the start candidate's turned by the minimal rotation that
  takes its y axis onto y;  the centre stays where sum u_j == 0 or the new axis is shorter than 1e-12;
  mass = sum_j w_j kappa(d(final centre, x_j)) / W.
W == 0: the identity rotation / the zero translation, mass 0.
"""
import numpy as np

import consensus_reference as cr

BW_ROT_DEG, BW_TRANS, ITERS = 10.0, 0.02, 8


def matrix_to_quat(R):
    """[...,3,3] -> [...,4] (w, x, y, z): pytorch3d v0.7.2 matrix_to_quaternion (the candidate of the largest component, divisor floored
    at 0.1), the sign as it comes."""
    R = np.asarray(R, dtype=np.float64)
    m = lambda i, j: R[..., i, j]
    with np.errstate(invalid="ignore"):
        qa = np.sqrt(np.maximum(0.0, np.stack([1 + m(0, 0) + m(1, 1) + m(2, 2), 1 + m(0, 0) - m(1, 1) - m(2, 2),
                                               1 - m(0, 0) + m(1, 1) - m(2, 2), 1 - m(0, 0) - m(1, 1) + m(2, 2)], axis=-1)))
    cand = np.stack([np.stack([qa[..., 0] ** 2, m(2, 1) - m(1, 2), m(0, 2) - m(2, 0), m(1, 0) - m(0, 1)], axis=-1),
                     np.stack([m(2, 1) - m(1, 2), qa[..., 1] ** 2, m(1, 0) + m(0, 1), m(0, 2) + m(2, 0)], axis=-1),
                     np.stack([m(0, 2) - m(2, 0), m(1, 0) + m(0, 1), qa[..., 2] ** 2, m(1, 2) + m(2, 1)], axis=-1),
                     np.stack([m(1, 0) - m(0, 1), m(2, 0) + m(0, 2), m(2, 1) + m(1, 2), qa[..., 3] ** 2], axis=-1)], axis=-2)
    cand = cand / (2.0 * np.maximum(qa, 0.1)[..., None])
    best = np.argmax(np.nan_to_num(qa, nan=-1.0), axis=-1)
    return np.take_along_axis(cand, best[..., None, None], axis=-2)[..., 0, :]


def quat_to_matrix(q):
    """[4] (w, x, y, z) -> [3,3]: pytorch3d quaternion_to_matrix"""
    r, i, j, k = q
    s = 2.0 / (q * q).sum()
    return np.array([[1 - s * (j * j + k * k), s * (i * j - k * r), s * (i * k + j * r)],
                     [s * (i * j + k * r), 1 - s * (i * i + k * k), s * (j * k - i * r)],
                     [s * (i * k - j * r), s * (j * k + i * r), 1 - s * (i * i + j * j)]])


def rot_dist(Rc, R, sym):
    """centre [3,3] (sym: only its y axis counts) against R [K,3,3] -> [K] radians"""
    with np.errstate(invalid="ignore", over="ignore"):
        if sym:
            e = R[:, :, 1] - Rc[:, 1]
            x = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]) / 2.0
        else:
            e = (R - Rc).reshape(-1, 9)
            ss = np.zeros(len(R))
            for c in range(9):
                ss = ss + e[:, c] * e[:, c]
            x = np.sqrt(ss) / cr.TWO_SQRT2
        return 2.0 * np.arcsin(np.minimum(1.0, x))


def trans_dist(tc, t):
    with np.errstate(invalid="ignore", over="ignore"):
        u = t - tc
        return np.sqrt((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2])


def kappa(d, h):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.exp(-(d * d) / (2.0 * h * h))


def minimal_turn(R, y):
    """R [3,3] turned by the minimal rotation that takes its y axis onto the unit vector y"""
    ys = R[:, 1]
    v, c1 = np.cross(ys, y), 1.0 + float(ys @ y)
    if c1 < 1e-12:
        x = R[:, 0]
        return (2.0 * np.outer(x, x) - np.eye(3)) @ R
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return (np.eye(3) + vx + (vx @ vx) / c1) @ R


def _weighted(w, values):
    """sum_j w_j values_j over the candidates with w_j > 0 (the others may hold NaN)"""
    on = w > 0
    return (w[on] * values[on].T).T.sum(axis=0)


def cloud_mode(pose, sym=False, weight=None, bw_rot_deg=BW_ROT_DEG, bw_trans=BW_TRANS, iters=ITERS):
    """One cloud: pose [K,9], weight [K,2] or None -> dict(density [K,2], start [2] int, R [3,3], t [3], mass [2]), float64."""
    pose = np.asarray(pose, dtype=np.float64)
    K = pose.shape[0]
    fin = np.isfinite(pose).all(axis=1)
    R, t = cr.gram_schmidt(pose[:, :6]), pose[:, 6:9]
    w = np.ones((K, 2)) if weight is None else np.asarray(weight, dtype=np.float64)
    w = np.where(fin[:, None] & (w > 0), w, 0.0)
    W = w.sum(axis=0)
    h = (np.deg2rad(bw_rot_deg), float(bw_trans))
    density = np.zeros((K, 2))
    for i in np.nonzero(fin)[0]:
        if W[0] > 0:
            density[i, 0] = _weighted(w[:, 0], kappa(rot_dist(R[i], R, sym), h[0])) / W[0]
        if W[1] > 0:
            density[i, 1] = _weighted(w[:, 1], kappa(trans_dist(t[i], t), h[1])) / W[1]
    density[~fin] = -np.inf
    start = np.array([int(np.argmax(np.where(w[:, c] > 0, density[:, c], -np.inf))) if W[c] > 0 else -1 for c in range(2)])
    mass = np.zeros(2)
    # translation
    tc = np.zeros(3)
    if W[1] > 0:
        tc = t[start[1]].copy()
        for _ in range(iters):
            u = w[:, 1] * np.nan_to_num(kappa(trans_dist(tc, t), h[1]))
            if u.sum() > 0:
                tc = _weighted(u, t) / u.sum()
        mass[1] = _weighted(w[:, 1], kappa(trans_dist(tc, t), h[1])) / W[1]
    # rotation
    Rc = np.eye(3)
    if W[0] > 0:
        Rc = R[start[0]].copy()
        q = matrix_to_quat(R)
        for _ in range(iters):
            u = w[:, 0] * np.nan_to_num(kappa(rot_dist(Rc, R, sym), h[0]))
            if not u.sum() > 0:
                continue
            if sym:
                y = _weighted(u, R[:, :, 1])
                n = np.sqrt(y @ y)
                if n >= 1e-12:
                    Rc = Rc.copy()
                    Rc[:, 1] = y / n  # (only the y axis of the centre is read)
            else:
                A = _weighted(u, q[:, :, None] * q[:, None, :]) / u.sum()
                v = np.linalg.eigh(A)[1][:, -1]
                Rc = quat_to_matrix(-v if v[0] < 0 else v)
        mass[0] = _weighted(w[:, 0], kappa(rot_dist(Rc, R, sym), h[0])) / W[0]
        if sym and iters > 0:
            Rc = minimal_turn(R[start[0]], Rc[:, 1])
    return {"density": density, "start": start, "R": Rc, "t": tc, "mass": mass}


def modes(poses, sym=None, weight=None, bw_rot_deg=BW_ROT_DEG, bw_trans=BW_TRANS, iters=ITERS):
    """poses [B,K,9], sym [B] or None, weight [B,K,2] or None -> dict(density [B,K,2], start [B,2], RT [B,4,4], mass [B,2])."""
    B = poses.shape[0]
    sym = np.zeros(B, dtype=bool) if sym is None else np.asarray(sym).astype(bool)
    per = [cloud_mode(poses[b], bool(sym[b]), None if weight is None else weight[b], bw_rot_deg, bw_trans, iters) for b in range(B)]
    RT = np.tile(np.eye(4), (B, 1, 1))
    for b, r in enumerate(per):
        RT[b, :3, :3], RT[b, :3, 3] = r["R"], r["t"]
    return {"density": np.stack([r["density"] for r in per]), "start": np.stack([r["start"] for r in per]), "RT": RT,
            "mass": np.stack([r["mass"] for r in per])}


def top_gap(density, weight=None):
    """[K,2] float64 densities (+ the [K,2] weights) -> [2]: relative difference of the two highest densities among the candidates that can
    start (finite, weight > 0); inf with fewer than two of them."""
    out = np.full(2, np.inf)
    for c in range(2):
        d = density[:, c]
        ok = np.isfinite(d) if weight is None else np.isfinite(d) & (np.asarray(weight)[:, c] > 0)
        d = np.sort(d[ok])
        if len(d) >= 2:
            out[c] = (d[-1] - d[-2]) / d[-1]
    return out


# ---------------------------------------------------------------------------------------------- test clouds
def make_bimodal(seed, B, m1, m2, turn_deg=90.0, shift=0.05):
    """-> poses [B,m1+m2,9] float32, (A_R [B,3,3], A_t [B,3]), (B_R, B_t), member [B,m1+m2] (0: around A, 1: around B).  Pose B is pose A
    turned by turn_deg about a random axis and shifted by `shift` in a random direction; the candidates carry make_clouds' inlier noise
    (rotation vectors of 2.9 deg per axis, 6 mm per axis) and column scaling, and are shuffled."""
    rng = np.random.default_rng(seed)
    K = m1 + m2
    A_R, A_t = cr._rand_rot(rng, B), rng.standard_normal((B, 3)) * 0.3
    ax = rng.standard_normal((B, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    B_R = A_R @ cr._rodrigues(ax * np.deg2rad(turn_deg))
    d = rng.standard_normal((B, 3))
    B_t = A_t + shift * d / np.linalg.norm(d, axis=1, keepdims=True)
    poses, member = np.zeros((B, K, 9)), np.zeros((B, K), dtype=np.int64)
    for b in range(B):
        member[b] = rng.permutation(np.r_[np.zeros(m1, dtype=np.int64), np.ones(m2, dtype=np.int64)])
        base_R = np.where(member[b][:, None, None] == 0, A_R[b], B_R[b])
        base_t = np.where(member[b][:, None] == 0, A_t[b], B_t[b])
        R = base_R @ cr._rodrigues(rng.standard_normal((K, 3)) * np.deg2rad(2.9))
        t = base_t + rng.standard_normal((K, 3)) * 0.006
        s = rng.uniform(0.8, 1.2, (K, 2))
        poses[b, :, 0:3] = s[:, :1] * R[:, :, 0]
        poses[b, :, 3:6] = s[:, 1:] * (R[:, :, 1] + 0.1 * rng.standard_normal((K, 1)) * R[:, :, 0])
        poses[b, :, 6:9] = t
    return poses.astype(np.float32), (A_R, A_t), (B_R, B_t), member
