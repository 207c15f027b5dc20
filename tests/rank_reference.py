"""Float64 numpy restatement of energy ranking and top-`sel` pose aggregation (include/genpose_hip.h, section D: gp_rank_aggregate(_rt);
the definition in the header comment of csrc/rank.hip), written from that definition and independently of genpose_amd.rotation and of the
oracle, and a seeded generator of candidate clusters.  A plain helper module (imported by the tests, not collected by pytest).

For one cloud with candidates i = 0..K-1, pose9 = two rotation columns a1, a2 and a translation t, energy [K,2]:
  order[:, c]   torch.sort(energy[:, c], descending=True, stable=True): column 0 ranks the rotations, column 1 the translations;
  sorted_pose   rank r holds the rotation columns of candidate order[r, 0] and the translation of candidate order[r, 1];
  R_i           Gram-Schmidt: b1 = a1 / max(|a1|, 1e-12), c = a2 - (b1 . a2) b1, b2 = c / max(|c|, 1e-12), columns b1, b2, b1 x b2;
  q_i           pytorch3d 0.7.2 matrix_to_quaternion: qa = sqrt(max(0, [1+m00+m11+m22, 1+m00-m11-m22, 1-m00+m11-m22, 1-m00-m11+m22])),
                the candidate row of the FIRST arg-max of qa, divided by 2 max(qa[best], 0.1); then q if w > 0 else -q (w == 0 gives -q);
  A             mean of q q^T over the top `sel` candidates of the rotation ranking;
  avg_pose[:4]  the eigenvector of A's largest eigenvalue (numpy.linalg.eigh), oriented the same way;
  avg_pose[4:]  the mean translation of the top `sel` candidates of the translation ranking.
The eigenvector is as well determined as the eigenvalue gap lambda_max - lambda_2 is wide: the reference returns the gap, and a test states
what it requires of its inputs before it compares."""
import numpy as np
import torch


def gram_schmidt(p6):
    """[...,6] -> [...,3,3] float64, columns b1, b2, b1 x b2.  The dot product and the norms run left to right, as the definition writes them."""
    p6 = np.asarray(p6, dtype=np.float64)
    a1, a2 = p6[..., 0:3], p6[..., 3:6]
    n1 = np.sqrt(a1[..., 0] * a1[..., 0] + a1[..., 1] * a1[..., 1] + a1[..., 2] * a1[..., 2])
    b1 = a1 / np.where(n1 > 1e-12, n1, 1e-12)[..., None]
    d = b1[..., 0] * a2[..., 0] + b1[..., 1] * a2[..., 1] + b1[..., 2] * a2[..., 2]
    c = a2 - d[..., None] * b1
    n2 = np.sqrt(c[..., 0] * c[..., 0] + c[..., 1] * c[..., 1] + c[..., 2] * c[..., 2])
    b2 = c / np.where(n2 > 1e-12, n2, 1e-12)[..., None]
    b3 = np.stack([b1[..., 1] * b2[..., 2] - b1[..., 2] * b2[..., 1], b1[..., 2] * b2[..., 0] - b1[..., 0] * b2[..., 2],
                   b1[..., 0] * b2[..., 1] - b1[..., 1] * b2[..., 0]], axis=-1)
    return np.stack([b1, b2, b3], axis=-1)


def pose9_to_rt(poses):
    """[...,9] -> [...,4,4] float64 homogeneous matrices."""
    poses = np.asarray(poses, dtype=np.float64)
    out = np.zeros(poses.shape[:-1] + (4, 4))
    out[..., :3, :3] = gram_schmidt(poses[..., :6])
    out[..., :3, 3] = poses[..., 6:9]
    out[..., 3, 3] = 1.0
    return out


def quat_branch(m):
    """[...,3,3] -> (qa [...,4] the four candidate magnitudes, best [...] the first arg-max)."""
    m = np.asarray(m, dtype=np.float64)
    m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
    qa = np.sqrt(np.maximum(0.0, np.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], axis=-1)))
    return qa, np.argmax(qa, axis=-1)  # numpy's arg-max is the first


def matrix_to_quat(m):
    """[...,3,3] -> [...,4] (w, x, y, z), not yet oriented."""
    m = np.asarray(m, dtype=np.float64)
    qa, best = quat_branch(m)
    m01, m02, m10, m12, m20, m21 = m[..., 0, 1], m[..., 0, 2], m[..., 1, 0], m[..., 1, 2], m[..., 2, 0], m[..., 2, 1]
    sq = qa * qa
    rows = np.stack([np.stack([sq[..., 0], m21 - m12, m02 - m20, m10 - m01], axis=-1),
                     np.stack([m21 - m12, sq[..., 1], m10 + m01, m02 + m20], axis=-1),
                     np.stack([m02 - m20, m10 + m01, sq[..., 2], m12 + m21], axis=-1),
                     np.stack([m10 - m01, m20 + m02, m21 + m12, sq[..., 3]], axis=-1)], axis=-2)  # [...,4 candidates,4]
    row = np.take_along_axis(rows, best[..., None, None], axis=-2)[..., 0, :]
    qb = np.take_along_axis(qa, best[..., None], axis=-1)
    return row / (2.0 * np.maximum(qb, 0.1))


def orient(q):
    """q where w > 0, else -q (so w == 0 gives -q)."""
    return np.where(q[..., 0:1] > 0, q, -q)


def stable_order(energy):
    """[B,K,2] float32 energies -> [B,K,2] int64: the candidate at each rank, per column."""
    e = torch.from_numpy(np.ascontiguousarray(energy, dtype=np.float32))
    return torch.sort(e, dim=1, descending=True, stable=True).indices.numpy()


def top_eigvec(A):
    """symmetric [4,4] -> (oriented eigenvector of the largest eigenvalue, lambda_max - lambda_2)"""
    w, v = np.linalg.eigh(A)
    return orient(v[:, -1]), float(w[-1] - w[-2])


def rank_aggregate(poses, energy, sel=0):
    """poses [B,K,9] (any float dtype: the values are widened to float64 as they are), energy [B,K,2] float32, sel = candidates to average
    (0: ranking only) -> dict(order [B,K,2] i64, sorted_energy [B,K,2] f32, sorted_poses [B,K,9] in the input's dtype, sorted_RTs
    [B,K,4,4] f64, avg_pose [B,7] f64 or None, gap [B] or None, quats [B,sel,4] the oriented quaternions that were averaged)."""
    poses = np.asarray(poses)
    energy = np.ascontiguousarray(energy, dtype=np.float32)
    B, K, _ = poses.shape
    order = stable_order(energy)
    bi = np.arange(B)[:, None]
    sorted_energy = np.stack([energy[bi, order[:, :, 0], 0], energy[bi, order[:, :, 1], 1]], axis=-1)
    sorted_poses = np.concatenate([poses[bi, order[:, :, 0], :6], poses[bi, order[:, :, 1], 6:]], axis=-1)
    out = {"order": order, "sorted_energy": sorted_energy, "sorted_poses": sorted_poses, "sorted_RTs": pose9_to_rt(sorted_poses),
           "avg_pose": None, "gap": None, "quats": None}
    if sel <= 0:
        return out
    assert sel <= K
    p64 = poses.astype(np.float64)
    q = orient(matrix_to_quat(gram_schmidt(p64[bi, order[:, :sel, 0], :6])))  # [B,sel,4]
    avg, gap = np.zeros((B, 7)), np.zeros(B)
    for b in range(B):
        A = (q[b][:, :, None] * q[b][:, None, :]).sum(axis=0) / sel
        avg[b, :4], gap[b] = top_eigvec(A)
    avg[:, 4:] = p64[bi, order[:, :sel, 1], 6:].mean(axis=1)
    out.update(avg_pose=avg, gap=gap, quats=q)
    return out


def quat_trans_to_rt(avg):
    """[B,7] (w, x, y, z, t) -> [B,4,4] float64: pytorch3d quaternion_to_matrix (two_s = 2 / |q|^2) and the translation."""
    avg = np.asarray(avg, dtype=np.float64)
    r, i, j, k = avg[:, 0], avg[:, 1], avg[:, 2], avg[:, 3]
    two_s = 2.0 / (avg[:, :4] * avg[:, :4]).sum(axis=1)
    out = np.zeros((avg.shape[0], 4, 4))
    out[:, :3, :3] = np.stack([1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                               two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                               two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)], axis=-1).reshape(-1, 3, 3)
    out[:, :3, 3] = avg[:, 4:]
    out[:, 3, 3] = 1.0
    return out


def jacobi_top_eigvec(A, max_sweeps=30):
    """Float64 transliteration of the device's 4x4 cyclic Jacobi (csrc/rank.hip: top_eigvec4) -> (eigenvector column of the largest diagonal
    entry, first such entry on a tie, NOT oriented; sweeps that rotated).  It is not the reference: the CPU tests use it to show that, on
    the inputs the GPU tests take, the method itself ends within rounding of eigh."""
    A = np.array(A, dtype=np.float64)
    V = np.eye(4)
    sweeps = 0
    for _ in range(max_sweeps):
        off = 0.0
        for p in range(4):
            for q in range(p + 1, 4):
                off += A[p, q] * A[p, q]
        if off < 1e-60:
            break
        sweeps += 1
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if abs(apq) < 1e-300:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                kp, kq = A[:, p].copy(), A[:, q].copy()
                A[:, p], A[:, q] = c * kp - s * kq, s * kp + c * kq
                pk, qk = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * pk - s * qk, s * pk + c * qk
                kp, kq = V[:, p].copy(), V[:, q].copy()
                V[:, p], V[:, q] = c * kp - s * kq, s * kp + c * kq
    best = 0
    for b in range(1, 4):
        if A[b, b] > A[best, best]:
            best = b
    return V[:, best].copy(), sweeps


# ---------------------------------------------------------------------------------------------- test inputs
def rodrigues(v):
    """rotation vectors [...,3] -> [...,3,3] (exp of the skew matrix)"""
    v = np.asarray(v, dtype=np.float64)
    th = np.sqrt((v * v).sum(axis=-1))
    k = v / np.maximum(th, 1e-300)[..., None]
    Kx = np.zeros(v.shape[:-1] + (3, 3))
    Kx[..., 0, 1], Kx[..., 0, 2], Kx[..., 1, 0], Kx[..., 1, 2], Kx[..., 2, 0], Kx[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th)[..., None, None] * Kx + (1.0 - np.cos(th))[..., None, None] * (Kx @ Kx)


def _axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return rodrigues(a / np.linalg.norm(a) * angle)


# The cluster centres: the identity (branch w), the three half turns (branches x, y, z, and w = 0 up to rounding: the orientation rule at its
# edge), 120 degrees about (1, 1, 1) (trace 0: all four candidates tie), a near-half turn about a generic axis (w = 5e-4: candidates on both
# sides of w = 0 once they spread), and one generic rotation.
CENTRES = {
    "identity": np.eye(3),
    "pi_x": np.diag([1.0, -1.0, -1.0]),
    "pi_y": np.diag([-1.0, 1.0, -1.0]),
    "pi_z": np.diag([-1.0, -1.0, 1.0]),
    "tie_111": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
    "near_pi": _axis_angle([0.3, -0.8, 0.5], np.pi - 1e-3),
    "generic": _axis_angle([-0.6, 0.2, 0.7], 1.1),
}
SPREADS = (0.0, 0.02, 0.3)


def make_cluster(seed, B, K, centre, spread):
    """-> poses [B,K,9] float64.  Candidate rotations R_i = exp(spread * n_i) R_c with n_i uniform in [-1, 1]^3; the 6-D pose is R_i's first two
    columns, each rescaled by a factor in 0.5..2, the second sheared by 0.3 of the first (Gram-Schmidt has to undo both); translations
    scatter 5 cm around a centre of a few decimetres."""
    rng = np.random.default_rng(seed)
    R = rodrigues(spread * rng.uniform(-1.0, 1.0, (B, K, 3))) @ np.asarray(centre, dtype=np.float64)
    s = rng.uniform(0.5, 2.0, (B, K, 2))
    poses = np.zeros((B, K, 9))
    poses[..., 0:3] = s[..., :1] * R[..., :, 0]
    poses[..., 3:6] = s[..., 1:] * (R[..., :, 1] + 0.3 * R[..., :, 0])
    poses[..., 6:9] = rng.standard_normal((B, 1, 3)) * 0.3 + rng.standard_normal((B, K, 3)) * 0.05
    return poses


def make_energy(seed, B, K, ties=False):
    """-> [B,K,2] float32: N(0, 1) draws, or (ties) integers 0..3 - hundreds of equal energies, the stable order decides."""
    rng = np.random.default_rng(seed)
    if ties:
        return rng.integers(0, 4, (B, K, 2)).astype(np.float32)
    return rng.standard_normal((B, K, 2)).astype(np.float32)


# (B, K, sel): one candidate; two; one short of / exactly / one past the wave's 64 lanes; fewer candidates than lanes (the runners' 50 at
# ratio 0.6); three passes with few selected; the largest earlier test size; then the LDS request 16 K + 16 + 32 sel at exactly 64 KB
# (1365), first above it (1366), the cap at the runners' ratio 0.6 and the cap with everything selected (98 320 bytes).
SIZES = [(1, 1, 1), (3, 2, 1), (2, 63, 63), (2, 64, 38), (2, 65, 65), (5, 50, 30), (2, 130, 7), (1, 200, 200), (1, 1365, 1365), (1, 1366, 1366),
         (1, 2048, 1228), (2, 2048, 2048)]
FAMILIES = [(name, spread) for name in CENTRES for spread in SPREADS]


def family_inputs(name, spread, B, K, ties=False):
    """The seeded inputs of one (family, size): poses [B,K,9] float64, energy [B,K,2] float32.  CPU and GPU tests take the same arrays."""
    seed = 100000 * list(CENTRES).index(name) + 10000 * SPREADS.index(spread) + 3 * K + B
    return make_cluster(seed, B, K, CENTRES[name], spread), make_energy(seed + 1, B, K, ties)


# Degenerate 6-D poses: the all-zero pose (both 1e-12 floors; R = 0, every quaternion candidate 1, q = (1/2, 0, 0, 0)), a zero first column
# (first floor; R keeps one column, the arg-max ties between two candidates), and a second column parallel to the first (second floor).  The
# parallel pair is axis-aligned so that the residue a2 - (b1 . a2) b1 is exactly zero in any arithmetic: with a generic pair it is rounding
# noise divided by 1e-12, and no reference value exists.
# The last three sit on either side of the floors, again with residues that are exact in any arithmetic: a second column 1e-9 off the
# first's direction is ABOVE the floor (b2 = (1, 0, 0)), 1e-15 off is below it (b2 = (1e-3, 0, 0)), and a first column of length 1e-15 is
# below the first floor (b1 = (0, 0, 1e-3)) - a floor moved past either value gives another matrix.
DEGENERATE = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                       [0.0, 0.0, 0.0, 0.3, -0.2, 0.9],
                       [0.0, 0.0, 2.0, 0.0, 0.0, -3.0],
                       [0.0, 0.0, 2.0, 1e-9, 0.0, -3.0],
                       [0.0, 0.0, 2.0, 1e-15, 0.0, -3.0],
                       [0.0, 0.0, 1e-15, 0.0, 1.0, 0.0]])


def degenerate_positions(K):
    return [1, 2, K // 2, K // 2 + 1, K - 2, K - 1]


def with_degenerate(poses, energy, inside):
    """Copies of (poses, energy) with the degenerate rotation blocks at degenerate_positions(K) of every cloud, their rotation energies
    below every other candidate's (they rank last: beyond `sel` when sel <= K - 6) or, `inside`, above (they rank first)."""
    poses, energy = poses.copy(), energy.copy()
    where, n = degenerate_positions(poses.shape[1]), len(DEGENERATE)
    poses[:, where, :6] = DEGENERATE
    lo, hi = float(energy[:, :, 0].min()), float(energy[:, :, 0].max())
    energy[:, where, 0] = np.float32(hi + 1.0) + np.arange(n, dtype=np.float32) if inside else np.float32(lo - 1.0) - np.arange(n, dtype=np.float32)
    return poses, energy
