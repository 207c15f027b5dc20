"""CPU (no GPU): the float64 reference of ranking and aggregation (tests/rank_reference.py) before the device is held to it
(tests/test_gpu_rank_aggregate.py).  It reproduces fixture G8 at the tolerances the device's golden test uses, agrees with
genpose_amd.rotation's formulas evaluated in float64 on the input families of the GPU tests, and those inputs have the properties the GPU
tests' bounds assume: a wide eigenvalue gap, all four quaternion branches reached, and a Jacobi iteration (the device's loop, transliterated)
that ends within rounding of eigh."""
import numpy as np
import pytest
import torch

import rank_reference as rr

# Two float64 evaluations of one formula differ by a few ulp per step; an eigenvector of a symmetric matrix computed by two backward-stable
# methods differs by about (n eps / gap) each - with n = 4, eps = 2.2e-16 and the gap >= 0.5 asserted below, 2 * 4 * 2.2e-16 / 0.5 = 3.6e-15.
EIG_ATOL = 4e-15
F64_ATOL = 1e-12  # the project's bound on float64 matrices (test_energy_rank_aggregate_golden: RT_sorted)


def _up_to_sign(a, b):
    return np.minimum(np.abs(a - b).max(axis=-1), np.abs(a + b).max(axis=-1))


def test_reference_reproduces_the_golden_fixture(golden):
    g = golden("g8_rank.npz")
    pred, energy = g["pred"], g["energy"]
    K = pred.shape[1]
    r = rr.rank_aggregate(pred, energy, sel=max(1, int(K * 0.6)))
    np.testing.assert_array_equal(r["sorted_poses"], g["sorted_pose"])
    np.testing.assert_array_equal(r["sorted_energy"], g["sorted_energy"])
    np.testing.assert_allclose(r["sorted_RTs"], g["RT_sorted"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(rr.quat_trans_to_rt(r["avg_pose"]), g["average_sRT"], rtol=0, atol=2e-6)
    assert r["order"].dtype == np.int64 and r["sorted_poses"].dtype == pred.dtype


def test_orientation_and_arg_max_rules():
    """w == 0 gives -q; the first arg-max wins a tie; each centre takes the branch it is there for."""
    q = np.array([[0.0, 1.0, 0.0, 0.0], [-0.0, 0.0, -1.0, 0.0], [1e-300, 0.0, 0.0, 1.0], [-0.5, 0.5, 0.5, 0.5]])
    np.testing.assert_array_equal(rr.orient(q), [[-0.0, -1.0, -0.0, -0.0], [0.0, -0.0, 1.0, -0.0], [1e-300, 0.0, 0.0, 1.0], [0.5, -0.5, -0.5, -0.5]])
    qa, best = rr.quat_branch(rr.CENTRES["tie_111"])
    assert qa.tolist() == [1.0, 1.0, 1.0, 1.0] and best == 0
    np.testing.assert_array_equal(rr.matrix_to_quat(rr.CENTRES["tie_111"]), [0.5, 0.5, 0.5, 0.5])
    np.testing.assert_array_equal(rr.matrix_to_quat(np.zeros((3, 3))), [0.5, 0.0, 0.0, 0.0])
    # (the four squared candidates sum to 4 whatever the matrix, so the largest is at least 1 and the 0.1 floor of the divisor binds for
    # no finite input: it is part of the definition, and the all-zero matrix above is as close as an input gets)
    for name, b in (("identity", 0), ("pi_x", 1), ("pi_y", 2), ("pi_z", 3)):
        assert rr.quat_branch(rr.CENTRES[name])[1] == b
    # the degenerate poses give finite rotations and quaternions
    R = rr.gram_schmidt(rr.DEGENERATE)
    assert np.isfinite(R).all() and np.isfinite(rr.matrix_to_quat(R)).all()
    np.testing.assert_array_equal(R[0], np.zeros((3, 3)))
    np.testing.assert_array_equal(R[2], [[0, 0, 0], [0, 0, 0], [1, 0, 0]])
    np.testing.assert_array_equal(R[3], [[0, 1, 0], [0, 0, 1], [1, 0, 0]])  # 1e-9 is above the floor: a rotation
    np.testing.assert_allclose(R[4], [[0, 1e-3, 0], [0, 0, 1e-3], [1, 0, 0]], rtol=1e-15, atol=0)  # 1e-15 is below it
    np.testing.assert_allclose(R[5], [[0, 0, -1e-3], [0, 1, 0], [1e-3, 0, 0]], rtol=1e-15, atol=0)


def test_stable_order_is_torch_sort():
    e = rr.make_energy(3, 2, 130, ties=True)
    o = rr.stable_order(e)
    for b in range(2):
        for c in range(2):
            assert sorted(o[b, :, c].tolist()) == list(range(130))
            v = e[b, o[b, :, c], c]
            assert (np.diff(v) <= 0).all()
            assert all(o[b, r, c] < o[b, r + 1, c] for r in range(129) if v[r] == v[r + 1])


@pytest.mark.parametrize("name", list(rr.CENTRES))
def test_reference_agrees_with_the_rotation_helpers_in_float64(name):
    from genpose_amd import rotation
    for spread in rr.SPREADS:
        for B, K, sel in ((3, 2, 1), (5, 50, 30), (2, 65, 65)):
            poses, energy = rr.family_inputs(name, spread, B, K)
            r = rr.rank_aggregate(poses, energy, sel)
            assert r["gap"].min() >= 0.5
            top = torch.from_numpy(poses[np.arange(B)[:, None], r["order"][:, :sel, 0], :6])
            R = rotation.get_rot_matrix(top)
            np.testing.assert_allclose(R.numpy(), rr.gram_schmidt(top.numpy()), rtol=0, atol=F64_ATOL)
            q = rotation.matrix_to_quaternion(R)
            # up to sign only where the two may have taken different candidates of a tie (their Gram-Schmidt results differ by rounding)
            qa = np.sort(rr.quat_branch(R.numpy())[0], axis=-1)
            clear = (qa[..., 3] - qa[..., 2]) > 1e-9
            mine = rr.matrix_to_quat(R.numpy())
            assert np.abs(q.numpy() - mine)[clear].max(initial=0.0) <= F64_ATOL
            assert _up_to_sign(q.numpy(), mine).max() <= F64_ATOL
            avg = rotation.average_quaternion_batch(q).numpy()
            ref = r["avg_pose"][:, :4]
            fixed = np.abs(ref[:, 0]) >= 1e-6  # below that the sign of w is rounding (an exact half turn has w ~ 6e-17)
            assert np.abs(avg - ref).max(axis=-1)[fixed].max(initial=0.0) <= EIG_ATOL
            assert _up_to_sign(avg, ref).max() <= EIG_ATOL
            np.testing.assert_allclose(np.linalg.norm(ref, axis=1), 1.0, rtol=0, atol=1e-15)


def test_the_gpu_test_inputs_have_the_properties_its_bounds_assume():
    """On every (family, size) the GPU tests take, and on the degenerate variants: the gap is at least 0.5 (0.868 without degenerate
    candidates), the clusters reach all four quaternion branches, and the device's Jacobi loop - transliterated to float64 numpy - ends
    within EIG_ATOL of eigh, after its own 30-sweep loop and already after 6 sweeps.  Where A has full rank (four or more distinct
    candidates) its convergence test stops it within 6 sweeps.  Where A is rank deficient (sel < 4, or spread 0: identical candidates,
    A = q q^T) the test `off < 1e-60` may never fire - the null space keeps a rounding residue of ~1e-17 that the rotations move about
    but do not shrink to 1e-30 - and the loop runs to its cap: observed on 11 of these matrices; it costs sweeps, not accuracy, which is
    what the assertion on the vector shows.  f32 poses: the same after rounding to float32."""
    branches, worst_gap, worst_sweeps, worst_vec, stalled = set(), 1.0, 0, 0.0, 0
    cases = [(n, s, B, K, sel, False, None) for (n, s) in rr.FAMILIES for (B, K, sel) in rr.SIZES]
    cases += [("generic", 0.02, 2, 2048, 2048, True, None)]
    cases += [(n, 0.02, 5, 50, 30, False, inside) for n in rr.CENTRES for inside in (False, True)]
    for name, spread, B, K, sel, ties, inside in cases:
        poses, energy = rr.family_inputs(name, spread, B, K, ties)
        if inside is not None:
            poses, energy = rr.with_degenerate(poses, energy, inside)
        for p in (poses, poses.astype(np.float32)):
            r = rr.rank_aggregate(p, energy, sel)
            assert np.isfinite(r["avg_pose"]).all() and np.isfinite(r["sorted_RTs"]).all()
            # every candidate lies within 0.3 sqrt 3 rad of the centre: its quaternion has at most sin^2(0.26) = 0.066 of its unit
            # weight off the centre's, so lambda_max >= 0.934, the other three share <= 0.066, and the gap is >= 0.868
            assert r["gap"].min() >= (0.5 if inside else 0.868), (name, spread, B, K, sel, r["gap"].min())
            worst_gap = min(worst_gap, float(r["gap"].min()))
            top = p[np.arange(B)[:, None], r["order"][:, :sel, 0], :6]
            branches |= set(np.unique(rr.quat_branch(rr.gram_schmidt(top))[1]).tolist())
            for b in range(B):
                q = r["quats"][b]
                A = (q[:, :, None] * q[:, None, :]).sum(axis=0) / sel
                with np.errstate(over="ignore"):  # (theta^2 overflows to inf for a rounding-sized off-diagonal entry: t = 0, as on the device)
                    v, sweeps = rr.jacobi_top_eigvec(A)
                    v6, _ = rr.jacobi_top_eigvec(A, max_sweeps=6)
                if sel >= 4 and spread > 0 and inside is None:
                    assert sweeps <= 6, (name, spread, B, K, sel, sweeps)
                    worst_sweeps = max(worst_sweeps, sweeps)
                else:
                    stalled += sweeps == 30
                d = float(max(_up_to_sign(v, r["avg_pose"][b, :4]), _up_to_sign(v6, r["avg_pose"][b, :4])))
                assert d <= EIG_ATOL, (name, spread, B, K, sel, d)
                worst_vec = max(worst_vec, d)
    assert branches == {0, 1, 2, 3}
    print(f"smallest gap {worst_gap:.4f}, most Jacobi sweeps at full rank {worst_sweeps}, largest |jacobi - eigh| {worst_vec:.2e}, "
          f"rank-deficient matrices that ran all 30 sweeps: {stalled}")


def test_jacobi_picks_the_largest_diagonal_entry_of_a_diagonal_matrix():
    """Already diagonal: no sweep runs and the pick is the largest diagonal entry, wherever it sits."""
    for pos in range(4):
        d = np.full(4, 0.01)
        d[pos] = 0.97
        v, sweeps = rr.jacobi_top_eigvec(np.diag(d))
        assert sweeps == 0 and np.array_equal(v, np.eye(4)[pos])
        np.testing.assert_array_equal(np.abs(rr.top_eigvec(np.diag(d))[0]), np.eye(4)[pos])
