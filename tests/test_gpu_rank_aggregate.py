"""GPU: energy ranking and top-`sel` aggregation (csrc/rank.hip: rank_aggregate_kernel; reward.rank_aggregate, with and without the 4x4
forms) against the float64 restatement of its definition (tests/rank_reference.py; checked on the CPU by tests/test_rank_reference_cpu.py).

Inputs: candidates clustered around one pose - the regime the runners are in, where the top eigenvalue of mean(q q^T) is well separated -
for seven centres that between them take all four matrix_to_quaternion branches, the four-way tie and the w > 0 orientation at both sides
of a half turn, at spreads 0 (identical candidates), 0.02 and 0.3 rad; at sizes around the wave's 64 lanes, and around the 64 KB of
dynamic LDS a launch has by default (sel = k = 1365 asks for exactly 65 536 bytes, 1366 for more, the cap k = sel = 2048 for 98 320).

Bounds (derived, not measured).  The ranking is a permutation: order, sorted_energy and sorted_poses are compared bit for bit.  The
aggregate is computed in float64 registers and rounded ONCE to float32: components are at most 1 in magnitude, so the rounding costs
<= 2**-25; the float64 eigenvector is off by about eps / gap ~ 1e-15 at the gap >= 0.5 the test first asserts of its inputs.  The bound is
2**-23 per component, four times the rounding.  The unit norm follows to 2 * 2**-23 = 2**-22.  Translations: the same rounding relative to
their magnitude, 2**-23 max(1, |ref|).  sorted_RTs are float64 throughout: 1e-12, the bound the golden test has.  The sign of the quaternion
is the reference's wherever |w_ref| >= 1e-6; below that (an exact half turn has w ~ 6e-17) it is rounding, and the comparison is up to a
global sign."""
import numpy as np
import pytest
import torch

import rank_reference as rr

pytestmark = pytest.mark.gpu

QUAT_ATOL = 2.0 ** -23
NORM_ATOL = 2.0 ** -22
DTYPES = {"f32": np.float32, "f64": np.float64}


class Worst:
    """The largest observed value of every asserted quantity, printed for the record (the bounds above are the derived ones)."""

    def __init__(self):
        self.v = {"quat": 0.0, "norm": 0.0, "trans_rel": 0.0, "sorted_RTs": 0.0}

    def __str__(self):
        return ", ".join(f"{k} {v:.3e}" for k, v in self.v.items())


def _check(poses, energy, sel, worst, what):
    """poses [B,K,9] numpy in the dtype under test, energy [B,K,2] f32: both entry points against the reference."""
    from genpose_amd import reward, rotation
    ref = rr.rank_aggregate(poses, energy, sel)
    assert ref["gap"].min() >= 0.5, (what, ref["gap"])  # a property of the inputs: the eigenvector is determined to ~1e-15
    p, e = torch.from_numpy(poses).cuda(), torch.from_numpy(energy).cuda()
    for with_rt in (False, True):
        r = reward.rank_aggregate(p, e, selected_num=sel, with_rt=with_rt)
        tag = (what, "with_rt" if with_rt else "plain")
        assert r["order"].dtype == torch.int32 and r["sorted_poses"].dtype == p.dtype and r["avg_pose"].dtype == torch.float32
        assert np.array_equal(r["order"].cpu().numpy().astype(np.int64), ref["order"]), tag
        assert np.array_equal(r["sorted_energy"].cpu().numpy().view(np.int32), ref["sorted_energy"].view(np.int32)), tag
        sp = r["sorted_poses"].cpu().numpy()
        assert np.array_equal(sp.view(np.uint8), np.ascontiguousarray(ref["sorted_poses"]).view(np.uint8)), tag
        got = r["avg_pose"].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), tag
        q, q_ref = got[:, :4], ref["avg_pose"][:, :4]
        d_same, d_flip = np.abs(q - q_ref).max(axis=1), np.abs(q + q_ref).max(axis=1)
        d = np.where(np.abs(q_ref[:, 0]) >= 1e-6, d_same, np.minimum(d_same, d_flip))
        worst.v["quat"] = max(worst.v["quat"], float(d.max()))
        assert d.max() <= QUAT_ATOL, (tag, d, q, q_ref)
        n = np.abs(np.sqrt((q * q).sum(axis=1)) - 1.0)
        worst.v["norm"] = max(worst.v["norm"], float(n.max()))
        assert n.max() <= NORM_ATOL, (tag, n)
        t, t_ref = got[:, 4:], ref["avg_pose"][:, 4:]
        rel = np.abs(t - t_ref) / np.maximum(1.0, np.abs(t_ref))
        worst.v["trans_rel"] = max(worst.v["trans_rel"], float(rel.max()))
        assert rel.max() <= QUAT_ATOL, (tag, rel)
        if with_rt:
            rt = r["sorted_RTs"].cpu().numpy()
            assert rt.dtype == np.float64
            worst.v["sorted_RTs"] = max(worst.v["sorted_RTs"], float(np.abs(rt - ref["sorted_RTs"]).max()))
            np.testing.assert_allclose(rt, ref["sorted_RTs"], rtol=0, atol=1e-12, err_msg=str(tag))
            assert torch.equal(r["avg_RT"], rotation.quat_trans_to_RT(r["avg_pose"])), tag
            assert torch.equal(r["sorted_RTs"], rotation.pose9_to_RT(r["sorted_poses"])), tag
    return r


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("B,K,sel", rr.SIZES)
def test_clusters_against_the_float64_reference(B, K, sel, dtype):
    from genpose_amd import reward
    worst = Worst()
    for name, spread in rr.FAMILIES:
        poses, energy = rr.family_inputs(name, spread, B, K)
        r = _check(poses.astype(DTYPES[dtype]), energy, sel, worst, (name, spread))
    # ranking only (no aggregate, no LDS for the quaternions): the same permutation
    p, e = torch.from_numpy(poses.astype(DTYPES[dtype])).cuda(), torch.from_numpy(energy).cuda()
    for with_rt in (False, True):
        ro = reward.rank_aggregate(p, e, with_rt=with_rt)
        assert ro["avg_pose"] is None and (not with_rt or ro["avg_RT"] is None)
        for k in ("order", "sorted_energy", "sorted_poses") + (("sorted_RTs",) if with_rt else ()):
            assert torch.equal(ro[k], r[k]), k
    print(f"({B}, {K}, {sel}) {dtype}: worst {worst}")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_many_ties_at_the_cap(dtype):
    """Integer energies 0..3 at k = 2048: about 512 candidates tie at every level, the stable order decides every rank."""
    worst = Worst()
    for B, K, sel in ((2, 2048, 2048), (1, 2048, 1228)):
        for name, spread in (("generic", 0.02), ("near_pi", 0.3)):
            poses, energy = rr.family_inputs(name, spread, B, K, ties=True)
            _check(poses.astype(DTYPES[dtype]), energy, sel, worst, (name, spread, K, sel))
    print(f"ties at k = 2048, {dtype}: worst {worst}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("inside", [False, True], ids=["tail", "inside"])
def test_degenerate_poses_in_a_cluster(inside, dtype):
    """The all-zero pose, a zero first column, a second column parallel to the first, and columns just above and below the 1e-12 floors of
    the Gram-Schmidt step (rank_reference.DEGENERATE: matrix_to_quaternion inputs that are no rotations) among the candidates of a cluster:
    ranked beyond `sel`, where they reach sorted_poses and sorted_RTs only, and ranked first, where they enter the average.  The expected
    values are what the definition gives."""
    worst = Worst()
    for name in rr.CENTRES:
        poses, energy = rr.family_inputs(name, 0.02, 5, 50)
        poses, energy = rr.with_degenerate(poses, energy, inside)
        r = _check(poses.astype(DTYPES[dtype]), energy, 30, worst, (name, "inside" if inside else "tail"))
        assert torch.isfinite(r["sorted_RTs"]).all() and torch.isfinite(r["avg_RT"]).all()
        first = r["order"][:, :30, 0].cpu().numpy()
        where = rr.degenerate_positions(50)
        assert all((np.isin(where, first[b]).all() if inside else not np.isin(where, first[b]).any()) for b in range(5))
    print(f"degenerate {'inside' if inside else 'tail'} {dtype}: worst {worst}")
