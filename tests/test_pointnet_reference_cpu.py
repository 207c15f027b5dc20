"""CPU: the plain-torch PointNet reference of tests/pointnet_reference.py and the yardstick test_gpu_f64_pointnet.py takes from it.

The kernels of csrc/pointnet.hip are gated at MARGIN x the float32 reference's OWN error against float64.  That means something only if
the reference is the reference project's network (it reproduces the fixture g18_pointnet.npz), its own error is a rounding error (above
zero, under ORACLE_CEILING), and the inputs reach what the kernels can get wrong: clouds on which a zero padding row would win the
maximum, pooled values of both signs, an integer network on which float32 is exact.  Every check here is a condition on the reference
alone; no kernel enters this file."""
import numpy as np
import torch

import f64_reference as fr
import pointnet_reference as pr

FIXTURE_SHAPES = ((3, 1024), (2, 37), (1, 1), (2, 1100))
FIXTURE_ATOL = 5e-6  # the reference project's fp32 CPU result against this file's fp32 functions (measured: at most 2.4e-6)


def test_reference_reproduces_the_fixture(golden):
    g = golden("g18_pointnet.npz")
    sd = pr.state_dict("seed0")
    worst = 0.0
    for B, n in FIXTURE_SHAPES:
        feat, trans = pr.pointnet(sd, torch.from_numpy(g[f"clouds_{B}x{n}"]))
        for name, got in (("feat", feat), ("trans", trans)):
            d = float(np.abs(got.numpy() - g[f"{name}_{B}x{n}"]).max())
            worst = max(worst, d)
            assert d <= FIXTURE_ATOL, (name, B, n, d)
    for mode in ("score", "energy"):
        d = float(np.abs(pr.fused_case(mode)["f32"].numpy() - g[f"fused_feat_{mode}"]).max())
        worst = max(worst, d)
        assert d <= FIXTURE_ATOL, ("fused", mode, d)
    print(f"fp32 reference vs g18_pointnet.npz: max |diff| = {worst:.3e}")


def test_oracles_own_error_is_a_rounding_error():
    """0 < E_oracle < ORACLE_CEILING per quantity, in every case; the maxima printed here are what the GPU tests multiply by MARGIN"""
    for c in pr.case_set():
        for q, e in pr.oracle_errors(*c).items():
            assert 0 < e < fr.ORACLE_CEILING, (c, q, e)
    for i, e in enumerate(pr.dense_oracle_errors()):
        print(f"E_oracle | dense {pr.DENSE_CASES[i]} | {e:.3e}")
        assert 0 <= e < fr.ORACLE_CEILING, (pr.DENSE_CASES[i], e)  # (a K = 4 product can be exact)
    for q in ("g", "trans", "feat_given_trans", "feat", "dense", "fused"):
        e = pr.e_oracle(q)
        print(f"E_oracle | {q:16s} | {e:.3e}")
        assert 0 < e < fr.ORACLE_CEILING, (q, e)


def test_clouds_exercise_the_mask_and_the_signed_maximum():
    """Offset-0.5 clouds: a zero padding row (x . trans = 0 under any trans: the trunk's bias chain) exceeds the maximum over the real points in at
    least MASK_SHARE of the 1024 channels of every cloud - an unmasked padding row is visible there.  Every case: at least
    NEGATIVE_SHARE of the pooled trunk channels are negative (the order-preserving key's negative branch)."""
    lo_mask, lo_neg = 1.0, 1.0
    for which, B, n, off in pr.case_set():
        c = pr.case(which, B, n, off)
        neg = (c["feat64"] < 0).double().mean(dim=1)
        lo_neg = min(lo_neg, float(neg.min()))
        assert float(neg.min()) >= pr.NEGATIVE_SHARE, (which, B, n, off, neg)
        if off == pr.MASK_OFFSET:
            pad = pr.trunk_rows(pr.state_dict64(which), torch.zeros(1, 1, 3), c["trans64"][:1])[0, 0]
            share = (pad[None, :] > c["feat64"]).double().mean(dim=1)
            lo_mask = min(lo_mask, float(share.min()))
            assert float(share.min()) >= pr.MASK_SHARE, (which, B, n, share)
    print(f"padding row wins in >= {lo_mask:.3f} of the channels (offset {pr.MASK_OFFSET}); negative pooled channels >= {lo_neg:.3f}")


def test_integer_network_is_exact_in_float32():
    sd = pr.integer_state_dict()
    sd64 = fr.f64_state_dict(sd)
    for k, v in sd.items():
        assert torch.equal(v, v.round()) and (float(v.abs().max()) <= 1 or k.endswith(".bias")), k
    for B, n in pr.INTEGER_SHAPES:
        pts = pr.integer_clouds(B, n)
        assert pr.integer_bound(sd, pts) < pr.EXACT
        (f32, t32), (f64, t64) = pr.pointnet(sd, pts), pr.pointnet(sd64, pts)
        g32, g64 = pr.stn_pool(sd, pts), pr.stn_pool(sd64, pts)
        assert f32.dtype == torch.float32 and f64.dtype == torch.float64
        assert torch.equal(f32.double(), f64) and torch.equal(g32.double(), g64)
        assert torch.equal(t64, torch.eye(3, dtype=torch.float64).expand(B, 3, 3)) and torch.equal(t32.double(), t64)
        # a network worth running: many distinct values of both signs, clouds that differ
        assert len(torch.unique(f64)) > 50 and bool((f64 < 0).any()) and bool((f64 > 0).any()) and not torch.equal(f64[0], f64[1])
    for i in range(len(pr.DENSE_CASES)):
        assert torch.equal(pr.dense_reference(i, torch.float32, integer=True).double(), pr.dense_reference(i, torch.float64, integer=True))
