"""CPU: the float64 references of tests/f64_reference.py and the yardstick the GPU tests take from them.

The fp32 kernels are gated at MARGIN x the fp32 CPU oracle's OWN error against float64 (test_gpu_f64_score.py, test_gpu_f64_encoder.py).
That only means something if (a) the float64 functions are the oracle's functions - they agree with it to AGREE of the scale - and (b) the
oracle's own error is a rounding error: above zero and under ORACLE_CEILING in every (weights, quantity, block, t) cell.  Both are
conditions on the reference alone; no kernel enters this file."""
import numpy as np
import pytest
import torch

import f64_reference as fr
from oracle import genpose_oracle as go

QUANTITIES = ("score", "energy", "escore", "sdiv", "embed")


def _cells(which, quantity):
    for t in fr.TIMES:
        for B, K in fr.SHAPES:
            for sc in (fr.POSE_SCALES if quantity != "embed" else fr.POSE_SCALES[:1]):
                yield t, B, K, sc


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_float64_functions_are_the_oracles(which):
    """every float64 quantity against the fp32 oracle on the GPU tests' inputs: AGREE of the block's scale (derivatives on kink-free rows)"""
    for q in QUANTITIES:
        for t, B, K, sc in _cells(which, q):
            for name, e in fr.oracle_error(which, q, B, K, sc, t).items():
                assert max(e) <= fr.AGREE, (which, name, t, B, K, sc, e)


@pytest.mark.parametrize("which", fr.WEIGHTS)
def test_oracles_own_error_is_a_rounding_error(which):
    """0 < E_oracle < ORACLE_CEILING per (quantity, block, t); the rows left out for a ReLU kink stay under KINK_SHARE of every case; the
    energies' inner products cancel by at most CANCEL_LIMIT on every case."""
    for q in QUANTITIES:
        for t in fr.TIMES:
            e = fr.e_oracle(which, q, t)
            print(f"{which:8s} {q:7s} t {t:<6g} " + "  ".join(f"{n} " + "/".join(f"{x:.2e}" for x in v) for n, v in e.items()))
            for name, v in e.items():
                assert all(0 < x < fr.ORACLE_CEILING for x in v), (which, name, t, v)
        if q in ("escore", "sdiv"):
            for t, B, K, sc in _cells(which, q):
                keep = fr.case(which, q, B, K, sc, t)["keep"]
                assert 1.0 - float(keep.double().mean()) <= fr.KINK_SHARE, (which, q, t, B, K, sc, int((~keep).sum()))
    for t, B, K, sc in _cells(which, "energy"):  # no case measures the cancellation of an inner product instead of an evaluation
        assert max(fr.cancellation(which, B, K, sc, t)) <= fr.CANCEL_LIMIT, (which, t, B, K, sc, fr.cancellation(which, B, K, sc, t))


def test_block_error_keeps_blocks_apart():
    ref = torch.zeros(4, 9, dtype=torch.float64)
    ref[:, 0:3], ref[:, 3:6], ref[:, 6:9] = 100.0, 1.0, 0.01
    got = ref.clone()
    got[2, 7] += 1e-4  # 1 % of the small head, 1e-6 of the large one
    assert fr.block_error(got, ref) == [0.0, 0.0, pytest.approx(1e-2)]
    assert fr.block_error(got, ref, None) == [pytest.approx(1e-6)]
    assert fr.block_error(got[:, :2], ref[:, :2]) == [0.0, 0.0] and fr.block_error(got[:, 0], ref[:, 0]) == [0.0]
    assert fr.block_error(got, ref, rows=torch.tensor([True, True, False, True])) == [0.0, 0.0, 0.0]


def test_near_kink_finds_a_unit_at_zero():
    """a bias moved so that one head unit's pre-activation is exactly zero on row 0: that row is reported, and only rows like it"""
    sd64 = dict(fr.state_dict64("seed0", "score"))
    feat, pose, _, _ = fr.inputs(3, 7, 1.0)
    assert not bool(fr.near_kink(sd64, feat, 7, pose, 0.55).any())
    key = fr.P + "fusion_tail_rot_y.0"
    h2 = torch.relu(go._lin(sd64, fr.P + "pose_encoder.2", torch.relu(go._lin(sd64, fr.P + "pose_encoder.0", pose[:1].double()))))
    total = torch.cat([feat[:1].double(), fr.embed_time(sd64, 0.55), h2], dim=-1)
    b = sd64[key + ".bias"].clone()
    b[5] -= go._lin(sd64, key, total)[0, 5]
    sd64[key + ".bias"] = b
    assert fr.near_kink(sd64, feat, 7, pose, 0.55).tolist() == [True] + [False] * 20


@pytest.mark.parametrize("which", ["seed0", "stress", "trained"])
def test_float64_encoder_is_the_oracles(which):
    """the float64 encoder on the oracle's grouping against encoder_forward, two clouds (one of tiled duplicates): every level and the
    1024 features to AGREE of the scale; its own error above zero and under the ceiling"""
    pts = fr.encoder_clouds()[2:]
    sd = fr.state_dict(which, "score")
    out, inter = go.encoder_forward(sd, pts, return_intermediates=True)
    out64, levels = fr.encoder64(fr.f64_state_dict(sd), pts, inter)
    assert out64.dtype == torch.float64 and out64.shape == (2, 1024)
    errs = fr.encoder_errors([r["features"] for r in inter], levels)
    for k, per_cloud in enumerate(errs):
        for e in per_cloud:
            assert all(0 < x < fr.ORACLE_CEILING for x in e), (which, k, e)
    np.testing.assert_allclose(out.numpy(), out64.numpy(), rtol=0, atol=fr.AGREE * float(out64.abs().max()))
