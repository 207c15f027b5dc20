"""CPU (no GPU): the arithmetic of the SIX-product form of the nine-term split (csrc/bf16x9.h, mma9<.., NPROD = 6>: lo.lo, lo.mid and
mid.lo are not issued) - the encoder kernels as the project builds them and the PC step's six-product kernels (csrc/trunk_bf16x9.hip) - in
numpy float64 on the project's own split (weights.split_bf16x9).  It supersedes, for those kernels, the eight-product statement of
tests/test_x9_products_host.py, whose bounds on the terms (|mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|) and whose argument that float64 is an
exact judge of a single multiply are used here unchanged.

1. nine - six == mid_a lo_b + lo_a mid_b + lo_a lo_b, exactly, per multiply.
2. |dropped| <= (2^-23 + 2^-32) |a||b| per multiply, hence <= (2^-23 + 2^-32) sum |a_i||b_i| per dot product.
3. Whole layers, EMULATED: the split kernels as k-blocks of 32 with the products smallest first and one fp32 rounding per MFMA (an
   assumption about the matrix pipe's internal sum: its 32 products and the C operand are added exactly and rounded once); the fp32 MFMA
   kernels as k-blocks of 4 in one chain.  On every BN-folded weight matrix the kernels use and on random matrices, signed and post-ReLU
   partners: the six-product result's max error against float64, over the output scale, is at most GATE_VS_F32 = 1.5 x the emulated fp32
   MFMA layer's (the project's gate for a split kernel against the fp32 kernel it replaces, tests/test_gpu_bf16x9.py).
4. Negative control: FIVE products (lo.hi dropped as well, 2^-16 |a b| per multiply) exceed that rule on the same inputs - six is the
   boundary."""
import functools

import numpy as np
import pytest
import torch

from oracle import genpose_oracle as go

from test_x9_products_host import _folded, _split

GATE_VS_F32 = 1.5
# mma9's order (term of W, term of X), 0 = hi, 1 = mid, 2 = lo, smallest terms first; NPROD = 6 starts at the fourth entry
ORDER = ((2, 2), (2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))
DROPPED = ORDER[:3]
NCOLS = 128


def test_what_six_products_leave_out():
    rng = np.random.default_rng(606)
    for K in (64, 128, 256, 512):
        A = rng.standard_normal((256, K)).astype(np.float32)
        B = rng.standard_normal((256, K)).astype(np.float32)
        for A_, B_, what in ((A, B, "normal"), (np.abs(A), np.abs(B), "|normal|"), (A, np.maximum(B, 0), "normal x relu")):
            a, b = A_.astype(np.float64), B_.astype(np.float64)
            ta, tb = _split(A_), _split(B_)
            nine = sum(ta[i] * tb[j] for i, j in ORDER)
            six = sum(ta[i] * tb[j] for i, j in ORDER[3:])
            assert np.array_equal(nine, a * b), (what, K)                                    # the nine products are the product, exactly
            miss = nine - six
            assert np.array_equal(miss, sum(ta[i] * tb[j] for i, j in DROPPED)), (what, K)   # 1.
            c = 2.0 ** -23 + 2.0 ** -32
            assert np.all(np.abs(miss) <= c * np.abs(a * b)), (what, K)                      # 2., per multiply
            bound = c * np.sum(np.abs(a) * np.abs(b), axis=1)
            diff = np.abs(np.sum(six, axis=1) - np.sum(a * b, axis=1))
            print(f"{what}, K = {K}: max |sum of six - dot| / ((2^-23 + 2^-32) sum |a||b|) = {float(np.max(diff / bound)):.3e}")
            assert np.all(diff <= bound), (what, K)                                          # 2., per dot product


def _split_layer(W, X, nprod):
    """W [M, K] . X [K, N] as the split kernels form it: k-blocks of 32 ascending (K padded with zeros), the last `nprod` products of ORDER
    in order, the accumulator rounded to fp32 once per MFMA."""
    M, K = W.shape
    Kp = -(-K // 32) * 32
    Wp, Xp = np.zeros((M, Kp), np.float32), np.zeros((Kp, X.shape[1]), np.float32)
    Wp[:, :K], Xp[:K] = W, X
    tw, tx = _split(Wp), _split(Xp)
    acc = np.zeros((M, X.shape[1]), np.float32)
    for k0 in range(0, Kp, 32):
        for i, j in ORDER[9 - nprod:]:
            acc = (acc.astype(np.float64) + tw[i][:, k0:k0 + 32] @ tx[j][k0:k0 + 32]).astype(np.float32)
    return acc


def _f32_layer(W, X):
    """The fp32 MFMA kernels' form: one chain of k-blocks of 4, one fp32 rounding per MFMA."""
    M, K = W.shape
    Kp = -(-K // 4) * 4
    Wp, Xp = np.zeros((M, Kp), np.float64), np.zeros((Kp, X.shape[1]), np.float64)
    Wp[:, :K], Xp[:K] = W, X
    acc = np.zeros((M, X.shape[1]), np.float32)
    for k0 in range(0, Kp, 4):
        acc = (acc.astype(np.float64) + Wp[:, k0:k0 + 4] @ Xp[k0:k0 + 4]).astype(np.float32)
    return acc


@functools.lru_cache(maxsize=None)
def _cases():
    """(name, W [M, K] fp32, X [K, NCOLS] fp32): every weight matrix the six-product kernels multiply, and random ones"""
    rng = np.random.default_rng(66)
    out = []
    sd = go.make_state_dict(0, "score")
    p = "pose_score_net."
    mats = [("trunk pose_encoder.0", sd[p + "pose_encoder.0.weight"].numpy(), 50.0), ("trunk pose_encoder.2", sd[p + "pose_encoder.2.weight"].numpy(), 1.0)]
    mats += [(f"trunk head {h}", sd[f"{p}fusion_tail_{h}.0.weight"][:, -256:].numpy(), 1.0) for h in ("rot_x", "rot_y", "trans")]
    mats += [(f"encoder level {k[0]} scale {k[1]} layer {k[2] + 1}", W.numpy(), 1.0) for k, W in sorted(_folded().items())]
    for name, W, scale in mats:
        W = np.ascontiguousarray(W, dtype=np.float32)
        X = (rng.standard_normal((W.shape[1], NCOLS)) * scale).astype(np.float32)
        out.append((f"{name} {W.shape} x normal", W, X))
        if "pose_encoder.0" not in name:  # its input is the pose itself, signed
            out.append((f"{name} {W.shape} x relu(normal)", W, np.maximum(X, 0)))
    for K in (64, 128, 256, 512):
        W = rng.standard_normal((256, K)).astype(np.float32)
        X = rng.standard_normal((K, NCOLS)).astype(np.float32)
        out.append((f"normal (256, {K}) x normal", W, X))
        out.append((f"normal (256, {K}) x relu(normal)", W, np.maximum(X, 0)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _errors():
    rows = []
    for name, W, X in _cases():
        ref = W.astype(np.float64) @ X.astype(np.float64)
        scale = float(np.abs(ref).max())
        e = {n: float(np.abs(_split_layer(W, X, n) - ref).max()) / scale for n in (9, 6, 5)}
        e[32] = float(np.abs(_f32_layer(W, X) - ref).max()) / scale
        rows.append((name, e))
    return tuple(rows)


def test_trunk_and_encoder_matrices_are_all_there():
    names = [n for n, _, _ in _cases()]
    assert sum(n.startswith("trunk") for n in names) == 1 + 2 * 4 and sum(n.startswith("encoder") for n in names) == 2 * 14
    shapes = {n.split(" (")[0]: W.shape for n, W, _ in _cases()}
    assert shapes["trunk pose_encoder.0"] == (256, 9) and shapes["trunk pose_encoder.2"] == (256, 256) and shapes["trunk head trans"] == (256, 256)


def test_six_product_layers_stay_in_the_fp32_class():
    bad = []
    for name, e in _errors():
        print(f"{name:64s} fp32 MFMA {e[32]:.2e} | nine {e[9]:.2e} | six {e[6]:.2e} ({e[6] / e[32]:.2f}x fp32) | five {e[5]:.2e} ({e[5] / e[32]:.1f}x)")
        if not e[6] <= GATE_VS_F32 * e[32]:
            bad.append((name, e[32], e[6]))
    assert not bad, bad


def test_negative_control_five_products_leave_it():
    bad = [(name, e[32], e[5]) for name, e in _errors() if not e[5] > GATE_VS_F32 * e[32]]
    assert not bad, bad
