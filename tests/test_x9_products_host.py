"""CPU (no GPU): the arithmetic of the encoder kernels' EIGHT-product form of the nine-term split (csrc/bf16x9.h, mma9<.., NPROD = 8>: lo.lo
is not issued), in numpy float64 on the project's own split (weights.split_bf16x9: hi = bf16(x), mid = bf16(x - hi), lo = x - hi - mid).

Why float64 is an exact judge here: every term is a bf16 value (8 significand bits), every product of two terms has at most 16 bits, and
any partial sum of the nine products of one multiply a_k b_k lies on the grid of its smallest product and below 4 |a_k b_k| - at most 50
bits.  So `a_k b_k - (eight kept products)` is computed without rounding and IS lo_a lo_b.  Only the K-long sums round (2^-53 relative per
addition: K 2^-53 << 2^-32).

Bounds (round to nearest even at every stage, 2^e <= |x| < 2^(e+1)): |x - hi| <= 2^-8 2^e, so |mid| <= 2^-8 |x|; |(x - hi) - mid| <=
2^-8 2^-8 2^e, so |lo| <= 2^-16 |x|; hence |lo_a lo_b| <= 2^-32 |a b| per multiply."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from oracle import genpose_oracle as go

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (64, 128, 512)
# mma9's order as bf16x9.h states it, (term of W, term of X) with 0 = hi, 1 = mid, 2 = lo, smallest terms first - restated once, WITHOUT
# the ninth entry (lo.lo, which stands first in the text's tables)
KEPT = ((2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


def _split(x):
    """fp32 array -> (hi, mid, lo) as float64 arrays, by the project's split (which also checks hi + mid + lo == x bit for bit)."""
    from genpose_amd.weights import split_bf16x9
    return tuple(t.double().numpy() for t in split_bf16x9(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))))


def _check_rows(A, B, what):
    """Rows of A against rows of B (fp32, same shape [R, K]): the bounds on the terms and on what eight products leave out."""
    a, b = A.astype(np.float64), B.astype(np.float64)
    ta, tb = _split(A), _split(B)
    for x, t in ((a, ta), (b, tb)):
        assert np.array_equal((t[0] + t[1]) + t[2], x), what                      # the split is exact
        assert np.all(np.abs(t[1]) <= 2.0 ** -8 * np.abs(x)), what
        assert np.all(np.abs(t[2]) <= 2.0 ** -16 * np.abs(x)), what
    kept = np.zeros_like(a)
    for wa, xb in KEPT:  # smallest first, as the kernel issues them; exact in float64 in any order (module text)
        kept += ta[wa] * tb[xb]
    miss = a * b - kept
    assert np.array_equal(miss, ta[2] * tb[2]), what                              # what is not formed is lo.lo, exactly
    assert np.all(np.abs(miss) <= 2.0 ** -32 * np.abs(a * b)), what               # per multiply
    bound = 2.0 ** -32 * np.sum(np.abs(a) * np.abs(b), axis=1)
    diff = np.abs(np.sum(kept, axis=1) - np.sum(a * b, axis=1))
    print(f"{what}: max |sum of eight - dot| / (2^-32 sum |a||b|) = {float(np.max(diff / bound)):.3e}")
    assert np.all(diff <= bound), what                                            # per dot product


@pytest.mark.parametrize("K", KS)
def test_random_normal_vectors(K):
    rng = np.random.default_rng(1000 + K)
    A = rng.standard_normal((256, K)).astype(np.float32)
    B = rng.standard_normal((256, K)).astype(np.float32)
    _check_rows(A, B, f"normal, K = {K}")
    # all signs equal: nothing cancels in the sum - the worst case of the bound
    _check_rows(np.abs(A), np.abs(B), f"|normal|, K = {K}")


@functools.lru_cache(maxsize=None)
def _folded():
    from genpose_amd.weights import EncoderWeights
    w = EncoderWeights(go.make_state_dict(0, "score"), "cpu")
    return {(k, i, l): sc._folded_plain[l][0] for k in (1, 2, 3) for i, sc in enumerate(w.levels[k]) for l in (1, 2)} | {
        (3, i, 0): sc._folded_plain[0][0][:, :-3] for i, sc in enumerate(w.levels[3])}  # GroupAll: layer 1's feature half is split bf16 too


def test_folded_encoder_weights():
    shapes = {key: tuple(W.shape) for key, W in _folded().items()}
    assert shapes[(1, 0, 1)] == (64, 64) and shapes[(1, 1, 2)] == (128, 96) and shapes[(2, 0, 1)] == (196, 128) and shapes[(2, 1, 2)] == (256, 196)
    assert shapes[(3, 0, 0)] == (256, 512) and shapes[(3, 1, 1)] == (384, 256) and shapes[(3, 1, 2)] == (512, 384)
    assert len(shapes) == 14
    rng = np.random.default_rng(7)
    for key, W in sorted(_folded().items()):
        W = W.numpy()
        # activations as the layers see them: after a ReLU (non-negative), and signed (the GroupAll level's input features are post-ReLU
        # too, but a signed partner is the harder case for the per-multiply bound's generality)
        X = rng.standard_normal(W.shape).astype(np.float32)
        _check_rows(W, np.maximum(X, 0), f"level {key[0]} scale {key[1]} layer {key[2] + 1} {W.shape} x relu(normal)")
        _check_rows(W, X, f"level {key[0]} scale {key[1]} layer {key[2] + 1} {W.shape} x normal")


def test_order_table_of_mma9():
    text = open(os.path.join(ROOT, "genpose_amd", "csrc", "bf16x9.h")).read()
    body = text[text.index("void mma9("):]
    body = body[:body.index("\n}\n")]
    tables = {m.group(1): tuple(int(v) for v in m.group(2).split(",")) for m in re.finditer(r"constexpr int (WA|XB)\[9\] = \{([0-9, ]+)\};", body)}
    assert set(tables) == {"WA", "XB"}
    order = tuple(zip(tables["WA"], tables["XB"]))
    assert sorted(order) == [(i, j) for i in range(3) for j in range(3)]           # nine entries: every pair of terms once
    assert order[0] == (2, 2)                                                      # the ninth product, lo.lo, stands first ...
    assert order[1:] == KEPT                                                       # ... and without it the table is the eight kept ones
    sizes = [wa + xb for wa, xb in order]
    assert sizes == sorted(sizes, reverse=True)                                    # smallest terms first (term index = 8 bits down each)
    # the loop starts behind lo.lo for NPROD = 8 and opens the accumulator on the first product it issues
    assert re.search(r"constexpr int Q0 = 9 - NPROD;", body) and re.search(r"for \(int q = Q0; q < 9; \+\+q\)", body)
    assert re.search(r"first && q == Q0 \? f32x4\{0\.f, 0\.f, 0\.f, 0\.f\} : acc\[p\]", body)
    assert re.search(r"static_assert\(NPROD == 9 \|\| NPROD == 8", body)
    assert re.search(r"template <int NT, bool TRANSPOSED = false, int NPROD = 9>\s*\n__device__ __forceinline__ void mma9\(", text)
    # the encoder kernels' count: eight unless a measurement build says otherwise; the trunks never name it
    assert re.search(r"#ifndef GP_SA_X9_PRODUCTS\n#define GP_SA_X9_PRODUCTS 8\n#endif", text)
    for name, uses in (("sa_bf16x9.hip", 1), ("sa_lds_bf16x9.hip", 2), ("sa_groupall_bf16x9.hip", 1)):
        src = open(os.path.join(ROOT, "genpose_amd", "csrc", name)).read()
        assert len(re.findall(r"(?:mma9|ring_step)<[^>]*\bSA_NPROD>", src)) == uses, name
        assert not re.search(r"(?:mma9|ring_step)<(?![^>]*SA_NPROD)[^>]*>\(", src), name   # no site left at the default
    for name in ("trunk_bf16x9.h", "trunk_bf16x9.hip", "rk45.hip", "heun_solve.hip", "trunk_chain.h"):
        assert "SA_NPROD" not in open(os.path.join(ROOT, "genpose_amd", "csrc", name)).read(), name
