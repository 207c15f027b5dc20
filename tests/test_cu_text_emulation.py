"""CPU: what the reference's CUDA kernel TEXT computes, against the oracle - a DIAGNOSTIC, not a parity pin.

The text of sampling_gpu.cu (furthest point sampling incl. its shared-memory tree), ball_query_gpu.cu and interpolate_gpu.cu (three_nn,
three_interpolate) was compiled by the HOST compilers against oracle/cu_emul/cuda_model.h (every CUDA thread a cooperative fiber,
__syncthreads() a round-robin barrier) and run on the golden clouds of g1_g2_ops.npz; its outputs are stored in tests/golden/g17_cu_text.npz
(oracle/gen_cu_text_golden.py, build container only: it needs the reference tree).  Nothing of the reference is committed or shipped; the
model stands in for the CUDA headers, so this is not an oracle/_ref build.

What it establishes:
  1. oracle/pn2_ops.c follows the kernel text (tie rule of the tree, multi-point threads, first-hit prefill, double best-distances):
     with contraction OFF the text's outputs equal the oracle's convention C bit for bit;
  2. what real compilers do to `dx*dx + dy*dy + dz*dz` in THIS text: g++ and clang++ (LLVM, the family nvcc's NVVM derives from) with
     contraction on both produce the oracle's convention B - never A - which is why B is the default.
"""
import hashlib

import numpy as np
import pytest

from oracle import pn2_oracle as ops

FIXTURE = "g17_cu_text.npz"
VARIANTS = {
    # tag: (compiler and contraction flags the text was built with, the oracle convention the text must reproduce)
    "gxx_off": ("g++ -ffp-contract=off", "C"),
    "gxx_fma": ("g++ -mfma -ffp-contract=fast", "B"),
    "clang_fma": ("clang++ -mfma -ffp-contract=fast", "B"),
    "clang_default": ("clang++ -mfma", "B"),  # clang's default -ffp-contract=on (front-end fmuladd): the same fusion
}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.int32).tobytes()).hexdigest()


def _text(golden, tag):
    g = golden(FIXTURE)
    return {k.split("__", 1)[1]: v for k, v in g.items() if k.startswith(tag + "__")}


def test_fixture_holds_every_variant(golden):
    g = golden(FIXTURE)
    assert sorted(str(v) for v in g["variants"]) == sorted(VARIANTS)
    for tag, (_, conv) in VARIANTS.items():
        assert str(g[f"{tag}__convention"]) == conv, tag


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kernel_text_equals_the_oracle(variant, golden):
    conv = VARIANTS[variant][1]
    text = _text(golden, variant)
    clouds = golden("g1_g2_ops.npz")["clouds"]  # REAL275-shaped surfaces, a tiled-duplicate cloud, an exact-grid-tie cloud
    odd = np.ascontiguousarray(golden("g1_g2_ops.npz")["odd_clouds"])
    assert int(text["opt_n_threads_700"]) == ops.opt_n_threads(700) == 512
    with ops.use_arith(conv):
        cur = clouds
        for lvl, (npnt, radii) in enumerate(zip([512, 256, 128], [[0.02, 0.04], [0.04, 0.08], [0.08, 0.16]])):
            ref, ref_t = ops.furthest_point_sampling(cur, npnt)
            assert np.array_equal(text[f"fps_idx{lvl}"], ref), f"FPS level {lvl} under {conv}"
            assert np.array_equal(text[f"fps_temp{lvl}"], ref_t)
            new = np.ascontiguousarray(np.take_along_axis(cur, ref[:, :, None].astype(np.int64), axis=1))
            for r, ns in zip(radii, [16, 32]):
                assert sha(ops.ball_query(r, ns, cur, new)) == str(text[f"bq{lvl}_{ns}_sha"]), f"ball query level {lvl} r={r}"
            cur = new
        # n not a power of two: threads own several points (k = tid, tid + S, ...), S = 512 < n = 700
        ref, ref_t = ops.furthest_point_sampling(odd, 60)
        assert np.array_equal(text["odd_fps_idx"], ref) and np.array_equal(text["odd_fps_temp"], ref_t)
        # three_nn (double best-distances, strict <) and three_interpolate
        unk, kn = np.ascontiguousarray(clouds[:2, :300]), np.ascontiguousarray(clouds[:2, 300:364])
        rd, ri = ops.three_nn(unk, kn)
        assert np.array_equal(text["nn_idx"], ri) and np.array_equal(text["nn_dist2"], rd)
        g = golden(FIXTURE)
        assert np.array_equal(text["interp_out"], ops.three_interpolate(g["interp_feats"], ri, g["interp_w"]))


def test_no_host_compiler_produces_convention_A(golden):
    """The round-1..4 default (A: the FIRST product rounded on its own) is what neither g++ nor clang++ make of the text: on the golden
    clouds the contracted text picks B's centres, and those differ from A's."""
    clouds = golden("g1_g2_ops.npz")["clouds"]
    a = ops.furthest_point_sampling(clouds, 512, arith="A")[0]
    b = ops.furthest_point_sampling(clouds, 512, arith="B")[0]
    assert not np.array_equal(a, b)
    for tag in ("gxx_fma", "clang_fma"):
        got = _text(golden, tag)["fps_idx0"]
        assert np.array_equal(got, b) and not np.array_equal(got, a)
