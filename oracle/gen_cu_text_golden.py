"""ORACLE — TEST INFRASTRUCTURE ONLY; runs ONLY in the build container (needs the reference tree, g++ and an FMA-capable host).

Generates tests/golden/g17_cu_text.npz, the fixture of tests/test_cu_text_emulation.py:

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.gen_cu_text_golden

The TEXT of the reference's CUDA kernels - sampling_gpu.cu (furthest point sampling incl. its shared-memory tree), ball_query_gpu.cu,
interpolate_gpu.cu (three_nn, three_interpolate) - is extracted into a temporary directory, compiled by the HOST compilers against
oracle/cu_emul/cuda_model.h (every CUDA thread a cooperative fiber, __syncthreads() a round-robin barrier) and run on the golden clouds
of g1_g2_ops.npz, once per compiler / contraction variant.  Only the OUTPUTS are stored (data: indices, distances, weights; the ball
queries as SHA-256 digests of their int32 index arrays, like g1_g2_ops.npz); nothing of the reference's text is committed.

One edit is applied to the extracted text: a `__syncthreads();` after `old = dists_i[0];` (sampling_gpu.cu:205).  The kernel has a
benign read/write race there (a fast thread of iteration j+1 may overwrite dists_i[0] before a slow thread of iteration j has read
it) that lock-step warps do not lose; a sequential scheduler always would.
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

from oracle.ref_import import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REF, "networks", "pts_encoder", "pointnet2_utils", "pointnet2", "src")
EMU = os.path.join(ROOT, "oracle", "cu_emul")
GOLDEN = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLDEN, "g17_cu_text.npz")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

VARIANTS = {
    # tag: (compiler, flags, the oracle convention the text must reproduce)
    "gxx_off": ("g++", ["-ffp-contract=off"], "C"),
    "gxx_fma": ("g++", ["-mfma", "-ffp-contract=fast"], "B"),
    "clang_fma": (CLANG, ["-mfma", "-ffp-contract=fast"], "B"),
    "clang_default": (CLANG, ["-mfma"], "B"),  # clang's default -ffp-contract=on (front-end fmuladd): the same fusion
}
LEVELS = [(512, [0.02, 0.04]), (256, [0.04, 0.08]), (128, [0.08, 0.16])]  # (centres, ball radii) of the three sampled levels
NSAMPLE = [16, 32]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _extract(path, start_marker, end_marker):
    """Lines from the one that starts with start_marker up to (not including) the one that starts with end_marker."""
    lines = open(path).read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.startswith(start_marker))
    b = next(i for i, l in enumerate(lines) if i > a and l.startswith(end_marker))
    return "\n".join(lines[a:b]) + "\n"


def write_kernel_text(d):
    fps = _extract(os.path.join(SRC, "sampling_gpu.cu"), "__device__ void __update", "void furthest_point_sampling_kernel_launcher")
    race = "old = dists_i[0];"
    assert fps.count(race) == 1
    fps = fps.replace(race, race + "\n    __syncthreads(); /* generation-time edit, see the module docstring */")
    parts = {
        "fps_kernel.inc": fps,
        "ball_query_kernel.inc": _extract(os.path.join(SRC, "ball_query_gpu.cu"), "__global__ void ball_query_kernel_fast",
                                          "void ball_query_kernel_launcher_fast"),
        "three_nn_kernel.inc": _extract(os.path.join(SRC, "interpolate_gpu.cu"), "__global__ void three_nn_kernel_fast",
                                        "void three_nn_kernel_launcher_fast"),
        "three_interpolate_kernel.inc": _extract(os.path.join(SRC, "interpolate_gpu.cu"), "__global__ void three_interpolate_kernel_fast",
                                                 "void three_interpolate_kernel_launcher_fast"),
    }
    for name, text in parts.items():
        with open(os.path.join(d, name), "w") as f:
            f.write(text)


def build(d, tag, cxx, flags):
    so = os.path.join(d, f"libcu_emul_{tag}.so")
    cmd = [cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-fno-fast-math", "-w", f"-I{d}", f"-I{EMU}",
           f'-DEMU_CUDA_UTILS_H="{SRC}/cuda_utils.h"'] + flags + ["-o", so, os.path.join(EMU, "driver.cpp")]
    subprocess.check_call(cmd)
    return ctypes.CDLL(so)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def emu_fps(lib, xyz, m):
    B, N, _ = xyz.shape
    temp = np.full((B, N), 1e10, np.float32)
    idx = np.zeros((B, m), np.int32)
    lib.emu_fps(B, N, m, _p(xyz), _p(temp), _p(idx))
    return idx, temp


def run_variant(lib, clouds, odd, feats, w):
    """Everything tests/test_cu_text_emulation.py compares against the oracle, as the kernel text computes it."""
    out = {"opt_n_threads_700": np.int32(lib.emu_opt_n_threads(700))}
    cur = clouds
    for lvl, (npnt, radii) in enumerate(LEVELS):
        idx, temp = emu_fps(lib, cur, npnt)
        out[f"fps_idx{lvl}"], out[f"fps_temp{lvl}"] = idx.astype(np.int16), temp
        new = np.ascontiguousarray(np.take_along_axis(cur, idx[:, :, None].astype(np.int64), axis=1))
        for r, ns in zip(radii, NSAMPLE):
            bq = np.zeros((cur.shape[0], npnt, ns), np.int32)
            lib.emu_ball_query(cur.shape[0], cur.shape[1], npnt, ctypes.c_float(r), ns, _p(new), _p(cur), _p(bq))
            out[f"bq{lvl}_{ns}_sha"] = np.array(sha(bq))
        cur = new
    idx, temp = emu_fps(lib, odd, 60)
    out["odd_fps_idx"], out["odd_fps_temp"] = idx.astype(np.int16), temp
    unk, kn = np.ascontiguousarray(clouds[:2, :300]), np.ascontiguousarray(clouds[:2, 300:364])
    d2 = np.zeros((2, 300, 3), np.float32)
    i3 = np.zeros((2, 300, 3), np.int32)
    lib.emu_three_nn(2, 300, 64, _p(unk), _p(kn), _p(d2), _p(i3))
    out["nn_dist2"], out["nn_idx"] = d2, i3.astype(np.int16)
    o = np.zeros((2, 7, 300), np.float32)
    lib.emu_three_interpolate(2, 7, 64, 300, _p(feats), _p(i3), _p(w), _p(o))
    out["interp_out"] = o
    return out


def _has_fma():
    try:
        return " fma " in open("/proc/cpuinfo").read()
    except OSError:
        return False


def main():
    if not (os.path.isdir(SRC) and shutil.which("g++") and _has_fma()):
        print("needs the reference tree, g++ and an FMA-capable host (build container only)", file=sys.stderr)
        return 1
    g = np.load(os.path.join(GOLDEN, "g1_g2_ops.npz"))
    clouds, odd = np.ascontiguousarray(g["clouds"]), np.ascontiguousarray(g["odd_clouds"])
    feats = np.random.default_rng(5).standard_normal((2, 7, 64)).astype(np.float32)
    w = np.random.default_rng(6).uniform(size=(2, 300, 3)).astype(np.float32)
    data = {"interp_feats": feats, "interp_w": w, "variants": np.array(list(VARIANTS))}
    with tempfile.TemporaryDirectory() as d:
        write_kernel_text(d)
        for tag, (cxx, flags, conv) in VARIANTS.items():
            data[f"{tag}__convention"] = np.array(conv)
            for k, v in run_variant(build(d, tag, cxx, flags), clouds, odd, feats, w).items():
                data[f"{tag}__{k}"] = v
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
