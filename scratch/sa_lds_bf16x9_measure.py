"""Stand-alone timing of encoder level 1 (both scales, from the fp32 hoisted features): the fp32 kernels (gp_sa_pre_mlp_max_layout) against
gp_sa_lds_bf16x9, alternating in one process, HIP events, 2 warm-ups + 11 repeats per batch size; median [min, max] in us.

    python scratch/sa_lds_bf16x9_measure.py [--clouds 640 320 128 64 5] [--libs tag=path ...]

--libs: tuning builds of the library (GP_BUILD_TAG=<tag> GP_EXTRA_FLAGS='-DSALX9_...' python -m genpose_amd.build) whose gp_sa_lds_bf16x9 is
timed beside the shipped one (workgroup geometry candidates)."""
import argparse
import ctypes
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[640, 320, 128, 64, 5])
    ap.add_argument("--libs", nargs="*", default=[])
    ap.add_argument("--repeats", type=int, default=11)
    a = ap.parse_args()
    from genpose_amd import _lib, synth
    from genpose_amd._lib import ptr, stream_ptr
    from genpose_amd.encoder import Pointnet2EncoderHIP
    from oracle import genpose_oracle as go
    sd = go.make_state_dict(0, "score")
    e = Pointnet2EncoderHIP(sd, "cuda")
    libs = {"shipped": _lib.lib()}
    for spec in a.libs:
        tag, path = spec.split("=", 1)
        L = ctypes.CDLL(path)
        L.gp_sa_lds_bf16x9.argtypes = _lib.SIGNATURES["gp_sa_lds_bf16x9"]
        L.gp_sa_lds_bf16x9.restype = ctypes.c_int
        libs[tag] = L
    scales = e.w.levels[1]
    nss = e.cfg["nsamples"][1]
    print(f"# level 1 alone, us, median [min, max] of {a.repeats} after 2 warm-ups; columns: fp32 kernels, then gp_sa_lds_bf16x9 of each library")
    for B in a.clouds:
        pts = torch.from_numpy(synth.make_batch(min(B, 24), start=100)).cuda().float()
        pts = pts[torch.arange(B, device="cuda") % pts.shape[0]].contiguous()
        _, ws = e.forward(pts, return_intermediates=True)
        xyz, cen, z, idx, ref = ws["new_xyz"][0], ws["new_xyz"][1], ws["z"][1], ws["bq"][1], ws["feat"][1].clone()
        out = torch.empty_like(ref)

        def head(i):
            sc = scales[i]
            return (B, 512, 256, nss[i], *sc.couts, ptr(xyz), ptr(cen), ptr(idx[i]), ptr(z), 128, 64 * i, ptr(sc.wxyz), ptr(sc.layers[0][1]))

        def f32(i):
            sc = scales[i]
            (_, _), (w2, b2), (w3, b3) = sc.layers
            _lib.call("gp_sa_pre_mlp_max_layout", sc.hidden_layout, *head(i), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 256, 128 * i, stream_ptr())

        def x9(L):
            def run(i):
                w2, b2, w3, b3 = scales[i].bf16x9_lds_packs()
                rc = L.gp_sa_lds_bf16x9(*head(i), ptr(w2), ptr(b2), ptr(w3), ptr(b3), ptr(out), 256, 128 * i, stream_ptr())
                if rc:
                    raise RuntimeError(f"gp_sa_lds_bf16x9 -> {rc}")
            return run

        arms = [("fp32", f32)] + [(t, x9(L)) for t, L in libs.items()]
        times = {(t, i): [] for t, _ in arms for i in (0, 1)}
        for rep in range(2 + a.repeats):
            for t, fn in arms:  # the arms alternate
                for i in (0, 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn(i)
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        times[(t, i)].append(e0.elapsed_time(e1) * 1e3)
            if rep == 0:  # sanity: the last arm's output against the fp32 features
                torch.cuda.synchronize()
                err = float((out - ref).abs().max()) / float(ref.abs().max())
                assert err < 1e-5, err
        for t, _ in arms:
            both = [x + y for x, y in zip(times[(t, 0)], times[(t, 1)])]
            cells = [f"{statistics.median(v):8.1f} [{min(v):7.1f}, {max(v):7.1f}]" for v in (times[(t, 0)], times[(t, 1)], both)]
            print(f"clouds {B:4d}  {t:10s}  ns16 64-64-128 {cells[0]}   ns32 64-96-128 {cells[1]}   both {cells[2]}", flush=True)


if __name__ == "__main__":
    main()
