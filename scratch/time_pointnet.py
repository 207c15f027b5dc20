"""Times the vanilla PointNet encoder pass (genpose_amd/pointnet_encoder.py) against the same network as stock torch on the same device.

    python scratch/time_pointnet.py [--clouds 320] [--points 1024] [--out FILE]       timing (HIP events)
    rocprofv3 --kernel-trace --stats -d DIR -- python scratch/time_pointnet.py --profile   kernel table: the HIP pass only, run of its own

HIP events around one pass, 5 warm-ups, median [min, max] of 9 repeats in one session.  Executed FLOPs are computed from the layer
widths (2 * Cin * Cout per point and layer, plus the head); the fp32 MFMA peak is 157.3 TFLOP/s (MI355X).  Also prints the distance of
the HIP result and of torch's own fp32 result on the device to the float64 restatement (first 4 clouds)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from genpose_amd import synth  # noqa: E402
from genpose_amd.pointnet_encoder import PointNetEncoderHIP  # noqa: E402
from genpose_amd.weights_synth import make_state_dict  # noqa: E402

PEAK_F32_MFMA = 157.3e12
STN_CONV = ((3, 64), (64, 128), (128, 1024))
TRUNK = ((3, 64), (64, 128), (128, 512), (512, 1024))
HEAD = ((1024, 512), (512, 256), (256, 9))


def flops(clouds, n):
    per_point = lambda layers: sum(2 * a * b for a, b in layers)
    return {"stn_pool": clouds * n * per_point(STN_CONV), "feat_pool": clouds * n * (per_point(TRUNK) + 2 * 9), "head": clouds * per_point(HEAD)}


def pointnet_torch(sd, pts, prefix="pts_encoder.", dtype=torch.float32):
    """PointNetfeat (networks/pts_encoder/pointnets.py:45-118) as plain torch, points as rows (the restatement of tests/test_pointnet_host.py)."""
    r = torch.relu
    w = {k: v.to(pts.device, dtype) for k, v in sd.items() if k.startswith(prefix)}
    lin = lambda x, name: x @ w[prefix + name + ".weight"].reshape(w[prefix + name + ".weight"].shape[0], -1).T + w[prefix + name + ".bias"]
    x = pts.to(dtype)
    g = r(lin(r(lin(r(lin(x, "stn.conv1")), "stn.conv2")), "stn.conv3")).max(dim=1)[0]
    trans = (lin(r(lin(r(lin(g, "stn.fc1")), "stn.fc2")), "stn.fc3") + torch.eye(3, dtype=dtype, device=pts.device).reshape(9)).view(-1, 3, 3)
    y = torch.bmm(x, trans)
    return lin(r(lin(r(lin(r(lin(y, "conv1")), "conv2")), "conv3")), "conv4").max(dim=1)[0]


def timed(fn, warmup=5, repeats=9):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, default=320)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--profile", action="store_true", help="the HIP pass only, 5 + 9 times (for rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sd = make_state_dict(0, "score", pts_encoder="pointnet")
    pts = torch.from_numpy(synth.make_batch(a.clouds)[:, :a.points].copy()).cuda()
    enc = PointNetEncoderHIP(sd, "cuda")
    if a.profile:
        timed(lambda: enc.forward(pts))
        return
    fl = flops(a.clouds, a.points)
    res = {"clouds": a.clouds, "points": a.points, "flops": fl, "flops_total": sum(fl.values()),
           "hip_forward": timed(lambda: enc.forward(pts)), "hip_encode_graph": timed(lambda: enc.encode(pts)),
           "torch_fp32_same_device": timed(lambda: pointnet_torch(sd, pts))}
    for k in ("hip_forward", "hip_encode_graph", "torch_fp32_same_device"):
        res[k]["tflops"] = res["flops_total"] / (res[k]["median_ms"] * 1e-3) / 1e12
        res[k]["fraction_of_fp32_mfma_peak"] = res[k]["tflops"] * 1e12 / PEAK_F32_MFMA
    ref64 = pointnet_torch(sd, pts[:4].cpu(), dtype=torch.float64)
    res["max_abs_diff_to_float64"] = {"hip": float((enc.forward(pts[:4]).cpu().double() - ref64).abs().max()),
                                      "torch_fp32_same_device": float((pointnet_torch(sd, pts[:4]).cpu().double() - ref64).abs().max()),
                                      "torch_fp32_cpu": float((pointnet_torch(sd, pts[:4].cpu()).double() - ref64).abs().max())}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
