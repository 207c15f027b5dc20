"""Energy ranking + top-k aggregation on the device (csrc/rank.hip), the consensus ranker (ours): an "energy" array that needs no
network - every candidate scored by its mean distance to the cloud's other candidates - and the mode-seeking aggregation (ours): a kernel
density over the candidates and a mean shift from the densest one, in place of the mean over the selected candidates.
Reference: networks/reward.py:131-155 (sort_poses_by_energy), utils/sgpa_utils.py:897-954 (sort_sRT_by_energy,
'average'), runners/evaluation_tracking.py:60-77 (cal_average_sRT)."""
import math

import torch

from . import _lib, rotation
from ._lib import ptr, stream_ptr

# mode_aggregate's defaults: the bandwidths (degrees, metres) and the iteration count of the synthetic prototype (clouds of 50 candidates
# with 70 % / 50 % inliers and a 30 + 20 bimodal set: the mode lay within 1.6 deg / 3.6 mm, the last iteration moved it by < 1e-7 deg).
# They are NOT tuned on the accuracy proxy or on REAL275.
MODE_BW_ROT_DEG, MODE_BW_TRANS, MODE_ITERS = 10.0, 0.02, 8


def rank_aggregate(poses, energy, ratio=None, selected_num=None, with_rt=False):
    """poses [B,K,9] (f32 or f64, device), energy [B,K,2] f32 ->
    dict(sorted_poses, sorted_energy, order [B,K,2] i32, avg_pose [B,7] f32 (w,x,y,z,t) or None).
    with_rt: the same launch also writes sorted_RTs [B,K,4,4] f64 (= rotation.pose9_to_RT(sorted_poses)) and, when aggregating,
    avg_RT [B,4,4] f32 (= rotation.quat_trans_to_RT(avg_pose)) - what the runners hand on (gp_rank_aggregate_rt)."""
    _lib.check_device()
    B, K, _ = poses.shape
    if poses.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("poses must be float32 or float64")
    poses = poses.contiguous()
    energy = energy.contiguous().float()
    sel = 0
    if selected_num is not None:
        sel = int(selected_num)
    elif ratio is not None:
        sel = max(1, int(K * ratio))
    out = {"sorted_poses": torch.empty_like(poses), "sorted_energy": torch.empty_like(energy),
           "order": torch.empty(B, K, 2, dtype=torch.int32, device=poses.device),
           "avg_pose": torch.empty(B, 7, device=poses.device) if sel > 0 else None}
    if with_rt:
        out["sorted_RTs"] = torch.empty(B, K, 4, 4, dtype=torch.float64, device=poses.device)
        out["avg_RT"] = torch.empty(B, 4, 4, device=poses.device) if sel > 0 else None
        _lib.call("gp_rank_aggregate_rt", B, K, sel, 1 if poses.dtype == torch.float64 else 0, ptr(poses), ptr(energy), ptr(out["sorted_poses"]),
                  ptr(out["sorted_energy"]), ptr(out["order"]), ptr(out["avg_pose"]), ptr(out["sorted_RTs"]), ptr(out["avg_RT"]), stream_ptr())
        return out
    _lib.call("gp_rank_aggregate", B, K, sel, 1 if poses.dtype == torch.float64 else 0, ptr(poses), ptr(energy), ptr(out["sorted_poses"]),
              ptr(out["sorted_energy"]), ptr(out["order"]), ptr(out["avg_pose"]), stream_ptr())
    return out


def _sym_arg(sym, B, device):
    """sym: None or [B] (bool / int, any device) -> int8 device tensor or None (no cloud symmetric)."""
    if sym is None:
        return None
    sym = torch.as_tensor(sym)
    if sym.shape != (B,):
        raise ValueError(f"sym must hold one flag per cloud ([{B}]), got {tuple(sym.shape)}")
    if sym.dtype == torch.int8 and sym.device == device:
        return sym.contiguous()  # (a tracker's static flags: used as they are, nothing launched)
    return (sym != 0).to(device=device, dtype=torch.int8).contiguous()


def _check_consensus(poses):
    if poses.dim() != 3 or poses.shape[2] != 9:
        raise ValueError(f"poses must be [B,K,9], got {tuple(poses.shape)}")
    if poses.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("poses must be float32 or float64")
    if not 1 <= poses.shape[1] <= _lib.CONSENSUS_MAX_K:
        raise ValueError(f"the consensus ranker serves 1..{_lib.CONSENSUS_MAX_K} candidates per cloud, got {poses.shape[1]}")


def consensus_energy(poses, sym=None):
    """poses [B,K,9] (f32 or f64, device) -> [B,K,2] f32 consensus scores (gp_consensus_energy): minus the mean geodesic angle (column 0) and
    minus the mean Euclidean translation distance (column 1) to the cloud's other finite candidates, accumulated in float64; a non-finite
    candidate scores -inf.  sym [B] (optional): clouds of objects symmetric about their y axis compare the y axes only.  The array ranks
    through rank_aggregate like the energy model's: higher = first."""
    _check_consensus(poses)
    B, K, _ = poses.shape
    poses = poses.contiguous()
    sym = _sym_arg(sym, B, poses.device)
    _lib.check_device()
    out = torch.empty(B, K, 2, device=poses.device)
    _lib.call("gp_consensus_energy", B, K, 1 if poses.dtype == torch.float64 else 0, ptr(poses), ptr(sym), ptr(out), stream_ptr())
    return out


def consensus_rank_aggregate(poses, sym=None, ratio=None, selected_num=None, with_rt=False):
    """consensus_energy followed by rank_aggregate in ONE launch (gp_consensus_rank_aggregate_rt), bit for bit the two calls: rank_aggregate's
    dict plus "energy" [B,K,2] f32."""
    _check_consensus(poses)
    B, K, _ = poses.shape
    poses = poses.contiguous()
    sym = _sym_arg(sym, B, poses.device)
    _lib.check_device()
    sel = 0
    if selected_num is not None:
        sel = int(selected_num)
    elif ratio is not None:
        sel = max(1, int(K * ratio))
    dev = poses.device
    out = {"energy": torch.empty(B, K, 2, device=dev), "sorted_poses": torch.empty_like(poses), "sorted_energy": torch.empty(B, K, 2, device=dev),
           "order": torch.empty(B, K, 2, dtype=torch.int32, device=dev), "avg_pose": torch.empty(B, 7, device=dev) if sel > 0 else None}
    if with_rt:
        out["sorted_RTs"] = torch.empty(B, K, 4, 4, dtype=torch.float64, device=dev)
        out["avg_RT"] = torch.empty(B, 4, 4, device=dev) if sel > 0 else None
    _lib.call("gp_consensus_rank_aggregate_rt", B, K, sel, 1 if poses.dtype == torch.float64 else 0, ptr(poses), ptr(sym), ptr(out["energy"]),
              ptr(out["sorted_poses"]), ptr(out["sorted_energy"]), ptr(out["order"]), ptr(out["avg_pose"]), ptr(out.get("sorted_RTs")),
              ptr(out.get("avg_RT")), stream_ptr())
    return out


def selection_weight(order, sel):
    """rank_aggregate's order [B,K,2] (candidate index at each rank) and sel -> [B,K,2] f32: 1 for the candidates among a column's first
    `sel` ranks, else 0 - what the mean aggregates, as mode_aggregate's weight.  On the device, nothing read back."""
    B, K, _ = order.shape
    sel = int(sel)
    if not 1 <= sel <= K:
        raise ValueError(f"sel must lie in 1..{K}, got {sel}")
    w = torch.zeros(B, K, 2, dtype=torch.float32, device=order.device)
    return w.scatter_(1, order[:, :sel].long(), 1.0)


def mode_aggregate(poses, sym=None, weight=None, bw_rot_deg=MODE_BW_ROT_DEG, bw_trans=MODE_BW_TRANS, iters=MODE_ITERS, with_rt=False):
    """poses [B,K,9] (f32 or f64, device) -> dict(density [B,K,2] f32, mode_pose [B,7] f32 (w,x,y,z,t), mass [B,2] f32, start [B,2] i32,
    mode_RT [B,4,4] f32 = rotation.quat_trans_to_RT(mode_pose) with with_rt, else None), one launch (gp_mode_aggregate; the definition is in
    include/genpose_hip.h, section D).  Rotation (column 0) and translation (column 1) independently: `density` is a Gaussian kernel density
    over the cloud's candidates (bandwidths bw_rot_deg degrees of geodesic angle and bw_trans metres; it ranks through rank_aggregate like
    an energy array: higher = first), `start` the densest weighted candidate, `mode_pose` where `iters` mean-shift steps from it arrive and
    `mass` the weighted share of the candidates under the kernel there - a confidence in [0, 1].  sym [B] (optional): clouds of objects
    symmetric about their y axis compare the y axes only.  weight [B,K,2] f32 (optional; default all ones): a candidate counts with its
    weight where that is > 0 (selection_weight makes the 0/1 weight of a ranking's first `sel` candidates)."""
    _check_consensus(poses)
    B, K, _ = poses.shape
    if not (math.isfinite(bw_rot_deg) and bw_rot_deg > 0 and math.isfinite(bw_trans) and bw_trans > 0):
        raise ValueError(f"the bandwidths must be finite and > 0, got {bw_rot_deg} deg and {bw_trans} m")
    if int(iters) != iters or not 0 <= iters <= _lib.MODE_MAX_ITERS:
        raise ValueError(f"iters must be an integer in 0..{_lib.MODE_MAX_ITERS}, got {iters}")
    poses = poses.contiguous()
    sym = _sym_arg(sym, B, poses.device)
    if weight is not None:
        if weight.shape != (B, K, 2):
            raise ValueError(f"weight must hold one pair per candidate ([{B},{K},2]), got {tuple(weight.shape)}")
        weight = weight.to(device=poses.device, dtype=torch.float32).contiguous()
    _lib.check_device()
    dev = poses.device
    out = {"density": torch.empty(B, K, 2, device=dev), "mode_pose": torch.empty(B, 7, device=dev), "mass": torch.empty(B, 2, device=dev),
           "start": torch.empty(B, 2, dtype=torch.int32, device=dev), "mode_RT": torch.empty(B, 4, 4, device=dev) if with_rt else None}
    _lib.call("gp_mode_aggregate", B, K, 1 if poses.dtype == torch.float64 else 0, ptr(poses), ptr(sym), ptr(weight), math.radians(bw_rot_deg),
              float(bw_trans), int(iters), ptr(out["density"]), ptr(out["mode_pose"]), ptr(out["mode_RT"]), ptr(out["mass"]), ptr(out["start"]),
              stream_ptr())
    return out


def cloud_extent(pts, rt, trim=0, sym=None):
    """pts [B,n,3] f32 (device), rt [B,4,4] f32 (object -> camera: avg_RT's layout) -> half [B,3] f32 (gp_cloud_extent; ours, no counterpart
    in the reference): per cloud and object axis j the (trim + 1)-th largest |q_j| over its points, q = R^T (p - t) in the float32 operation
    order of include/genpose_hip.h - exactly a value of the array, np.sort's bits.  trim = 0: the maximum.  sym [B] (optional): objects
    symmetric about their y axis measure the radius sqrt(q_0^2 + q_2^2) into columns 0 and 2.  2 * half is the object's size in a frame
    centred on it.  One launch, nothing read back."""
    if pts.dim() != 3 or pts.shape[2] != 3 or pts.dtype != torch.float32:
        raise ValueError(f"pts must be float32 [B,n,3], got {pts.dtype} {tuple(pts.shape)}")
    B, n, _ = pts.shape
    if tuple(rt.shape) != (B, 4, 4) or rt.dtype != torch.float32:
        raise ValueError(f"rt must be float32 [{B},4,4], got {rt.dtype} {tuple(rt.shape)}")
    if not 1 <= n <= _lib.EXTENT_MAX_N:
        raise ValueError(f"cloud_extent serves clouds of 1..{_lib.EXTENT_MAX_N} points, got {n}")
    if int(trim) != trim or not 0 <= trim < n:
        raise ValueError(f"trim must be an integer in 0..{n - 1}, got {trim}")
    sym = _sym_arg(sym, B, pts.device)
    if pts.device.type != "cuda" or rt.device != pts.device:
        raise ValueError(f"pts and rt must be on one GPU, got {pts.device} and {rt.device}")
    pts, rt = pts.contiguous(), rt.contiguous()
    _lib.check_device()
    out = torch.empty(B, 3, device=pts.device)
    if B:
        _lib.call("gp_cloud_extent", B, n, ptr(pts), ptr(rt), int(trim), ptr(sym), ptr(out), stream_ptr())
    return out


def sort_poses_by_energy(poses, energy):
    """Same contract as networks/reward.py:131-155 -> (sorted_poses [B,K,9], sorted_energy [B,K,2])."""
    r = rank_aggregate(poses, energy)
    return r["sorted_poses"], r["sorted_energy"]


def cal_average_sRT(poses_sorted_or_unsorted, energy, selected_num):
    """Aggregated 4x4 pose from the top `selected_num` candidates (evaluation_tracking.py:60-77 semantics).
    Takes the UNSORTED 9-D poses + energies (ranking happens in the same launch) -> [B,4,4] f32."""
    r = rank_aggregate(poses_sorted_or_unsorted, energy, selected_num=selected_num)
    return rotation.quat_trans_to_RT(r["avg_pose"])
