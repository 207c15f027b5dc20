"""Energy ranking + top-k aggregation on the device (csrc/rank.hip), and the consensus ranker (ours): an "energy" array that needs no
network - every candidate scored by its mean distance to the cloud's other candidates.
Reference: networks/reward.py:131-155 (sort_poses_by_energy), utils/sgpa_utils.py:897-954 (sort_sRT_by_energy,
'average'), runners/evaluation_tracking.py:60-77 (cal_average_sRT)."""
import torch

from . import _lib, rotation
from ._lib import ptr, stream_ptr


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


def sort_poses_by_energy(poses, energy):
    """Same contract as networks/reward.py:131-155 -> (sorted_poses [B,K,9], sorted_energy [B,K,2])."""
    r = rank_aggregate(poses, energy)
    return r["sorted_poses"], r["sorted_energy"]


def cal_average_sRT(poses_sorted_or_unsorted, energy, selected_num):
    """Aggregated 4x4 pose from the top `selected_num` candidates (evaluation_tracking.py:60-77 semantics).
    Takes the UNSORTED 9-D poses + energies (ranking happens in the same launch) -> [B,4,4] f32."""
    r = rank_aggregate(poses_sorted_or_unsorted, energy, selected_num=selected_num)
    return rotation.quat_trans_to_RT(r["avg_pose"])
