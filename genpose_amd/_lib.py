"""ctypes binding of libgenpose_hip.so (the C ABI of include/genpose_hip.h).

There is NO CPU fallback: if the library is missing or a call fails, the caller gets an exception.
`lib()` only dlopens (safe without a GPU); `check_device()` verifies the device is gfx950.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# GENPOSE_HIP_LIB: tuning only (a variant built with GP_BUILD_TAG=<tag> beside the shipped library, genpose_amd/build.py)
SO_PATH = os.environ.get("GENPOSE_HIP_LIB") or os.path.join(_HERE, "lib", "libgenpose_hip.so")

c_int, c_float, c_void_p, c_int64 = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64
P = c_void_p
PLAN_SHARED = 0x200     # GP_PLAN_SHARED: the RK45 driver's shared-chunk plan (16 | or 48 |), see include/genpose_hip.h
PLAN_FLAGS = 0x300
RK45_MODEL_LIKELIHOOD_EXACT = 4  # GP_RK45_MODEL_LIKELIHOOD_EXACT: the likelihood ODE with the exact divergence (3 stays an unknown model)
CONSENSUS_MAX_K = 512   # GP_CONSENSUS_MAX_K: the largest candidate count the consensus ranker's LDS layout serves
EXTENT_MAX_N = 4096    # GP_EXTENT_MAX_N: the largest cloud gp_cloud_extent keeps in a wave's registers
MODE_MAX_ITERS = 64    # GP_MODE_MAX_ITERS: the most mean-shift iterations gp_mode_aggregate runs
PLAN_HEADSPLIT = 0x100  # GP_PLAN_HEADSPLIT (include/genpose_hip.h): OR-ed onto a 16-row tile plan = three workgroups per tile, one head each


class GpScoreNet(ctypes.Structure):
    """struct gp_scorenet (include/genpose_hip.h)."""
    _fields_ = [(n, c_void_p) for n in ("w_pose0", "b_pose0", "w_pose2", "b_pose2", "w_headx", "w_out", "b_out", "fourier_w",
                                        "w_t1", "b_t1", "w_headt", "w_headp", "b_head", "w_headx_t", "w_pose2_t", "w_pose0_t")]


NETP = ctypes.POINTER(GpScoreNet)


def seed_words(seed, run=0, base=0):
    """The Philox seed state the kernels read (csrc/philox.h) -> np.uint32 [8]: seed lo, seed hi, run, 0, row base lo, row base hi, 0, 0 -
    the little-endian words of the uint64s [seed mod 2^64, run, base, 0], so .view(np.int64) is the same state for an int64 [4] tensor."""
    seed, run, base = int(seed) % (1 << 64), int(run), int(base)
    if not 0 <= run < (1 << 32):
        raise ValueError(f"run_index {run}: 32 bits")
    if not 0 <= base < (1 << 63):
        raise ValueError(f"row_base {base}")
    return np.array([seed, run, base, 0], dtype="<u8").view(np.uint32)

# what every gp_rk45_phase* entry point takes behind its geometry: net, cvec, tvec, centre, state, y, ynew, K, partials, traj, traj_cap,
# t0, t_bound, rtol, atol, denoise_scale, do_denoise, nstates, x_out
RK45_SOLVE = [NETP] + [P] * 9 + [c_int] + [ctypes.c_double] * 5 + [c_int, c_int, P]

# name -> argtypes ; every function returns int (0 ok / negative GP_E*), except gp_pack_weight_size (int64)
SIGNATURES = {
    "gp_version": [],
    "gp_device_arch": [ctypes.c_char_p, c_int],
    "gp_arith_default": [],
    "gp_furthest_point_sampling": [c_int, c_int, c_int, P, P, P, P],
    "gp_furthest_point_sampling_arith": [c_int, c_int, c_int, c_int, P, P, P, P],
    "gp_ball_query_arith": [c_int, c_int, c_int, c_int, c_float, c_int, P, P, P, P],
    "gp_three_nn_arith": [c_int, c_int, c_int, c_int, P, P, P, P, P],
    "gp_three_interpolate_arith": [c_int, c_int, c_int, c_int, c_int, P, P, P, P, P],
    "gp_fps_chain_arith": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), P, P, P, P, P, P, P, P],
    "gp_ball_query_msg_fits": [c_int, c_int, c_int],
    "gp_ball_query_msg_arith": [c_int, c_int, c_int, c_int, c_float, c_int, c_float, c_int, P, P, P, P, P],
    "gp_gather_points": [c_int, c_int, c_int, c_int, P, P, P, P],
    "gp_gather_points_grad": [c_int, c_int, c_int, c_int, P, P, P, P],
    "gp_ball_query": [c_int, c_int, c_int, c_float, c_int, P, P, P, P],
    "gp_group_points": [c_int, c_int, c_int, c_int, c_int, P, P, P, P],
    "gp_group_points_grad": [c_int, c_int, c_int, c_int, c_int, P, P, P, P],
    "gp_three_nn": [c_int, c_int, c_int, P, P, P, P, P],
    "gp_three_interpolate": [c_int, c_int, c_int, c_int, P, P, P, P, P],
    "gp_three_interpolate_grad": [c_int, c_int, c_int, c_int, P, P, P, P, P],
    "gp_fps_chain": [c_int, c_int, c_int, ctypes.POINTER(c_int), P, P, P, P, P, P, P, P],
    "gp_ball_query_msg": [c_int, c_int, c_int, c_float, c_int, c_float, c_int, P, P, P, P, P],
    "gp_sa_mlp_max": [c_int] * 8 + [P] * 10 + [P, c_int, c_int, P],
    "gp_point_linear": [c_int, c_int, c_int, P, P, P, P],
    "gp_sa_pre_mlp_max": [c_int] * 7 + [P, P, P, P, c_int, c_int] + [P] * 7 + [c_int, c_int, P],
    "gp_sa_pre_mlp_max_layout": [c_int] * 8 + [P, P, P, P, c_int, c_int] + [P] * 7 + [c_int, c_int, P],
    "gp_sa_tail_position": [c_int, c_int],
    "gp_sa_pre_mlp_max_bf16x3": [c_int] * 7 + [P, P, P, P, c_int, c_int] + [P] * 7 + [c_int, c_int, P],
    "gp_sa_pre_mlp_max_bf16x9": [c_int] * 7 + [P, P, P, P, c_int, c_int] + [P] * 6 + [c_int, c_int, P],
    "gp_sa_lds_bf16x9": [c_int] * 7 + [P, P, P, P, c_int, c_int] + [P] * 7 + [c_int, c_int, P],
    "gp_sa_groupall_bf16x9": [c_int] * 5 + [P, P] + ([c_int] + [P] * 5 + [c_int]) * 2 + [P, c_int, P],
    "gp_pointnet_stn_pool": [c_int, c_int] + [P] * 8 + [P],
    "gp_pointnet_feat_pool": [c_int, c_int] + [P] * 11 + [P],
    "gp_dense_rows": [c_int, c_int, c_int, c_int, P, P, P, P, c_int, P, P],
    "gp_pack_weight_size": [c_int, c_int],
    "gp_pack_weight": [c_int, c_int, P, c_int, P],
    "gp_score_tile_rows": [c_int],
    "gp_cloud_embed": [c_int, NETP, P, P, P],
    "gp_time_embed": [c_int, NETP, P, P, P],
    "gp_score_eval": [c_int, c_int, NETP, P, P, P, P, c_int, P, P],
    "gp_pc_step": [c_int, c_int, c_int, c_int, NETP] + [P] * 11 + [P],
    "gp_roi_to_cloud": [c_int, c_int, c_int, c_int, P, P, P, c_float, c_float, c_float, c_float, P, P, P, P],
    "gp_cloud_sample": [c_int, c_int, c_int, P, P, P, P, P],
    "gp_roi_sample_seeded": [c_int] * 5 + [P, P, P] + [c_float] * 4 + [P] * 5 + [P],
    "gp_roi_sample_frames": [c_int] * 6 + [P, P, c_int64] + [P] * 4 + [c_float] * 4 + [P] * 5 + [P],
    "gp_cloud_extent": [c_int, c_int, P, P, c_int, P, P, P],
    "gp_box_sample_max_segments": [],
    "gp_box_sample": [c_int] * 5 + [P] * 4 + [c_float, c_float, c_int] + [c_float] * 4 + [P] * 5 + [P],
    "gp_score_div": [c_int, c_int, NETP, P, P, P, P, P, P, P, P],
    "gp_energy_score": [c_int, c_int, NETP, P, P, P, P, P, P, P],
    "gp_score_div_exact": [c_int, c_int, NETP, P, P, P, P, P, P, P],
    "gp_pc_tile_rows": [c_int, c_int, c_int],
    "gp_pc_layout": [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)],
    "gp_pc_step_plan": [c_int, c_int, c_int, c_int, c_int, c_int, c_int, NETP] + [P] * 12 + [c_int, P],
    "gp_score_eval_plan": [c_int, c_int, c_int, NETP, P, P, P, P, c_int, P, P],
    "gp_pc_layout_bf16x3": [c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "gp_pc_step_bf16x3": [c_int] * 5 + [P] * 18 + [P],
    "gp_pc_step_bf16x9": [c_int] * 5 + [NETP] + [P] * 12 + [c_int] + [P] * 3 + [P],
    "gp_pc_step_plan_seeded": [c_int] * 6 + [NETP] + [P] * 11 + [c_int, P],
    "gp_pc_step_bf16x9_seeded": [c_int] * 5 + [NETP] + [P] * 11 + [c_int] + [P] * 3 + [P],
    "gp_pc_step_bf16x6": [c_int] * 5 + [NETP] + [P] * 12 + [c_int] + [P] * 3 + [P],
    "gp_pc_step_bf16x6_seeded": [c_int] * 5 + [NETP] + [P] * 11 + [c_int] + [P] * 3 + [P],
    "gp_pc_noise_fill": [P, c_int, c_int, c_int64, c_int64, P, P, P],
    "gp_philox_raw": [c_int64, P, P, P, P],
    "gp_track_warm_start": [c_int, c_int] + [P] * 7 + [P],
    "gp_track_prior_fill": [P, c_int64, c_int64, P, P],
    "gp_heun_launches": [c_int, c_int],
    "gp_heun_layout": [c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "gp_heun_step_plan": [c_int] * 7 + [NETP] + [P] * 9 + [P],
    "gp_heun_step_bf16x9": [c_int] * 6 + [NETP] + [P] * 9 + [P] * 3 + [P],
    "gp_heun_solve_tile": [c_int] * 6 + [NETP] + [P] * 9 + [P],
    "gp_dpm2m_launches": [c_int, c_int],
    "gp_dpm2m_step_plan": [c_int] * 7 + [NETP] + [P] * 9 + [P],
    "gp_dpm2m_step_bf16x9": [c_int] * 6 + [NETP] + [P] * 9 + [P] * 3 + [P],
    "gp_dpm2m_solve_tile": [c_int] * 6 + [NETP] + [P] * 9 + [P],
    "gp_heun_layout_model": [c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "gp_heun_step_plan_model": [c_int] * 8 + [NETP] + [P] * 9 + [P],
    "gp_dpm2m_step_plan_model": [c_int] * 8 + [NETP] + [P] * 9 + [P],
    "gp_heun_solve_tile_model": [c_int] * 7 + [NETP] + [P] * 9 + [P],
    "gp_dpm2m_solve_tile_model": [c_int] * 7 + [NETP] + [P] * 9 + [P],
    "gp_heun_step_classes": [c_int] * 8 + [NETP] + [P] * 9 + [c_int, P] + [P],
    "gp_dpm2m_step_classes": [c_int] * 8 + [NETP] + [P] * 9 + [c_int, P] + [P],
    "gp_heun_solve_classes": [c_int] * 7 + [NETP] + [P] * 9 + [c_int, P] + [P],
    "gp_dpm2m_solve_classes": [c_int] * 7 + [NETP] + [P] * 9 + [c_int, P] + [P],
    "gp_track_start_classes": [c_int, c_int, P, P, c_int] + [P] * 6 + [c_int, P],
    "gp_heun_likelihood_launches": [c_int],
    "gp_heun_likelihood_step": [c_int] * 4 + [NETP] + [P] * 9 + [P],
    "gp_pc_step_grouped": [c_int, c_int, c_int, c_int, c_int, NETP] + [P] * 11 + [P],
    "gp_pc_step_coupled": [c_int, c_int, c_int, c_int, c_int, NETP] + [P] * 12 + [P],
    "gp_rk45_state_bytes": [],
    "gp_rk45_state_layout": [ctypes.POINTER(c_int64), c_int],
    "gp_rk45_set_dense": [P, P, c_int, P, P],
    "gp_rk45_phase": [c_int] * 3 + RK45_SOLVE + [P],
    "gp_rk45_phase_grouped": [c_int] * 4 + RK45_SOLVE + [P],
    "gp_rk45_plan_rows": [c_int, c_int, c_int, c_int],
    "gp_plan_headsplit_pays": [c_int],
    "gp_rk45_plan_rows_unshared": [c_int, c_int, c_int, c_int],
    "gp_rk45_partials_count": [c_int, c_int, c_int, c_int, c_int],
    "gp_rk45_phase_model": [c_int, c_int, P] + [c_int] * 4 + RK45_SOLVE + [P, c_int, P],
    "gp_rk45_phase_bf16x9": [c_int] * 4 + RK45_SOLVE + [P, c_int] + [P] * 3 + [P],
    "gp_rk45_set_dense_grouped": [c_int, P, P, c_int, P, P],
    "gp_rk45_phase_ragged": [c_int, c_int, P, c_int, P, c_int, c_int, c_int] + RK45_SOLVE + [P],
    "gp_time_embed_strided": [c_int, c_int, c_int64, NETP, P, P, P],
    "gp_rank_aggregate": [c_int, c_int, c_int, c_int, P, P, P, P, P, P, P],
    "gp_rank_aggregate_rt": [c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P],
    "gp_pose9_to_rt": [c_int, c_int, P, P, P],
    "gp_quat_trans_to_rt": [c_int, P, P, P],
    "gp_consensus_energy": [c_int, c_int, c_int, P, P, P, P],
    "gp_consensus_rank_aggregate_rt": [c_int, c_int, c_int, c_int] + [P] * 9 + [P],
    "gp_mode_aggregate": [c_int, c_int, c_int, P, P, P, ctypes.c_double, ctypes.c_double, c_int] + [P] * 5 + [P],
}
OPTIONAL = set()

_lib = None


class GenposeHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        import torch  # noqa: F401  torch's bundled libamdhip64.so.7 must be the process's HIP runtime (shared streams/pointers)
        if not os.path.exists(SO_PATH):
            raise GenposeHipError(
                f"{SO_PATH} is missing - build it with `python -m genpose_amd.build` (hipcc, gfx950). "
                "genpose_amd has no CPU fallback.")
        l = ctypes.CDLL(SO_PATH)
        for name, args in SIGNATURES.items():
            try:
                fn = getattr(l, name)
            except AttributeError:
                if name in OPTIONAL:
                    continue
                raise GenposeHipError(f"{SO_PATH} does not export {name} (stale build?)")
            fn.argtypes = args
            fn.restype = c_int64 if name in ("gp_pack_weight_size", "gp_rk45_state_bytes") else c_int
        _lib = l
    return _lib


_ERR = {-1: "GP_EINVAL (bad size / null pointer / unsupported shape)", -2: "GP_ELAUNCH (HIP launch failed)",
        -3: "GP_EARCH (device is not gfx950)"}


def check(rc, what):
    if rc != 0:
        raise GenposeHipError(f"{what} failed: {_ERR.get(rc, rc)}")


def call(name, *args):
    check(getattr(lib(), name)(*args), name)


_device_checked = False


def check_device():
    """Raise unless the current HIP device is gfx950 (MI355X)."""
    global _device_checked
    if _device_checked:
        return
    import torch
    if not torch.cuda.is_available():
        raise GenposeHipError("genpose_amd needs an MI355X (gfx950) device; torch.cuda.is_available() is False (no CPU fallback)")
    torch.cuda.init()
    buf = ctypes.create_string_buffer(64)
    rc = lib().gp_device_arch(buf, 64)
    if rc != 0:
        raise GenposeHipError(f"genpose_amd needs an MI355X (gfx950) device; found '{buf.value.decode()}' ({_ERR.get(rc, rc)})")
    _device_checked = True


def ptr(t):
    """Device (or host) pointer of a contiguous torch tensor; None -> NULL."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return c_void_p(t.data_ptr())


def stream_ptr():
    import torch

    return c_void_p(torch.cuda.current_stream().cuda_stream)
