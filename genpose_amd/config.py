"""The subset of the reference's flat argparse namespace (configs/config.py:4-112) the inference hot path reads,
with the reference's defaults.  `get_config(**overrides)` returns an argparse.Namespace, so code written against the
reference's `cfg` object works unchanged; the reference's own namespace can be passed to PoseNet(cfg) directly."""
import argparse

# How the reference's `dx*dx + dy*dy + dz*dz` (sampling_gpu.cu:133, ball_query_gpu.cu:33, interpolate_gpu.cu:36; also the weighted sum
# of interpolate_gpu.cu:95) is contracted into fused multiply-adds - nvcc's choice, which decides FPS / ball-query indices when two
# distances agree to an ulp (include/genpose_hip.h GP_ARITH_*).  Flipping the default is this one line (+ the
# GP_ARITH_DEFAULT of the header for the C entry points without an `_arith` suffix; tests/test_abi_and_host.py holds the two and the
# oracle's default together).
DIST_ARITH_CODES = {"A": 0, "B": 1, "C": 2}
DEFAULT_DIST_ARITH = "B"


def dist_arith_code(arith=None):
    a = DEFAULT_DIST_ARITH if arith is None else arith
    if a not in DIST_ARITH_CODES:
        raise ValueError(f"dist_arith must be one of {sorted(DIST_ARITH_CODES)}, got {a!r}")
    return DIST_ARITH_CODES[a]


DEFAULTS = dict(
    device="cuda", num_points=1024, pose_mode="rot_matrix", pts_encoder="pointnet2", pointnet2_params="light",
    posenet_mode="score", regression_head="Rx_Ry_and_T", sde_mode="ve", sampler_mode=["ode"], sampling_steps=None,
    energy_mode="IP", s_theta_mode="score", norm_energy="identical", eval_repeat_num=50, batch_size=192, T0=1.0,
    pooling_mode="nearest", ranker="energy_ranker", score_model_dir="", energy_model_dir="", result_dir="", test_source="Real",
    save_video=False, is_train=False, use_pretrain=False, log_dir="debug", parallel=False, seed=0,
    # pre-processing / evaluation side (preprocess.py, evaluation.py): configs/config.py:8,72-78
    sampler_precision="f32",  # (ours) 'bf16x3': opt-in, exploratory split-bf16 products in the PC sampler's score network (csrc/trunk_bf16x3.hip)
    sampler_seed=None,  # (ours) an integer: opt-in seeded noise drawn inside the PC step kernels (csrc/philox.h), reproducible per row; None: torch's generator
    likelihood_divergence="hutchinson",  # (ours) 'exact': net(data, mode='likelihood') integrates the exact trace of the score Jacobian instead of the reference's one-probe Skilling-Hutchinson estimate (csrc/score_bwd.h: score_div_exact_tile) - deterministic, no prior draw
    likelihood_solver="rk45",  # (ours) 'heun': likelihoods (mode 'likelihood', calc_likelihood, PoseNet.get_likelihood) from the fixed-step Heun solve of the exact-divergence ODE (samplers.HeunLikelihood) instead of the adaptive RK45 driver; needs likelihood_divergence / divergence 'exact' and likelihood_steps
    likelihood_steps=None,  # (ours) N of likelihood_solver 'heun' (NFE = 2 N)
    likelihood_grid="geometric",  # (ours) sigma grid of likelihood_solver 'heun': 'geometric' or 'edm' (heun_grid's two)
    heun_grid="geometric",  # (ours) sampler_mode ['heun'] (the fixed-step Heun solver of the probability-flow ODE, samplers.HeunSampler; sampling_steps = its N) and ['dpm2m'] (the DPM-Solver++(2M) solver on the same grid, samplers.Dpm2mSampler: one evaluation per step): the sigma grid - 'geometric' (t uniform) or 'edm' (cond_edm_sampler's rho = 7 discretisation)
    fixed_step_energy=False,  # (ours) True: opt-in - sampler_mode ['heun'] / ['dpm2m'] serve a posenet_mode='energy' agent too: the fixed-step solvers driven by the energy model's score, the gradient of its inner-product energy evaluated inside the kernels (samplers.HeunSampler / Dpm2mSampler(model='energy')); False: such an agent refuses both samplers, as before
    sampler_products="auto",  # (ours) products per multiply of the PC sampler's split-bf16 chain kernel (PCSampler(products=), csrc/bf16x9.h), read where that kernel applies (score model, 128-row chain plan): 6 = lo.lo, lo.mid and mid.lo are not issued (at most (2^-23 + 2^-32) |a b| per multiply, below the fp32 accumulation's own rounding: still the fp32 kernels' error class, 6 / 9 of the matrix-pipe work), 9 = all nine, bit for bit as before, 'auto' = 6 for a score-model agent of the PC sampler
    ode_trunk=None,  # (ours) 'bf16x9': opt-in exact-product split-bf16 trunk in the ODE sampler's chain-plan stage kernels (ODESampler(trunk=)); None / 'f32mfma': the fp32 MFMA kernels
    encoder_precision="f32",  # (ours) 'bf16x3': opt-in, exploratory split-bf16 products on the 128-196-256 grouping level (csrc/sa_bf16x3.hip)
    encoder_level2="auto",  # (ours) under encoder_precision 'f32', the arithmetic of grouping level 2 (128-196-256): 'bf16x9' = exact-product split bf16 on the BF16 matrix pipe (csrc/sa_bf16x9.hip, the fp32 kernels' error class; the kernel forms six of the nine products of the split, each exact - lo.lo, lo.mid and mid.lo, together at most (2^-23 + 2^-32) |a b| per multiply, are not issued (csrc/bf16x9.h)), 'f32mfma' = the fp32 MFMA kernels, bit for bit as before, 'auto' = 'bf16x9' for an agent of the fixed-step PC sampler, 'f32mfma' for the adaptive ODE sampler (its goldens pin RK45 attempt counts that move with the last bits of the features); encoder_precision='bf16x9' forces it
    encoder_level1="auto",  # (ours) the arithmetic of grouping level 1 (64-64/96-128): 'bf16x9' = layers 2-3 as exact-product split bf16 with LDS-resident weights (csrc/sa_lds_bf16x9.hip, the fp32 kernels' error class; the kernel forms six of the nine products of the split, each exact - lo.lo, lo.mid and mid.lo, together at most (2^-23 + 2^-32) |a b| per multiply, are not issued (csrc/bf16x9.h); batches below Pointnet2EncoderHIP.LEVEL1_BF16X9_MIN_CLOUDS keep the fp32 kernels), 'f32mfma' = the fp32 MFMA kernels, bit for bit as before, 'auto' = 'bf16x9' for an agent of the fixed-step PC sampler, 'f32mfma' for the ODE, Heun and DPM samplers (their goldens pin fp32 bits)
    encoder_level3="auto",  # (ours) the arithmetic of the GroupAll level (128 points x 512 -> 256 -> 256 | 384 -> 512): 'bf16x9' = all three layers of both scales as exact-product split bf16 in one launch (csrc/sa_groupall_bf16x9.hip, the fp32 kernels' error class; the kernel forms six of the nine products of the split, each exact - lo.lo, lo.mid and mid.lo, together at most (2^-23 + 2^-32) |a b| per multiply, are not issued (csrc/bf16x9.h); batches below Pointnet2EncoderHIP.LEVEL3_BF16X9_MIN_CLOUDS keep the fp32 kernels), 'f32mfma' = the fp32 MFMA kernels, bit for bit as before, 'auto' = 'bf16x9' for an agent of the fixed-step PC sampler, 'f32mfma' for the ODE, Heun and DPM samplers (their goldens pin fp32 bits)
    dist_arith=DEFAULT_DIST_ARITH,  # (ours) contraction convention of the grouping operators' distances, see above
    synset_names=["bottle", "bowl", "camera", "can", "laptop", "mug"], img_size=256, max_eval_num=10000000, results_path="",
)


def _pipe_of(cfg, field):
    """An `auto | bf16x9 | f32mfma` field (the reference's own namespace has none of them: 'auto'); 'auto' resolves by sampler mode: 'bf16x9'
    for an agent of the fixed-step PC sampler, 'f32mfma' for every other."""
    v = getattr(cfg, field, "auto")
    if v not in ("auto", "bf16x9", "f32mfma"):
        raise ValueError(f"{field} {v!r}: 'auto', 'bf16x9' or 'f32mfma'")
    if v == "auto":
        mode = getattr(cfg, "sampler_mode", None) or ["ode"]
        v = "bf16x9" if mode[0] == "pc" else "f32mfma"
    return v


def sampler_products_of(cfg):
    """The `products` of PCSampler a namespace asks for: sampler_products 9 | 6, 'auto' = 6 for a score-model agent of the PC sampler and 9
    for every other (where the sampler ignores it)."""
    v = getattr(cfg, "sampler_products", "auto")
    if v not in ("auto", 9, 6):
        raise ValueError(f"sampler_products {v!r}: 'auto', 9 or 6")
    if v == "auto":
        mode = getattr(cfg, "sampler_mode", None) or ["ode"]
        v = 6 if mode[0] == "pc" and getattr(cfg, "posenet_mode", "score") == "score" else 9
    return v


def encoder_precision_of(cfg):
    """The `precision` of Pointnet2EncoderHIP a namespace asks for.  encoder_precision 'f32' names the accuracy class; within it
    encoder_level2 picks the matrix pipe of grouping level 2."""
    prec = getattr(cfg, "encoder_precision", "f32")
    return "bf16x9" if _pipe_of(cfg, "encoder_level2") == "bf16x9" and prec == "f32" else prec


def encoder_level1_of(cfg):
    """The `level1` of Pointnet2EncoderHIP a namespace asks for."""
    return _pipe_of(cfg, "encoder_level1")


def encoder_level3_of(cfg):
    """The `level3` of Pointnet2EncoderHIP a namespace asks for."""
    return _pipe_of(cfg, "encoder_level3")


def encoder_kwargs_of(cfg):
    """The keyword arguments of Pointnet2EncoderHIP a namespace asks for."""
    return dict(arith=getattr(cfg, "dist_arith", None), precision=encoder_precision_of(cfg), level1=encoder_level1_of(cfg), level3=encoder_level3_of(cfg))


def get_config(**overrides):
    d = dict(DEFAULTS)
    unknown = set(overrides) - set(d)
    if unknown:
        raise ValueError(f"unknown config fields: {sorted(unknown)}")
    d.update(overrides)
    return argparse.Namespace(**d)
