// The chain plan (128 rows per workgroup) of the score model's predictor-corrector step (cond_pc_sampler, samplers.py:102-160) with the
// network's three dense layers as EXACT-PRODUCT split-bf16 on the BF16 matrix pipe (bf16x9.h; the trunk itself is trunk_bf16x9.h's, shared
// with the RK45 chain stage of rk45.hip): every fp32 operand is hi + mid + lo,
// all nine cross products are exact in fp32 and only the fp32 accumulation rounds - the error class of pc_step_chain_kernel<2, 0>
// (trunk_chain.h), which stays selectable (PCSampler(trunk="f32mfma")).  Same job, inputs and partials contract as that kernel:
// sampler update (PcRows, pc_rows.h: the sampler contract is there) -> pose encoder -> three 256-wide heads -> fp32 Linear(256, 3) outputs on the accumulators -> one partial sum of
// |score| per WAVE (gp_pc_layout's plan 128: four per workgroup) -> x / mean_x / trajectory; cross-rank coupling (gn_ext) and ragged
// last workgroups as there.
//
// Form: 4 waves per workgroup (one per SIMD, the whole 512-entry register file), each carrying TWO 16-row B tiles = 32 rows, 128 rows
// per workgroup, one workgroup per CU.  The D fragment of a layer is the next layer's B operand (two chunks per k-block of
// v_mfma_f32_16x16x32_bf16).  All weights stream through a 2-slot LDS ring in 33 slices of 48 KB: pose_encoder.0 (1) and pose_encoder.2
// (8) as (one 32-wide k-block) x (16 output chunks) x (hi, mid, lo), the fp32 activations split one k-block at a time; the three heads
// (8 each) as (two output chunks) x (eight k-blocks) x (hi, mid, lo) against pose_encoder.2's output split ONCE (trunk_bf16x9.h); slice
// s + 1 (held in registers since step s - 1) is written into the other slot while slot s is multiplied, slice s + 2 is requested, one
// barrier per slice.
// Budget per workgroup and launch (MI355X: LDS 256 B/clk/CU for conflict-free ds_read_b128, v_mfma_f32_16x16x32_bf16 16 cycles):
//   LDS fragment reads  33 slices x 48 KB x 4 waves = 6.3 MB  -> 24.8 k cycles (49.5 k at 128 B/clk)
//   MFMA                33 x 16 chunks x 9 products x 2 tiles = 9 504 per wave x 16 cycles = 152 k cycles per SIMD (63 us at the 2.4 GHz
//                       peak clock; dense BF16 MFMA loops on random data sustain 1.5-1.95 GHz on this part: 80 us at 1.9 GHz)
// so the matrix pipe bounds it, not LDS (bf16x3's 8 waves x 16 rows read the same 1.5 MB weight stream twice as often per row) and not
// the fp32 peak: 9 bf16 products per fp32 product at 16x the fp32 rate = 1.8x the fp32 MFMA FLOP rate.
// Measured (MI355X, 32 000 rows, HIP events around the PC-100 graph): 100.3 us per launch with chunk-major heads against 103.8 us with
// k-major heads (profiles/x9_heads_chunk_major.txt); 98.2 us against 102.3 us in one session (profiles/x9_kmajor_under_mfma.txt) with
//   - the staged fp32 operands (w_out, b0, b2, cvec[cloud] + tvec) requested BEFORE the weight ring's prologue and the sampler update
//     and stored to LDS after it (stage_request; 16-byte loads): -2.5 us, the larger part - they used to queue behind 24 weight loads and
//     were waited for at the first barrier;
//   - the k-major layers' splits and pose_encoder.0's bias + ReLU between their MFMAs: -1.0 us;
//   - pose_encoder.2's bias + ReLU + split tail in pieces beside its last step's MFMAs: -0.5 us on the PC kernels; the Heun kernel runs
//     without it (run<1>: with it 117 values parked in AGPRs against 76 and its pass is no faster than the parent's).
// Headline blocks 36.04-36.17 ms against 36.94-37.09 ms (-2.4 %); 98.7 against 102.9 us under rocprofv3; MFMA-busy cycles equal.
// What is left of the gap to the floor - 80 us at a sustained 1.9 GHz (the clock inside the kernel has not been measured) - is the
// prologue up to the first MFMA (~1 800 static instructions, both branch arms), barrier drains (one wave per SIMD), the half of the tail
// that does not fit two-per-MFMA, the head loop's short runs and the last head's last chunk.
//
// SIX PRODUCTS (pc_step_chain_kernel_bf16x6 and its seeded twin; gp_pc_step_bf16x6, PCSampler(products=6), what a score-model PC agent
// runs): the same text with NPROD = 6 - lo.lo, lo.mid and mid.lo are not issued (bf16x9.h: at most (2^-23 + 2^-32) |a b| per multiply,
// below the fp32 accumulation's own rounding); the weight packs are unchanged (the lo terms are still read for lo.hi and hi.lo).
//   MFMA                33 x 16 chunks x 6 products x 2 tiles = 6 336 per wave x 16 cycles = 101 k cycles per SIMD (42 us at 2.4 GHz, 53 us
//                       at 1.9 GHz); SQ_VALU_MFMA_BUSY_CYCLES 101 376 000 per launch against 152 064 000
// Measured with the nine-product side work and three other instructions behind each of a chunk's 12 MFMAs (profiles/x6_products.txt):
// 75.0-75.2 us per launch against 95.6-95.7 us in one alternating session (HIP events around the PC-100 graph, 32 000 rows); MFMA-busy
// over 4 x busy-CU cycles 0.57 against 0.65 - one wave per SIMD issues every instruction itself, an MFMA holds the vector issue for 8 of
// its 16 cycles and a VALU instruction for 4, and 6 336 MFMAs + 16 100 other instructions per wave are more issue than the matrix pipe's
// 101 k cycles.  So the six-product kernels issue FEWER instructions for the same side work (trunk_bf16x9.h, DIET;
// profiles/x6_issue_budget.txt): the ReLU behind a pinned sum as one v_max_i32 on the bits (the pin cost a v_max_f32 v, v, v each),
// the heads' Linear(256, 3) epilogue as one fma chain per output (4 instructions for 8, one rounding fewer per product), the second ring
// slot and the staged fp32 operands read through a pinned base register + an immediate (no add per address, no addresses parked in
// AGPRs), and two other instructions behind each MFMA again, as nine products have it.  Per wave and launch 16 125 -> 13 703 instructions
// that are not MFMAs (VALU 8 562 -> 6 405; SQ_INSTS_VALU 15.36 M -> 13.10 M per launch, MFMA-busy 101 376 000 unchanged), 256 + 231
// registers, 18 values parked in AGPRs, 0 B of scratch, both kernels.  70.8-71.0 us per launch against 75.6-75.8 us in one alternating
// session (-6.4 %; 2.3 us the instructions, 1.8 us the two-per-MFMA placement), MFMA-busy over 4 x busy-CU 0.63; headline blocks
// 25.67-25.84 ms against 26.68-26.90 ms (-3.8 %).  Left: the pins' own s_nop pads, the 64-bit adds of the ring's global loads, 173 packed
// fp32 instructions of the splits (unpacking them raised the count and gained nothing), and the exposed parts listed above.  The clock
// inside the kernel has not been measured.  The Heun, DPM-Solver and RK45 kernels and the nine-product PC kernels keep nine products and
// their device code, instruction for instruction: their bits are recorded.
#include "pc_rows.h"
#include "trunk_bf16x9.h"
#include "trunk_chain.h"

namespace {

using namespace gp_trunk;
using namespace gp_x9trunk;

// SEEDED (pc_step_chain_seeded_kernel_bf16x9): PcRows draws the noise (pc_rows.h); the rest is the same text.
// HEUN (heun_step_chain_kernel_bf16x9; Args = HeunArgs): a launch of the fixed-step Heun solver of the probability-flow ODE
// (cond_edm_sampler's method, samplers.py:230-290) - PcRows runs the row-local update, the score is stored, there is no partial sum.
// SOLVER_DPM2M (dpm2m_step_chain_kernel_bf16x9): a launch of the DPM-Solver++(2M) solver (pc_rows.h), the same through PcRows' other update.
// NPROD = 6 (pc_step_chain_kernel_bf16x6, the PC step only): lo.lo, lo.mid and mid.lo are not issued (bf16x9.h) - the same text, weight
// packs and ring, 6 336 MFMAs per wave instead of 9 504.
template <bool SEEDED, int SOLVER = SOLVER_PC, class Args = PcArgs, int NPROD = 9>
__device__ __forceinline__ void pc_step_chain_bf16x9(const Args &a, const SplitNet &w) {
    constexpr bool HEUN = SOLVER != SOLVER_PC;
    static_assert(HEUN == std::is_same<Args, HeunArgs>::value && !(HEUN && SEEDED), "HeunArgs drive the HEUN instantiation");
    static_assert(NPROD == 9 || !HEUN, "the fixed-step solvers pin fp32 bits: nine products");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), i = a.step;
    const int wg_row0 = blockIdx.x * X9_ROWS;
    // ---- the rows' operands first, the ring prologue behind them (memory returns in order)
    PcRows<X9_RT, SEEDED, SOLVER> rs;
    rs.template request<X9_NW>(a, wave, lane);
    const float *tvec = a.tvec_all + (size_t)pc_time_row<SOLVER>(i) * HEADS;
    X9Staged sg;
    bf16x8 first[X9_PER_T], hold[X9_PER_T];
    if (i < a.nsteps) {
        stage_request(sg, w, a.cvec, tvec, wg_row0, a.nrows, a.kcand);  // nothing of it depends on the update: it arrives under it
        request(w, tid, first, hold);
    }
    if (rs.finish_previous(a, lane)) return;
    // each head's three score components are final once its epilogue is done: stored there, their squares summed in component order
    const float sden = rs.sigma + 1e-7f;
    float q[X9_RT] = {};
    run<HEUN ? 1 : 2, NPROD>(lds, w, a.cvec, tvec, wg_row0, a.nrows, a.kcand, first, hold, rs.xv, rs.row,
        [&](int h, int p, const float (&out)[3]) __attribute__((always_inline)) {
            const float sc[3] = {out[0] / sden, out[1] / sden, out[2] / sden};
            pc_store_score(a, rs.row[p], lane, 3 * h, sc, q[p]);
        }, sg);
    if constexpr (!HEUN) pc_store_partial<X9_RT, X9_NW>(a, rs.row, q, wave, lane);
}

__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_kernel_bf16x9(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<false>(a, w); }
__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_seeded_kernel_bf16x9(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<true>(a, w); }
__global__ __launch_bounds__(X9_NT, 1) void heun_step_chain_kernel_bf16x9(HeunArgs a, SplitNet w) { pc_step_chain_bf16x9<false, SOLVER_HEUN>(a, w); }
__global__ __launch_bounds__(X9_NT, 1) void dpm2m_step_chain_kernel_bf16x9(HeunArgs a, SplitNet w) { pc_step_chain_bf16x9<false, SOLVER_DPM2M>(a, w); }
// the PC step with six of the nine products (after the nine-product kernels: their device code keeps its place in the file)
__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_kernel_bf16x6(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<false, SOLVER_PC, PcArgs, 6>(a, w); }
__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_seeded_kernel_bf16x6(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<true, SOLVER_PC, PcArgs, 6>(a, w); }

// stage_request reads the staged fp32 operands with 16-byte loads
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool staged_aligned(const gp_scorenet *net, const float *cvec, const float *tvec_all) {
    return aligned16(net->b_pose0) && aligned16(net->b_pose2) && aligned16(net->w_out) && aligned16(cvec) && aligned16(tvec_all);
}

// What the two PC entry points share: the chain plan's rules, PcArgs / SplitNet and the launch.
// z_lang carries the Langevin noise or, for the seeded kernel, the seed state (PcArgs).
template <auto Kern>
int launch_pc_bf16x9(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                     const float *sched, const float *z_lang, const float *z_pred, const float *centre, float *x, float *mean_x, float *score, float *partials,
                     float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || step < 0 || step > nsteps || !net || !cvec || !tvec_all || !sched || !z_lang || !centre || !x ||
        !mean_x || !score || !partials || gn_rows_total < 0 || !w_pose0_x9 || !w_pose2_x9 || !w_headx_x9 || !staged_aligned(net, cvec, tvec_all))
        return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    if (ngroups * rg == 0) return GP_OK;
    int P = 0, nparts = 0;
    const int rc = gp_pc_layout(0, X9_ROWS, ngroups, nclouds_per_group, k, &P, &nparts);  // the chain plan's rules and partials size
    if (rc != GP_OK) return rc;
    if (P != X9_ROWS || !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    const PcArgs a = pc_args(ngroups, rg, k, step, nsteps, nparts, (rg + X9_ROWS - 1) / X9_ROWS, cvec, tvec_all, sched, z_lang, z_pred, centre, x, mean_x, score,
                             partials, traj, gn_ext, gn_rows_total);
    return gp_launch<Kern>(dim3(a.wgpg * ngroups), dim3(X9_NT), X9Lds::BYTES, (hipStream_t)s, a, split_net(net, w_pose0_x9, w_pose2_x9, w_headx_x9));
}

// A launch of a fixed-step solver (gp_heun_step_bf16x9, gp_dpm2m_step_bf16x9).
template <int SOLVER>
int fixed_step_bf16x9(int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                      const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                      const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || nsteps < 1 || launch < 0 || launch >= fixed_launches<SOLVER>(nsteps, denoise) || !net || !cvec ||
        !tvec_all || !sched || !centre || !x || !d || !score || !out || !w_pose0_x9 || !w_pose2_x9 || !w_headx_x9 || !staged_aligned(net, cvec, tvec_all))
        return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    if (ngroups * rg == 0) return GP_OK;
    int P = 0;
    const int rc = gp_heun_layout(X9_ROWS, ngroups, nclouds_per_group, k, &P);  // the chain plan's rules
    if (rc != GP_OK) return rc;
    const HeunArgs a = heun_args(ngroups * rg, k, launch, fixed_launches<SOLVER>(nsteps, denoise) - 1, cvec, tvec_all, sched, centre, x, d, score, out, traj);
    constexpr auto kern = SOLVER == SOLVER_DPM2M ? dpm2m_step_chain_kernel_bf16x9 : heun_step_chain_kernel_bf16x9;
    return gp_launch<kern>(dim3(ngroups * ((rg + X9_ROWS - 1) / X9_ROWS)), dim3(X9_NT), X9Lds::BYTES, (hipStream_t)s, a,
                           split_net(net, w_pose0_x9, w_pose2_x9, w_headx_x9));
}

}  // namespace

extern "C" {

int gp_pc_step_bf16x9(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                      const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score,
                      float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                      const void *w_headx_x9, gp_stream_t s) {
    if (!z_predictor) return GP_EINVAL;
    return launch_pc_bf16x9<pc_step_chain_kernel_bf16x9>(ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x,
                                                         mean_x, score, partials, traj, gn_ext, gn_rows_total, w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

int gp_pc_step_bf16x9_seeded(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                             const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                             float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                             const void *w_headx_x9, gp_stream_t s) {
    if ((uint32_t)nsteps >= gp_philox::MAX_STEPS) return GP_EINVAL;
    return launch_pc_bf16x9<pc_step_chain_seeded_kernel_bf16x9>(ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched,
                                                                reinterpret_cast<const float *>(seed_state), nullptr, centre, x, mean_x, score, partials, traj,
                                                                gn_ext, gn_rows_total, w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

int gp_pc_step_bf16x6(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                      const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score,
                      float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                      const void *w_headx_x9, gp_stream_t s) {
    if (!z_predictor) return GP_EINVAL;
    return launch_pc_bf16x9<pc_step_chain_kernel_bf16x6>(ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x,
                                                         mean_x, score, partials, traj, gn_ext, gn_rows_total, w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

int gp_pc_step_bf16x6_seeded(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                             const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                             float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                             const void *w_headx_x9, gp_stream_t s) {
    if ((uint32_t)nsteps >= gp_philox::MAX_STEPS) return GP_EINVAL;
    return launch_pc_bf16x9<pc_step_chain_seeded_kernel_bf16x6>(ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched,
                                                                reinterpret_cast<const float *>(seed_state), nullptr, centre, x, mean_x, score, partials, traj,
                                                                gn_ext, gn_rows_total, w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

int gp_heun_step_bf16x9(int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                        const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                        const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s) {
    return fixed_step_bf16x9<SOLVER_HEUN>(ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                          w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

int gp_dpm2m_step_bf16x9(int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                         const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                         const void *w_pose0_x9, const void *w_pose2_x9, const void *w_headx_x9, gp_stream_t s) {
    return fixed_step_bf16x9<SOLVER_DPM2M>(ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                           w_pose0_x9, w_pose2_x9, w_headx_x9, s);
}

}  // extern "C"
