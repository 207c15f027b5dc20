// The chain plan (128 rows per workgroup) of the score model's predictor-corrector step (cond_pc_sampler, samplers.py:102-160) with the
// network's three dense layers as EXACT-PRODUCT split-bf16 on the BF16 matrix pipe (bf16x9.h): every fp32 operand is hi + mid + lo,
// all nine cross products are exact in fp32 and only the fp32 accumulation rounds - the error class of pc_step_chain_kernel<2, 0>
// (trunk_chain.h), which stays selectable (PCSampler(trunk="f32mfma")).  Same job, inputs and partials contract as that kernel:
// sampler update (PcRows, pc_rows.h: the sampler contract is there) -> pose encoder -> three 256-wide heads -> fp32 Linear(256, 3) outputs on the accumulators -> one partial sum of
// |score| per WAVE (gp_pc_layout's plan 128: four per workgroup) -> x / mean_x / trajectory; cross-rank coupling (gn_ext) and ragged
// last workgroups as there.
//
// Form: 4 waves per workgroup (one per SIMD, the whole 512-entry register file), each carrying TWO 16-row B tiles = 32 rows, 128 rows
// per workgroup, one workgroup per CU.  The D fragment of a layer is the next layer's B operand (two chunks per k-block of
// v_mfma_f32_16x16x32_bf16); activations stay in fp32 registers and are split into hi / mid / lo one k-block at a time.  All weights
// stream through a 2-slot LDS ring in 33 slices of 48 KB = (one 32-wide k-block) x (16 output chunks) x (hi, mid, lo): pose_encoder.0
// (1), pose_encoder.2 (8), three heads (8 each); slice s + 1 (held in registers since step s - 1) is written into the other slot while
// slot s is multiplied, slice s + 2 is requested, one barrier per slice.
// Budget per workgroup and launch (MI355X: LDS 256 B/clk/CU for conflict-free ds_read_b128, v_mfma_f32_16x16x32_bf16 16 cycles):
//   LDS fragment reads  33 slices x 48 KB x 4 waves = 6.3 MB  -> 24.8 k cycles (49.5 k at 128 B/clk)
//   MFMA                33 x 16 chunks x 9 products x 2 tiles = 9 504 per wave x 16 cycles = 152 k cycles per SIMD (63 us at the 2.4 GHz
//                       peak clock; dense BF16 MFMA loops on random data sustain 1.5-1.95 GHz on this part: 80 us at 1.9 GHz)
// so the matrix pipe bounds it, not LDS (bf16x3's 8 waves x 16 rows read the same 1.5 MB weight stream twice as often per row) and not
// the fp32 peak: 9 bf16 products per fp32 product at 16x the fp32 rate = 1.8x the fp32 MFMA FLOP rate.
// Measured (MI355X, 32 000 rows, rocprofv3): 118.0 us per launch against 142.7 us for pc_step_chain_kernel<2, 0> (102.7 us by HIP events
// since); the rest of the gap to the floor - 80 us at a sustained 1.9 GHz, not the 63 us of the peak clock, so the kernel runs near 0.8 of
// what the clock allows - is barrier drains (one wave per SIMD), the head epilogues (not overlapped with MFMAs) and a few spilled registers.
#include "bf16x9.h"
#include "pc_rows.h"
#include "trunk_chain.h"

namespace {

using namespace gp_trunk;
using namespace gp_bf16x9;
using namespace gp_split;

constexpr int X9_NW = 4, X9_NT = 64 * X9_NW, X9_RT = 2, X9_ROWS = 16 * X9_RT * X9_NW;
using X9Lds = SplitLds<3, 2>;  // 2 slots of 48 KB
constexpr int X9_SLICE = X9Lds::SLICE, X9_PER_T = X9_SLICE / X9_NT;
static_assert(X9_ROWS == 128 && X9_PER_T <= 16, "one slice element per thread and output chunk at most");

// End of a ring step: this wave's LDS writes of the step have completed (lgkmcnt), then the bare barrier.  No vmcnt wait: the
// slice in flight to the registers may stay in flight across it.  The empty asm statements keep LDS accesses on their side.
__device__ __forceinline__ void x9_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// SEEDED (pc_step_chain_seeded_kernel_bf16x9): PcRows draws the noise (pc_rows.h); the rest is the same text.
template <bool SEEDED>
__device__ __forceinline__ void pc_step_chain_bf16x9(const PcArgs &a, const SplitNet &w) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);
    const float *woutl = lds + X9Lds::OFF_WOUT, *b0l = lds + X9Lds::OFF_B0, *b2l = lds + X9Lds::OFF_B2, *cvtl = lds + X9Lds::OFF_CVT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 4, i = a.step;
    const int wg_row0 = blockIdx.x * X9_ROWS;
    // ---- the rows' operands first, the ring prologue behind them (memory returns in order)
    PcRows<X9_RT, SEEDED> rs;
    rs.template request<X9_NW>(a, wave, lane);
    // slice 0 (-> slot 0 below) and slice 1 (-> registers, written during step 0)
    bf16x8 first[X9_PER_T], hold[X9_PER_T];
    if (i < a.nsteps) {
#pragma unroll
        for (int u = 0; u < X9_PER_T; ++u) first[u] = split_slice<3>(w, 0)[tid + u * X9_NT];
#pragma unroll
        for (int u = 0; u < X9_PER_T; ++u) hold[u] = split_slice<3>(w, 1)[tid + u * X9_NT];
    }
    if (rs.finish_previous(a, lane)) return;
    // ---- staged epilogue operands and slot 0
    split_stage<X9_NT, X9Lds>(lds, w, a.cvec, a.tvec_all + (size_t)i * HEADS, wg_row0, a.nrows, a.kcand);
#pragma unroll
    for (int u = 0; u < X9_PER_T; ++u) ring[tid + u * X9_NT] = first[u];
    __syncthreads();
    int gstep = 0;
    f32x4 acc[X9_RT][16];
    // one ring step over slot gstep % 2: for output chunk n, the three weight terms (read one chunk ahead) x the two row tiles' split
    // k-block = 18 MFMAs; beside chunk n < PER_T, element n of slice gstep + 1 goes from the registers to the other slot (last read
    // in step gstep - 1) and element n of slice gstep + 2 is requested; one barrier
    auto ring_step = [&](const Split8 (&xs)[X9_RT]) {
        const bf16x8 *slot = ring + (gstep & 1) * X9_SLICE;
        bf16x8 *dst = ring + ((gstep + 1) & 1) * X9_SLICE;
        const bf16x8 *src = split_slice<3>(w, gstep + 2);
        bf16x8 wf[2][3];
#pragma unroll
        for (int t = 0; t < 3; ++t) wf[0][t] = slot[t * 64 + lane];
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            if (n + 1 < 16) {
#pragma unroll
                for (int t = 0; t < 3; ++t) wf[(n + 1) & 1][t] = slot[((n + 1) * 3 + t) * 64 + lane];
            }
            if (n < X9_PER_T) {
                dst[tid + n * X9_NT] = hold[n];
                hold[n] = src[tid + n * X9_NT];
            }
            f32x4 an[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) an[p] = acc[p][n];
            mma9<X9_RT>(wf[n & 1], xs, an);
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) acc[p][n] = an[p];
            __builtin_amdgcn_sched_barrier(0);  // one chunk per region: the optimiser would hoist every fragment read of the step
        }
        ++gstep;
        x9_barrier();
    };
    auto zero_acc = [&]() {
#pragma unroll
        for (int p = 0; p < X9_RT; ++p)
#pragma unroll
            for (int n = 0; n < 16; ++n) acc[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // bias + ReLU of a 256-wide hidden layer, kept in fp32 (split one k-block at a time as the next layer consumes it)
    f32x4 act[X9_RT][16];
    auto hidden = [&](const float *bias) {
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 16 * n + 4 * g);
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) act[p][n] = relu4(acc[p][n] + bv);
        }
    };
    auto layer = [&]() {  // acc = W . act over the 8 k-blocks of a 256-wide input
        zero_acc();
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            Split8 xs[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) xs[p] = split8(act[p][2 * kb], act[p][2 * kb + 1]);
            ring_step(xs);
        }
    };
    // ---- pose_encoder.0
    {
        Split8 xs[X9_RT];
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            f32x4 pa, pb;
            split_pose_fragment(rs.xv[p], g, pa, pb);
            xs[p] = split8(pa, pb);
        }
        zero_acc();
        ring_step(xs);
    }
    hidden(b0l);
    // ---- pose_encoder.2
    layer();
    hidden(b2l);
    // ---- the three heads; their Linear(256, 3) output layers as fp32 dot products on the accumulator fragments
    int cl[X9_RT];
#pragma unroll
    for (int p = 0; p < X9_RT; ++p) {
        const int r = rs.row[p] < a.nrows ? rs.row[p] : a.nrows - 1;
        cl[p] = r / a.kcand - wg_row0 / a.kcand;  // < NCL (gp_pc_layout admits k only when a workgroup's rows span <= NCL clouds)
    }
    // each head's three score components are final once its epilogue is done: stored there, their squares summed in component order
    const float sden = rs.sigma + 1e-7f;
    float q[X9_RT] = {};
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        layer();
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            // (bf16_split_common.h's split_head_out written out: through the helper this kernel, which sits on the register cliff,
            // compiles to 168 spilled registers instead of 27)
            float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
            for (int n = 0; n < 16; ++n) {
                const int ch = 16 * n + 4 * g;
                const f32x4 v = relu4(acc[p][n] + *reinterpret_cast<const f32x4 *>(cvtl + cl[p] * HEADS + 256 * h + ch));
                const f32x4 w0 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 0) * HID + ch);
                const f32x4 w1 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 1) * HID + ch);
                const f32x4 w2 = *reinterpret_cast<const f32x4 *>(woutl + (3 * h + 2) * HID + ch);
                o0 += v.x * w0.x + v.y * w0.y + v.z * w0.z + v.w * w0.w;
                o1 += v.x * w1.x + v.y * w1.y + v.z * w1.z + v.w * w1.w;
                o2 += v.x * w2.x + v.y * w2.y + v.z * w2.z + v.w * w2.w;
            }
            // the four lane groups hold the four channel quarters: fixed order, every lane gets the sum
            const float sc[3] = {(lane_groups_sum(o0) + w.b_out[3 * h + 0]) / sden, (lane_groups_sum(o1) + w.b_out[3 * h + 1]) / sden,
                                 (lane_groups_sum(o2) + w.b_out[3 * h + 2]) / sden};
            pc_store_score(a, rs.row[p], lane, 3 * h, sc, q[p]);
        }
    }
    pc_store_partial<X9_RT, X9_NW>(a, rs.row, q, wave, lane);
}

__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_kernel_bf16x9(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<false>(a, w); }
__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_seeded_kernel_bf16x9(PcArgs a, SplitNet w) { pc_step_chain_bf16x9<true>(a, w); }

}  // namespace

extern "C" {

int gp_pc_step_bf16x9(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                      const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score,
                      float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                      const void *w_headx_x9, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || step < 0 || step > nsteps || !net || !cvec || !tvec_all || !sched || !z_langevin ||
        !z_predictor || !centre || !x || !mean_x || !score || !partials || gn_rows_total < 0 || !w_pose0_x9 || !w_pose2_x9 || !w_headx_x9)
        return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    if (ngroups * rg == 0) return GP_OK;
    int P = 0, nparts = 0;
    const int rc = gp_pc_layout(0, X9_ROWS, ngroups, nclouds_per_group, k, &P, &nparts);  // the chain plan's rules and partials size
    if (rc != GP_OK) return rc;
    if (P != X9_ROWS || !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    const PcArgs a = pc_args(ngroups, rg, k, step, nsteps, nparts, (rg + X9_ROWS - 1) / X9_ROWS, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x,
                             mean_x, score, partials, traj, gn_ext, gn_rows_total);
    const SplitNet w = {reinterpret_cast<const bf16x8 *>(w_pose0_x9), reinterpret_cast<const bf16x8 *>(w_pose2_x9),
                        reinterpret_cast<const bf16x8 *>(w_headx_x9), net->b_pose0, net->b_pose2, net->w_out, net->b_out};
    static bool done = false;
    if (!done) {
        if (set_lds(pc_step_chain_kernel_bf16x9, X9Lds::BYTES)) return GP_ELAUNCH;
        done = true;
    }
    hipLaunchKernelGGL(pc_step_chain_kernel_bf16x9, dim3(a.wgpg * ngroups), dim3(X9_NT), X9Lds::BYTES, (hipStream_t)s, a, w);
    return gp_launch_status();
}

int gp_pc_step_bf16x9_seeded(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                             const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                             float *partials, float *traj, const float *gn_ext, int gn_rows_total, const void *w_pose0_x9, const void *w_pose2_x9,
                             const void *w_headx_x9, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || step < 0 || step > nsteps || (uint32_t)nsteps >= gp_philox::MAX_STEPS || !net || !cvec ||
        !tvec_all || !sched || !seed_state || !centre || !x || !mean_x || !score || !partials || gn_rows_total < 0 || !w_pose0_x9 || !w_pose2_x9 ||
        !w_headx_x9)
        return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    if (ngroups * rg == 0) return GP_OK;
    int P = 0, nparts = 0;
    const int rc = gp_pc_layout(0, X9_ROWS, ngroups, nclouds_per_group, k, &P, &nparts);
    if (rc != GP_OK) return rc;
    if (P != X9_ROWS || !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    // (the seed state travels in the argument block's z_lang slot: PcArgs)
    const PcArgs a = pc_args(ngroups, rg, k, step, nsteps, nparts, (rg + X9_ROWS - 1) / X9_ROWS, cvec, tvec_all, sched,
                             reinterpret_cast<const float *>(seed_state), nullptr, centre, x, mean_x, score, partials, traj, gn_ext, gn_rows_total);
    const SplitNet w = {reinterpret_cast<const bf16x8 *>(w_pose0_x9), reinterpret_cast<const bf16x8 *>(w_pose2_x9),
                        reinterpret_cast<const bf16x8 *>(w_headx_x9), net->b_pose0, net->b_pose2, net->w_out, net->b_out};
    static bool done = false;
    if (!done) {
        if (set_lds(pc_step_chain_seeded_kernel_bf16x9, X9Lds::BYTES)) return GP_ELAUNCH;
        done = true;
    }
    hipLaunchKernelGGL(pc_step_chain_seeded_kernel_bf16x9, dim3(a.wgpg * ngroups), dim3(X9_NT), X9Lds::BYTES, (hipStream_t)s, a, w);
    return gp_launch_status();
}

}  // extern "C"
