// OPT-IN, EXPLORATORY (round 5): one launch of the predictor-corrector sampler (cond_pc_sampler, samplers.py:102-160) with the score network's
// dense layers on the BF16 matrix pipe as three-term split products, fp32 accumulation (bf16x3.h) - the arithmetic of sa_bf16x3.hip applied to
// pc_step_chain_kernel's job.  NOT the default and in no parity claim: the headline numbers are the fp32 kernels' (scorenet.hip, trunk_chain.h).
// PC sampler only: the adaptive RK45 driver keeps the fp32 trunk (its error estimate compares differences of right-hand sides).
//
// Form: 8 waves per workgroup, 16 rows per wave = 128 rows per workgroup (the fp32 chain form's row block, so the same batches-per-launch
// rules apply), one workgroup per CU.  A wave carries its rows from the sampler update to the score in registers (the D fragment of a layer
// IS the next layer's operand, two chunks per k-block of v_mfma_f32_16x16x32_bf16); ALL weights stream through a 3-slot LDS ring in 33 slices
// of 32 KB = (one 32-wide k-block) x (16 output chunks) x (hi, lo): pose_encoder.0 (1), pose_encoder.2 (8), three heads (8 each); one barrier
// per slice.  The three Linear(256, 3) output layers are fp32 dot products on the VALU, taken on the accumulator fragments.
// The sampler update, the stores and the partials contract are pc_step_chain_kernel's (PcRows, pc_rows.h); what it shares with the
// bf16x9 trunk is in bf16_split_common.h.
// Bound: the LDS fragment reads (every wave reads every slice: 8 MB per workgroup) and the barriers, not the matrix pipe.
#include "bf16x3.h"
#include "pc_rows.h"

namespace {

using namespace gp_trunk;
using namespace gp_bf16x3;
using namespace gp_split;

constexpr int BF_NW = 8, BF_NT = 64 * BF_NW, BF_ROWS = 16 * BF_NW;
using BfLds = SplitLds<2, 3>;  // 3 slots of 32 KB
constexpr int BF_SLICE = BfLds::SLICE, BF_PER_T = BF_SLICE / BF_NT;
static_assert(BF_ROWS == 128, "the chain plan's row block");

__global__ __launch_bounds__(BF_NT) void pc_step_bf16x3_kernel(PcArgs a, SplitNet w) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);
    const float *woutl = lds + BfLds::OFF_WOUT, *b0l = lds + BfLds::OFF_B0, *b2l = lds + BfLds::OFF_B2, *cvtl = lds + BfLds::OFF_CVT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, i = a.step;
    const int wg_row0 = blockIdx.x * BF_ROWS;
    // ---- the row's operands first, the ring prologue and the staged epilogue operands behind them
    PcRows<1> rs;
    rs.request<BF_NW>(a, wave, lane);
    if (i < a.nsteps) {
        // ring prologue: slices 0 and 1 into slots 0 and 1
#pragma unroll
        for (int u = 0; u < BF_PER_T; ++u) {
            ring[0 * BF_SLICE + tid + u * BF_NT] = split_slice<2>(w, 0)[tid + u * BF_NT];
            ring[1 * BF_SLICE + tid + u * BF_NT] = split_slice<2>(w, 1)[tid + u * BF_NT];
        }
        split_stage<BF_NT, BfLds>(lds, w, a.cvec, a.tvec_all + (size_t)i * HEADS, wg_row0, a.nrows, a.kcand);
    }
    if (rs.finish_previous(a, lane)) return;
    // slice 2 travels in registers until step 0 deposits it
    bf16x8 hold[BF_PER_T];
#pragma unroll
    for (int u = 0; u < BF_PER_T; ++u) hold[u] = split_slice<2>(w, 2)[tid + u * BF_NT];
    __syncthreads();
    int gstep = 0;
    // one ring step: slice gstep + 2 (held since the previous step) -> its slot (last read in step gstep - 1), request slice gstep + 3;
    // acc[nc] += W[slice gstep][nc] . (xh, xl) for the 16 output chunks, two at a time; one barrier
    auto ring_step = [&](f32x4 (&acc)[16], const bf16x8 xh, const bf16x8 xl) {
        {
            bf16x8 *dst = ring + ((gstep + 2) % 3) * BF_SLICE;
#pragma unroll
            for (int u = 0; u < BF_PER_T; ++u) dst[tid + u * BF_NT] = hold[u];
            const bf16x8 *src = split_slice<2>(w, gstep + 3);
#pragma unroll
            for (int u = 0; u < BF_PER_T; ++u) hold[u] = src[tid + u * BF_NT];
        }
        const bf16x8 *slot = ring + (gstep % 3) * BF_SLICE;
#pragma unroll
        for (int n0 = 0; n0 < 16; n0 += 2) {
            bf16x8 wh[2], wl[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                wh[u] = slot[((n0 + u) * 2 + 0) * 64 + lane];
                wl[u] = slot[((n0 + u) * 2 + 1) * 64 + lane];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[n0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[u], xh, acc[n0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[n0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[u], xh, acc[n0 + u], 0, 0, 0);
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[n0 + u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[u], xl, acc[n0 + u], 0, 0, 0);
        }
        ++gstep;
        __syncthreads();
    };
    f32x4 acc[16];
    auto zero_acc = [&]() {
#pragma unroll
        for (int n = 0; n < 16; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    // bias + ReLU + split of a 256-wide hidden layer: k-block m of the next layer = chunks 2m, 2m+1
    auto hidden = [&](const float *bias, bf16x8 (&hh)[8], bf16x8 (&hl)[8]) {
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const f32x4 v0 = relu4(acc[2 * m] + *reinterpret_cast<const f32x4 *>(bias + 16 * (2 * m) + 4 * g));
            const f32x4 v1 = relu4(acc[2 * m + 1] + *reinterpret_cast<const f32x4 *>(bias + 16 * (2 * m + 1) + 4 * g));
            split8(v0, v1, hh[m], hl[m]);
        }
    };
    // ---- pose_encoder.0
    bf16x8 xh, xl;
    {
        f32x4 pa, pb;
        split_pose_fragment(rs.xv[0], g, pa, pb);
        split8(pa, pb, xh, xl);
    }
    bf16x8 h1h[8], h1l[8], h2h[8], h2l[8];
    zero_acc();
    ring_step(acc, xh, xl);
    hidden(b0l, h1h, h1l);
    // ---- pose_encoder.2
    zero_acc();
#pragma unroll
    for (int kb = 0; kb < 8; ++kb) ring_step(acc, h1h[kb], h1l[kb]);
    hidden(b2l, h2h, h2l);
    // ---- the three heads; their Linear(256, 3) output layers as fp32 dot products on the accumulator fragments
    const int r = rs.row[0] < a.nrows ? rs.row[0] : a.nrows - 1;
    const int cl = r / a.kcand - wg_row0 / a.kcand;  // < NCL (gp_pc_layout admits k only when a workgroup's rows span <= NCL clouds)
    float sc9[9];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        zero_acc();
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) ring_step(acc, h2h[kb], h2l[kb]);
        float o[3];
        split_head_out(acc, cvtl + cl * HEADS, woutl, h, g, o);
#pragma unroll
        for (int c = 0; c < 3; ++c) sc9[3 * h + c] = o[c];
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) sc9[j] = (sc9[j] + w.b_out[j]) / (rs.sigma + 1e-7f);
    float q[1] = {};
    pc_store_score(a, rs.row[0], lane, 0, sc9, q[0]);
    pc_store_partial<1, BF_NW>(a, rs.row, q, wave, lane);
}

}  // namespace

extern "C" {

/* rows per workgroup / partial sums per step of the split-bf16 PC launch for (ngroups x nclouds_per_group clouds x k candidates); GP_EINVAL when a
 * workgroup would straddle two batches or its 128 rows could span more than four clouds (k < 43) */
int gp_pc_layout_bf16x3(int ngroups, int nclouds_per_group, int k, int *nparts_out) {
    if (ngroups <= 0 || nclouds_per_group <= 0 || k <= 0 || !nparts_out) return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    if (ngroups > 1 && rg % BF_ROWS != 0) return GP_EINVAL;
    if ((BF_ROWS - 2 + k) / k + 1 > NCL) return GP_EINVAL;
    *nparts_out = ngroups * ((rg + BF_ROWS - 1) / BF_ROWS) * BF_NW;
    return GP_OK;
}

int gp_pc_step_bf16x3(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const float *cvec, const float *tvec_all, const float *sched,
                      const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x, float *score, float *partials,
                      float *traj, const void *w_pose0_split, const void *w_pose2_split, const void *w_headx_split, const float *b_pose0, const float *b_pose2,
                      const float *w_out, const float *b_out, gp_stream_t s) {
    if (step < 0 || step > nsteps || !cvec || !tvec_all || !sched || !z_langevin || !z_predictor || !centre || !x || !mean_x || !score || !partials ||
        !w_pose0_split || !w_pose2_split || !w_headx_split || !b_pose0 || !b_pose2 || !w_out || !b_out)
        return GP_EINVAL;
    int nparts = 0;
    const int rc = gp_pc_layout_bf16x3(ngroups, nclouds_per_group, k, &nparts);
    if (rc != GP_OK) return rc;
    const int rg = nclouds_per_group * k;
    const PcArgs a = pc_args(ngroups, rg, k, step, nsteps, nparts, (rg + BF_ROWS - 1) / BF_ROWS, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x,
                             mean_x, score, partials, traj, nullptr, 0);
    const SplitNet w = {reinterpret_cast<const bf16x8 *>(w_pose0_split), reinterpret_cast<const bf16x8 *>(w_pose2_split),
                        reinterpret_cast<const bf16x8 *>(w_headx_split), b_pose0, b_pose2, w_out, b_out};
    return gp_launch<pc_step_bf16x3_kernel>(dim3(a.wgpg * ngroups), dim3(BF_NT), BfLds::BYTES, (hipStream_t)s, a, w);
}

}  // extern "C"
