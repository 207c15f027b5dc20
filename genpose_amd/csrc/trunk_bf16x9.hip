// The chain plan (128 rows per workgroup) of the score model's predictor-corrector step (cond_pc_sampler, samplers.py:102-160) with the
// network's three dense layers as EXACT-PRODUCT split-bf16 on the BF16 matrix pipe (bf16x9.h): every fp32 operand is hi + mid + lo,
// all nine cross products are exact in fp32 and only the fp32 accumulation rounds - the error class of pc_step_chain_kernel<2, 0>
// (trunk_chain.h), which stays selectable (PCSampler(trunk="f32mfma")).  Same job, inputs and partials contract as that kernel:
// sampler update -> pose encoder -> three 256-wide heads -> fp32 Linear(256, 3) outputs on the accumulators -> one partial sum of
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
//   MFMA                33 x 16 chunks x 9 products x 2 tiles = 9 504 per wave x 16 cycles = 152 k cycles per SIMD (63 us at 2.4 GHz)
// so the matrix pipe bounds it, not LDS (bf16x3's 8 waves x 16 rows read the same 1.5 MB weight stream twice as often per row) and not
// the fp32 peak: 9 bf16 products per fp32 product at 16x the fp32 rate = 1.8x the fp32 MFMA FLOP rate.
// Measured (MI355X, 32 000 rows, rocprofv3): 118.0 us per launch against 142.7 us for pc_step_chain_kernel<2, 0>; the rest of the gap to
// the 63 us floor is barrier drains (one wave per SIMD), the head epilogues (not overlapped with MFMAs) and a few spilled registers.
#include "bf16x9.h"
#include "score_trunk.h"
#include "trunk_chain.h"

namespace {

using namespace gp_trunk;
using namespace gp_bf16x9;

struct PcX9Args {
    int nrows, kcand, step, nsteps;
    int nparts, ppg, rows_per_group, wgpg;  // as PcArgs (scorenet.hip): one partial per wave, nparts from gp_pc_layout(0, 128, ...)
    const float *cvec, *tvec_all, *sched, *z_lang, *z_pred, *centre;
    float *x, *mean_x, *score, *partials, *traj;
    const float *gn_ext;  // [nsteps][ngroups] or null: the batch's statistic from outside (sum over gn_rows rows when gn_rows > 0)
    int ngroups;
    float gn_rows;
    const bf16x8 *w0;  // pose_encoder.0 [1][16][3][64]   k = component index (natural order, zero padded to 32)
    const bf16x8 *w2;  // pose_encoder.2 [8][16][3][64]   k order of the register chain (weights.pack_bf16x9)
    const bf16x8 *wh;  // stacked heads  [8][48][3][64]
    const float *b0, *b2, *w_out, *b_out;  // fp32: biases [256], [256]; output layers [9][256], [9]
};

constexpr int X9_NW = 4, X9_NT = 64 * X9_NW, X9_RT = 2, X9_ROWS = 16 * X9_RT * X9_NW, X9_NCL = 4;
constexpr int X9_SLICE = 16 * 3 * 64;  // bf16x8 (16 B) per slice = 48 KB
constexpr int X9_PER_T = X9_SLICE / X9_NT;
constexpr int X9_NSLICES = 33;
static_assert(X9_ROWS == 128 && X9_PER_T <= 16, "one slice element per thread and output chunk at most");
// LDS (floats): ring [2][SLICE] bf16x8 | w_out [9][256] | b0 [256] | b2 [256] | cvt [NCL][768] = cvec[cloud] + tvec
constexpr int X9_OFF_WOUT = 2 * X9_SLICE * 4, X9_OFF_B0 = X9_OFF_WOUT + POSE * HID, X9_OFF_B2 = X9_OFF_B0 + HID, X9_OFF_CVT = X9_OFF_B2 + HID,
              X9_TOTAL = X9_OFF_CVT + X9_NCL * HEADS;
constexpr size_t X9_LDS_BYTES = (size_t)X9_TOTAL * sizeof(float);
static_assert(X9_LDS_BYTES <= 160 * 1024, "LDS");

__device__ __forceinline__ const bf16x8 *x9_slice(const PcX9Args &a, int s) {
    s = s < X9_NSLICES ? s : X9_NSLICES - 1;  // the ring runs ahead: requests past the end re-read the last slice (never used)
    if (s == 0) return a.w0;
    if (s <= 8) return a.w2 + (size_t)(s - 1) * X9_SLICE;
    const int h = (s - 9) >> 3, kb = (s - 9) & 7;
    return a.wh + ((size_t)kb * 48 + 16 * h) * 3 * 64;
}

// End of a ring step: this wave's LDS writes of the step have completed (lgkmcnt), then the bare barrier.  No vmcnt wait: the
// slice in flight to the registers may stay in flight across it.  The empty asm statements keep LDS accesses on their side.
__device__ __forceinline__ void x9_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

__global__ __launch_bounds__(X9_NT, 1) void pc_step_chain_kernel_bf16x9(PcX9Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);
    float *woutl = lds + X9_OFF_WOUT, *b0l = lds + X9_OFF_B0, *b2l = lds + X9_OFF_B2, *cvtl = lds + X9_OFF_CVT;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), pt = lane & 15, g = lane >> 4, i = a.step;
    const int wg_row0 = blockIdx.x * X9_ROWS;
    int row[X9_RT];
#pragma unroll
    for (int p = 0; p < X9_RT; ++p) row[p] = wg_row0 + (wave * X9_RT + p) * 16 + pt;
    // ---- the rows' operands first, the ring prologue behind them (memory returns in order)
    float xv[X9_RT][9], gr[X9_RT][9], zz1[X9_RT][9], zz2[X9_RT][9], cen[X9_RT][3];
    float gdiff = 0.f, dt = 0.f, sqdt = 0.f, gn = 1.f, sigma = 1.f;
#pragma unroll
    for (int p = 0; p < X9_RT; ++p) {
        const int r = row[p] < a.nrows ? row[p] : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
#pragma unroll
        for (int j = 0; j < 9; ++j) xv[p][j] = a.x[(size_t)r * 9 + j];
        if (i > 0) {
            const float *z1 = a.z_lang + ((size_t)(i - 1) * a.nrows + r) * 9;
            const float *z2 = a.z_pred + ((size_t)(i - 1) * a.nrows + r) * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                gr[p][j] = a.score[(size_t)r * 9 + j];
                zz1[p][j] = z1[j];
                zz2[p][j] = z2[j];
            }
            const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
            cen[p][0] = cp[0], cen[p][1] = cp[1], cen[p][2] = cp[2];
        }
    }
    float psum[4] = {0.f, 0.f, 0.f, 0.f};
    const int grp = blockIdx.x / a.wgpg;
    const float *pp = a.partials + (size_t)(i > 0 ? i - 1 : 0) * a.nparts + (size_t)grp * a.ppg;
    if (i > 0) {
        const float *sc = a.sched + (size_t)(i - 1) * 4;
        gdiff = sc[1], dt = sc[2], sqdt = sc[3];
        if (a.gn_ext) {
            gn = a.gn_ext[(size_t)(i - 1) * a.ngroups + grp];
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) psum[u] = lane + 64 * u < a.ppg ? pp[lane + 64 * u] : 0.f;
        }
    }
    // slice 0 (-> slot 0 below) and slice 1 (-> registers, written during step 0)
    bf16x8 first[X9_PER_T], hold[X9_PER_T];
    if (i < a.nsteps) {
        sigma = a.sched[(size_t)i * 4 + 0];
#pragma unroll
        for (int u = 0; u < X9_PER_T; ++u) first[u] = x9_slice(a, 0)[tid + u * X9_NT];
#pragma unroll
        for (int u = 0; u < X9_PER_T; ++u) hold[u] = x9_slice(a, 1)[tid + u * X9_NT];
    }
    if (i > 0) {
        if (a.gn_ext) {
            if (a.gn_rows > 0.f) gn = gn / a.gn_rows;
        } else {
            float s = ((psum[0] + psum[1]) + psum[2]) + psum[3];  // pc_step_chain_kernel's order
            for (int q = lane + 256; q < a.ppg; q += 64) s += pp[q];
            gn = wave_sum_f32(s) / (float)a.rows_per_group;
        }
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            float mx[9];
            pc_update_row(xv[p], gr[p], zz1[p], zz2[p], gn, gdiff, dt, sqdt, mx);
            if (row[p] < a.nrows && g == 0) {
                const int r = row[p];
                if (a.traj) {
                    float *tr = a.traj + ((size_t)(i - 1) * a.nrows + r) * 9;
#pragma unroll
                    for (int j = 0; j < 6; ++j) tr[j] = xv[p][j];
#pragma unroll
                    for (int j = 0; j < 3; ++j) tr[6 + j] = xv[p][6 + j] + cen[p][j];
                }
#pragma unroll
                for (int j = 0; j < 9; ++j) a.x[(size_t)r * 9 + j] = xv[p][j];
                if (i == a.nsteps) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) mx[6 + j] += cen[p][j];
                    normalize_rot6(mx);
#pragma unroll
                    for (int j = 0; j < 9; ++j) a.mean_x[(size_t)r * 9 + j] = mx[j];
                }
            }
        }
        if (i == a.nsteps) return;
    }
    // ---- staged epilogue operands and slot 0
    for (int e = tid; e < POSE * HID; e += X9_NT) woutl[e] = a.w_out[e];
    for (int e = tid; e < HID; e += X9_NT) b0l[e] = a.b0[e], b2l[e] = a.b2[e];
    {
        const float *tvec = a.tvec_all + (size_t)i * HEADS;
        const int cloud0 = wg_row0 / a.kcand, last_cloud = (a.nrows - 1) / a.kcand;
        for (int e = tid; e < X9_NCL * HEADS; e += X9_NT) {
            const int c = e / HEADS, o = e - c * HEADS;
            const int cl = cloud0 + c < last_cloud ? cloud0 + c : last_cloud;
            cvtl[e] = a.cvec[(size_t)cl * HEADS + o] + tvec[o];
        }
    }
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
        const bf16x8 *src = x9_slice(a, gstep + 2);
        bf16x8 w[2][3];
#pragma unroll
        for (int t = 0; t < 3; ++t) w[0][t] = slot[t * 64 + lane];
#pragma unroll
        for (int n = 0; n < 16; ++n) {
            if (n + 1 < 16) {
#pragma unroll
                for (int t = 0; t < 3; ++t) w[(n + 1) & 1][t] = slot[((n + 1) * 3 + t) * 64 + lane];
            }
            if (n < X9_PER_T) {
                dst[tid + n * X9_NT] = hold[n];
                hold[n] = src[tid + n * X9_NT];
            }
            f32x4 an[X9_RT];
#pragma unroll
            for (int p = 0; p < X9_RT; ++p) an[p] = acc[p][n];
            mma9<X9_RT>(w[n & 1], xs, an);
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
    // ---- pose_encoder.0: the row's nine components as the one (zero-padded) k-block, natural k order: lane group g holds k = 8g .. 8g+7
    {
        Split8 xs[X9_RT];
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
            f32x4 pa = {0.f, 0.f, 0.f, 0.f}, pb = {0.f, 0.f, 0.f, 0.f};
            if (g == 0) pa = f32x4{xv[p][0], xv[p][1], xv[p][2], xv[p][3]}, pb = f32x4{xv[p][4], xv[p][5], xv[p][6], xv[p][7]};
            if (g == 1) pa = f32x4{xv[p][8], 0.f, 0.f, 0.f};
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
        const int r = row[p] < a.nrows ? row[p] : a.nrows - 1;
        cl[p] = r / a.kcand - wg_row0 / a.kcand;  // < NCL (gp_pc_layout admits k only when a workgroup's rows span <= NCL clouds)
    }
    // each head's three score components are final once its epilogue is done: stored there, their squares summed in component order
    const float sden = sigma + 1e-7f;
    float q[X9_RT] = {};
#pragma unroll 1
    for (int h = 0; h < 3; ++h) {
        layer();
#pragma unroll
        for (int p = 0; p < X9_RT; ++p) {
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
            const float sc[3] = {(lane_groups_sum(o0) + a.b_out[3 * h + 0]) / sden, (lane_groups_sum(o1) + a.b_out[3 * h + 1]) / sden,
                                 (lane_groups_sum(o2) + a.b_out[3 * h + 2]) / sden};
#pragma unroll
            for (int c = 0; c < 3; ++c) q[p] += sc[c] * sc[c];
            if (row[p] < a.nrows && g == 0) {
#pragma unroll
                for (int c = 0; c < 3; ++c) a.score[(size_t)row[p] * 9 + 3 * h + c] = sc[c];
            }
        }
    }
    float nsum = 0.f;
#pragma unroll
    for (int p = 0; p < X9_RT; ++p)
        if (row[p] < a.nrows && g == 0) nsum += sqrtf(q[p]);
    nsum = wave_sum_f32(nsum);
    if (lane == 0) a.partials[(size_t)i * a.nparts + (size_t)blockIdx.x * X9_NW + wave] = nsum;
}

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
    PcX9Args a;
    a.nrows = ngroups * rg, a.kcand = k, a.step = step, a.nsteps = nsteps;
    a.wgpg = (rg + X9_ROWS - 1) / X9_ROWS, a.nparts = nparts, a.ppg = nparts / ngroups, a.rows_per_group = rg;
    a.cvec = cvec, a.tvec_all = tvec_all, a.sched = sched, a.z_lang = z_langevin, a.z_pred = z_predictor, a.centre = centre;
    a.x = x, a.mean_x = mean_x, a.score = score, a.partials = partials, a.traj = traj;
    a.gn_ext = gn_ext, a.ngroups = ngroups, a.gn_rows = (float)gn_rows_total;
    a.w0 = reinterpret_cast<const bf16x8 *>(w_pose0_x9), a.w2 = reinterpret_cast<const bf16x8 *>(w_pose2_x9),
    a.wh = reinterpret_cast<const bf16x8 *>(w_headx_x9);
    a.b0 = net->b_pose0, a.b2 = net->b_pose2, a.w_out = net->w_out, a.b_out = net->b_out;
    static bool done = false;
    if (!done) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(pc_step_chain_kernel_bf16x9), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)X9_LDS_BYTES) != hipSuccess)
            return GP_ELAUNCH;
        done = true;
    }
    hipLaunchKernelGGL(pc_step_chain_kernel_bf16x9, dim3(a.wgpg * ngroups), dim3(X9_NT), X9_LDS_BYTES, (hipStream_t)s, a);
    return gp_launch_status();
}

}  // extern "C"
