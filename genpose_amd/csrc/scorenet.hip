// PoseScoreNet / PoseEnergyNet evaluation and the predictor-corrector sampler step for gfx950.
// Reference: networks/gf_algorithms/scorenet.py:178-222, energynet.py:143-198, samplers.py:102-160.
//
// Exact algebra used to cut the per-evaluation work: the first Linear of each head acts on
// cat[pts_feat(1024), t_feat(128), pose_feat(256)], so
//     W1 . total = W1p . pts_feat (once per cloud: gp_cloud_embed)
//                + W1t . t_feat   (once per time value, shared by every row: gp_time_embed)
//                + W1x . pose_feat (per row, per evaluation: here, on fp32 MFMA)
// The three heads are stacked into one 768-wide layer; their 256->3 output layers are applied in the
// accumulator epilogue (no 768-wide activation ever reaches LDS).
#include "pc_rows.h"
#include "score_bwd.h"
#include "trunk_chain_vjp.h"

namespace {

using namespace gp_trunk;

// ---------------------------------------------------------------------------------------------- cloud embed
// cvec[b, 768] = Wp[768 x 1024] . pts_feat[b] + b_head : plain MFMA GEMM, 16 clouds per workgroup.
__global__ __launch_bounds__(256) void cloud_embed_kernel(int nb, gp_scorenet net, const float *__restrict__ pts_feat, float *__restrict__ cvec) {
    constexpr int K = 1024, LD = K + GP_LD_PAD;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = blockIdx.x * 16;
    for (int e = tid; e < 16 * (K / 4); e += 256) {
        const int r = e / (K / 4), q = e - r * (K / 4);
        int g = r0 + r;
        if (g >= nb) g = nb - 1;
        *reinterpret_cast<f32x4 *>(lds + r * LD + 4 * q) = *reinterpret_cast<const f32x4 *>(pts_feat + (size_t)g * K + 4 * q);
    }
    __syncthreads();
    // 48 n-chunks: blockIdx.y selects a group of 16, each wave takes 4 of them
    const int ncb = blockIdx.y * 16 + wave * 4;
    int nc[4] = {ncb, ncb + 1, ncb + 2, ncb + 3};
    f32x4 acc[4][1];
    mfma_tile<4, 1>(lds, LD, 0, net.w_headp, K / 16, HEADS / 16, nc, acc);
    const int row = r0 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = nc[i] * 16 + 4 * (lane >> 4);
        const f32x4 v = acc[i][0] + *reinterpret_cast<const f32x4 *>(net.b_head + ch);
        if (row < nb) *reinterpret_cast<f32x4 *>(cvec + (size_t)row * HEADS + ch) = v;
    }
}

// ---------------------------------------------------------------------------------------------- time embed
// tvec[i, 768] = W1t . relu(Wt1 . [sin(x), cos(x)] + bt1),  x = t * W * 2 * pi   (scorenet.py:55-64,111-116)
// w_t1 and w_headt arrive TRANSPOSED ([k][n]) so consecutive threads read consecutive words.
// grid (nt, ngroups): group g reads its nt time values at t + g * t_stride and writes tvec rows [g*nt, (g+1)*nt)
__global__ __launch_bounds__(256) void time_embed_kernel(gp_scorenet net, const float *__restrict__ t, size_t t_stride, float *__restrict__ tvec) {
    __shared__ float four[128], tf[128];
    const int tid = threadIdx.x;
    const float tv = t[(size_t)blockIdx.y * t_stride + blockIdx.x];
    tvec += (size_t)blockIdx.y * gridDim.x * HEADS;
    if (tid < 64) {
        const float xp = ((tv * net.fourier_w[tid]) * 2.0f) * 3.14159274101257324f;  // f32 evaluation order of the reference
        four[tid] = sinf(xp);
        four[tid + 64] = cosf(xp);
    }
    __syncthreads();
    if (tid < 128) {
        float acc = 0.f;
        for (int k = 0; k < 128; ++k) acc = fmaf(four[k], net.w_t1[k * 128 + tid], acc);
        tf[tid] = fmaxf(acc + net.b_t1[tid], 0.f);
    }
    __syncthreads();
    // three outputs per thread, their k-ordered fmaf chains interleaved (same arithmetic per output, 3x the ILP)
    static_assert(HEADS == 3 * 256, "one pass of three outputs per thread");
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    const float *w = net.w_headt + tid;
#pragma unroll 4
    for (int k = 0; k < 128; ++k) {
        const float tk = tf[k];
        a0 = fmaf(tk, w[k * HEADS], a0);
        a1 = fmaf(tk, w[k * HEADS + 256], a1);
        a2 = fmaf(tk, w[k * HEADS + 512], a2);
    }
    float *o = tvec + (size_t)blockIdx.x * HEADS + tid;
    o[0] = a0, o[256] = a1, o[512] = a2;
}

// mode 0: score = f/(sigma+1e-7)  (scorenet.py:217);  mode 1: IP energy with s = f/sigma (energynet.py:163-185)
template <int P>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void score_eval_kernel(int nrows, int kcand, gp_scorenet net, const float *__restrict__ cvec,
                                                         const float *__restrict__ tvec, const float *__restrict__ x,
                                                         const float *__restrict__ sigma_dev, int mode, float *__restrict__ out) {
    using L = TrunkLds<P>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int row0 = blockIdx.x * P, tid = threadIdx.x;
    TrunkPre<P> pre;
    trunk_begin<P>(net, pre, cvec, tvec, row0, nrows, kcand);
    float sigma = *sigma_dev;  // requested now, used after the trunk
    gp_pin(sigma);
    load_x_tile<P>(lds, x, row0, nrows);
    __syncthreads();
    trunk_ftheta<P>(lds, net, cvec, tvec, row0, nrows, kcand, pre);
    const float *F = lds + L::OFF_H1;
    if (mode == 0) {
        for (int e = tid; e < P * POSE; e += TrunkCfg<P>::NT) {
            const int r = e / POSE, j = e - r * POSE;
            if (row0 + r < nrows) out[(size_t)(row0 + r) * POSE + j] = F[r * L::LDH + j] / (sigma + 1e-7f);
        }
    } else if (tid < P) {
        const int r = tid;
        if (row0 + r < nrows) {
            const float *xr = lds + r * L::LD0;
            float er = 0.f, et = 0.f;
#pragma unroll
            for (int j = 0; j < 6; ++j) er += xr[j] * (F[r * L::LDH + j] / sigma);
#pragma unroll
            for (int j = 6; j < 9; ++j) et += xr[j] * (F[r * L::LDH + j] / sigma);
            out[(size_t)(row0 + r) * 2 + 0] = er;
            out[(size_t)(row0 + r) * 2 + 1] = et;
        }
    }
}

// chain form (trunk_chain.h): one wave per 16 rows, the row's pose and outputs stay in its lanes
template <int PT>
__global__ __launch_bounds__(gp_chain::NT, 1) void score_eval_chain_kernel(int nrows, int kcand, gp_scorenet net, const float *__restrict__ cvec,
                                                                                                 const float *__restrict__ tvec, const float *__restrict__ x,
                                                                                                 const float *__restrict__ sigma_dev, int mode, float *__restrict__ out) {
    using C = gp_chain::Cfg<PT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, pt = lane & 15, g = lane >> 4;
    const int wg_row0 = blockIdx.x * C::ROWS;
    gp_chain::State<PT> st;
    gp_chain::begin<PT>(st, lds, net, cvec, tvec, wg_row0, nrows, kcand);
    const float sigma = *sigma_dev;
    float xv[PT][POSE];
    f32x4 xf[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        int r = wg_row0 + (wave * PT + p) * 16 + pt;
        r = r < nrows ? r : nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
#pragma unroll
        for (int j = 0; j < POSE; ++j) xv[p][j] = x[(size_t)r * POSE + j];
        xf[p] = gp_chain::pose_fragment(xv[p], g);
    }
    float f[PT][POSE];
    gp_chain::run<PT>(st, lds, net, xf, f);
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        const int r = wg_row0 + (wave * PT + p) * 16 + pt;
        if (r >= nrows || g != 0) continue;
        if (mode == 0) {
#pragma unroll
            for (int j = 0; j < POSE; ++j) out[(size_t)r * POSE + j] = f[p][j] / (sigma + 1e-7f);
        } else {
            float er = 0.f, et = 0.f;
#pragma unroll
            for (int j = 0; j < 6; ++j) er += xv[p][j] * (f[p][j] / sigma);
#pragma unroll
            for (int j = 6; j < 9; ++j) et += xv[p][j] * (f[p][j] / sigma);
            out[(size_t)r * 2 + 0] = er;
            out[(size_t)r * 2 + 1] = et;
        }
    }
}

// ---------------------------------------------------------------------------------------------- PC sampler
// PcArgs: pc_rows.h (the argument block of every plan; the wave-level front and back end of the chain plans live there too)

// Kernel for step i (0 <= i <= nsteps):
//   i > 0      : finish step i-1 for the tile's rows (Langevin corrector + Euler-Maruyama predictor, samplers.py:129-152)
//                using score_{i-1} and the batch-mean gradient norm reduced from every block's partial sum
//   i < nsteps : evaluate score_i = s(x_i, t_i) and write this block's partial sum of |score_i|_2
//   i == nsteps: (finish only) also post-process mean_x (:157-158)
// MODEL 0: the score network (score = f / (sigma + 1e-7), scorenet.py:217).  MODEL 1: the ENERGY network, whose score is the
// gradient of its inner-product energy (energynet.py:200-222): forward + vector-Jacobian product in the tile (score_bwd.h), 16-row
// tiles only.  The same kernel otherwise: sampling from the energy model is the same captured launch chain.
// SPLIT: the head-split plan (see PcArgs): three workgroups per tile.  Each finishes step i-1 for all 16 rows (the update is row-local
// and cheap; identical in the three, workgroup h = 0 stores) and evaluates ONE head of the score at t_i.
// SEEDED (pc_step_seeded_kernel below): the rows' noise is not loaded from z_lang / z_pred but drawn in registers (philox.h; the seed
// state sits behind a.z_lang) - everything after the draw is the same expression.
template <int P, int MODEL, bool SPLIT, bool SEEDED>
__device__ __forceinline__ void pc_step_tile(const PcArgs &a, const gp_scorenet &net) {
    static_assert(MODEL == 0 || P == gp_bwd::DP, "the backward pass runs on 16-row tiles");
    static_assert(!SPLIT || (MODEL == 0 && P == 16), "head-split: score model, 16-row tiles");
    using L = TrunkLds<P, MODEL == 1>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ float s_gn;
    const int tile = SPLIT ? blockIdx.x / 3 : blockIdx.x, hsel = SPLIT ? blockIdx.x - 3 * tile : 0;
    const int row0 = tile * P, tid = threadIdx.x, i = a.step;
    // SPLIT: three workgroups READ a tile's state and score and each writes a part - in place that would be a race between workgroups
    // (a workgroup dispatched late would read what a sibling has already written).  Launch i reads step i-1's copies and writes its own
    // (PcArgs).  The finish-only launch needs one workgroup per tile.
    if (SPLIT && i == a.nsteps && hsel != 0) return;
    const size_t R = (size_t)a.nrows;
    const float *prev = SPLIT && i > 0 ? a.partials + (size_t)(i - 1) * a.nparts : nullptr;
    float *mine = SPLIT && i < a.nsteps ? a.partials + (size_t)i * a.nparts : nullptr;
    const float *x_in = SPLIT ? (i <= 1 ? a.x : prev + 12 * R) : a.x;
    const float *score_in = SPLIT && i > 0 ? prev + 3 * R : a.score;
    float *x_out = SPLIT ? (mine ? mine + 12 * R : nullptr) : a.x;
    TrunkPre<P> pre;
    float sigma = 1.f;
    if (i < a.nsteps) {
        trunk_begin<P>(net, pre, a.cvec, a.tvec_all + (size_t)i * HEADS, row0, a.nrows, a.kcand);
        sigma = a.sched[(size_t)i * 4 + 0];  // requested now, used after the trunk
        gp_pin(sigma);
    }
    if (i > 0) {
        // (1) row threads request their operands first; (2) meanwhile the last wave reduces the per-block partial sums
        // of step i-1 into the batch-mean gradient norm (fixed order: deterministic); (3) one barrier, then the update.
        const bool live = row0 + tid < a.nrows;
        const int r = live ? row0 + tid : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
        float xv[9], gr[9], zz1[9], zz2[9], g = 0.f, dt = 0.f, sqdt = 0.f, cen[3] = {0.f, 0.f, 0.f};
        if (tid < P) {
            const float *sc = a.sched + (size_t)(i - 1) * 4;
            g = sc[1], dt = sc[2], sqdt = sc[3];
            if constexpr (SEEDED) {
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    xv[j] = x_in[(size_t)r * 9 + j];
                    gr[j] = score_in[(size_t)r * 9 + j];
                }
                const gp_philox::Seed sd = gp_philox::load_seed(reinterpret_cast<const uint32_t *>(a.z_lang));
                gp_philox::draw9(sd, (uint32_t)(i - 1), gp_philox::STREAM_LANGEVIN, sd.row_base + (uint64_t)r, zz1);
                gp_philox::draw9(sd, (uint32_t)(i - 1), gp_philox::STREAM_PREDICTOR, sd.row_base + (uint64_t)r, zz2);
            } else {
                const float *z1 = a.z_lang + ((size_t)(i - 1) * a.nrows + r) * 9;
                const float *z2 = a.z_pred + ((size_t)(i - 1) * a.nrows + r) * 9;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    xv[j] = x_in[(size_t)r * 9 + j];
                    gr[j] = score_in[(size_t)r * 9 + j];
                    zz1[j] = z1[j];
                    zz2[j] = z2[j];
                }
            }
            const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
            cen[0] = cp[0], cen[1] = cp[1], cen[2] = cp[2];
        }
        constexpr int LASTW = TrunkCfg<P>::NT - 64;
        if (a.gn_ext) {
            if (tid == LASTW) {
                const float v = a.gn_ext[(size_t)(i - 1) * a.ngroups + tile / a.wgpg];
                s_gn = a.gn_rows > 0.f ? v / a.gn_rows : v;
            }
        } else if (tid >= LASTW) {
            float s = 0.f;
            const float *pp = a.partials + (size_t)(i - 1) * a.nparts + (size_t)(tile / a.wgpg) * (SPLIT ? 3 * a.rows_per_group : a.ppg);
            if constexpr (SPLIT) {
                for (int r = tid - LASTW; r < a.rows_per_group; r += 64) s += sqrtf((pp[3 * r] + pp[3 * r + 1]) + pp[3 * r + 2]);
            } else {
                for (int q = tid - LASTW; q < a.ppg; q += 64) s += pp[q];
            }
            s = wave_sum_f32(s);
            if (tid == LASTW) s_gn = s / (float)a.rows_per_group;
        }
        __syncthreads();
        if (tid < P) {
            float mx[9];
            pc_update_row(xv, gr, zz1, zz2, s_gn, g, dt, sqdt, mx);
            if (live && hsel == 0) {
                if (a.traj) {
                    float *tr = a.traj + ((size_t)(i - 1) * a.nrows + r) * 9;
#pragma unroll
                    for (int j = 0; j < 6; ++j) tr[j] = xv[j];
#pragma unroll
                    for (int j = 0; j < 3; ++j) tr[6 + j] = xv[6 + j] + cen[j];
                }
                if (x_out) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) x_out[(size_t)r * 9 + j] = xv[j];
                }
                if (i == a.nsteps) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) mx[6 + j] += cen[j];
                    normalize_rot6(mx);
#pragma unroll
                    for (int j = 0; j < 9; ++j) a.mean_x[(size_t)r * 9 + j] = mx[j];
                }
            }
            // hand the new state to the trunk through LDS (no global round trip)
            float *xr = lds + tid * L::LD0;
#pragma unroll
            for (int j = 0; j < 9; ++j) xr[j] = xv[j];
#pragma unroll
            for (int j = 9; j < 16; ++j) xr[j] = 0.f;
        }
        if (i == a.nsteps) return;
    } else {
        load_x_tile<P>(lds, a.x, row0, a.nrows);
    }
    __syncthreads();
    float *F;
    int ldf;
    if constexpr (MODEL == 0) {
        trunk_ftheta<P, false, TrunkNoEmit, SPLIT>(lds, net, a.cvec, a.tvec_all + (size_t)i * HEADS, row0, a.nrows, a.kcand, pre, TrunkNoEmit(), hsel);
        F = lds + L::OFF_H1, ldf = L::LDH;
        for (int e = tid; e < P * POSE; e += TrunkCfg<P>::NT) {
            const int r = e / POSE, j = e - r * POSE;
            if (SPLIT && j / 3 != hsel) continue;
            const float v = F[r * ldf + j] / (sigma + 1e-7f);
            F[r * ldf + j] = v;
            if (row0 + r < a.nrows) {
                a.score[(size_t)(row0 + r) * POSE + j] = v;  // (an output only under the head-split plan: nothing reads it back)
                if (SPLIT) mine[3 * R + (size_t)(row0 + r) * POSE + j] = v;
            }
        }
    } else {
        F = const_cast<float *>(gp_bwd::score_vjp_tile<gp_bwd::ENERGY>(lds, net, a.cvec, a.tvec_all + (size_t)i * HEADS, row0, a.nrows, a.kcand, pre, sigma));
        ldf = gp_bwd::LDS_OUT;
        for (int e = tid; e < P * POSE; e += TrunkCfg<P>::NT) {
            const int r = e / POSE, j = e - r * POSE;
            if (row0 + r < a.nrows) a.score[(size_t)(row0 + r) * POSE + j] = F[r * ldf + j];
        }
    }
    __syncthreads();
    if constexpr (SPLIT) {
        // per row: the sum of squares of this head's three components (the row's norm is put together by the next launch)
        if (tid < P && row0 + tid < a.nrows) {
            const float *f = F + tid * ldf + 3 * hsel;
            mine[3 * (size_t)(row0 + tid) + hsel] = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
        }
        return;
    }
    if (tid < 64) {
        float s = 0.f;
        for (int r = tid; r < P; r += 64) {
            if (row0 + r < a.nrows) {
                float q = 0.f;
#pragma unroll
                for (int j = 0; j < 9; ++j) q += F[r * ldf + j] * F[r * ldf + j];
                s += sqrtf(q);
            }
        }
        s = wave_sum_f32(s);
        if (tid == 0) a.partials[(size_t)i * a.nparts + blockIdx.x] = s;
    }
}

template <int P, int MODEL, bool SPLIT = false>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void pc_step_kernel(PcArgs a, gp_scorenet net) {
    pc_step_tile<P, MODEL, SPLIT, false>(a, net);
}
template <int P, bool SPLIT = false>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void pc_step_seeded_kernel(PcArgs a, gp_scorenet net) {
    pc_step_tile<P, 0, SPLIT, true>(a, net);
}

// A launch of the fixed-step Heun solver of the probability-flow ODE (cond_edm_sampler's method, samplers.py:230-290, on the VE score
// model; HeunArgs, pc_rows.h) in the tile form: pc_step_tile's shape - row work on tid < P, the evaluation point handed to the trunk
// through LDS - with the row-local heun_update_row in place of the PC update: no noise, no gradient norm, no partial sums, so no barrier
// before the update and nothing after the score stores.  Whole tiles.
// SOLVER_DPM2M (dpm2m_step_kernel): a launch of the DPM-Solver++(2M) solver (pc_rows.h) - its schedule row, dpm2m_update_row, `d` holds
// D_{i-2}; everything else is the same text.
// MODEL 1 (heun_step_kernel<16, energy>, dpm2m_step_kernel<16, energy>): the ENERGY network drives the solver with ITS score, the gradient
// of the inner-product energy (energynet.py:200-222) - forward + vector-Jacobian product in the tile as in pc_step_tile<16, 1>; the nine
// words score_vjp_tile leaves are the score itself (f / sigma + J_f^T (x / sigma), no 1e-7f) and are stored as they come.
// Args = HeunClsArgs (heun_step_classes_kernel, dpm2m_step_classes_kernel; score model): SCHEDULE CLASSES (pc_rows.h) - the row thread reads
// its cloud's class's schedule row, the trunk adds that class's time embedding per cloud, and every score entry is divided by its own row's
// sigma (requested before the trunk like the launch-wide one); the kind and DPM2M's first-step flag come from class 0.  The same text
// otherwise, so a row's bits are the uniform launch's on its class's tables.
template <int P, int SOLVER = SOLVER_HEUN, int MODEL = 0, class Args = HeunArgs>
__device__ __forceinline__ void heun_step_tile(const Args &a, const gp_scorenet &net) {
    static_assert(MODEL == 0 || P == gp_bwd::DP, "the backward pass runs on 16-row tiles");
    constexpr bool CLS = std::is_same<Args, HeunClsArgs>::value;
    static_assert(!CLS || MODEL == 0, "schedule classes: the score model");
    using L = TrunkLds<P, MODEL == 1>;
    constexpr int SROW = fixed_sched_row<SOLVER>(), NSG = (P * POSE + TrunkCfg<P>::NT - 1) / TrunkCfg<P>::NT;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int row0 = blockIdx.x * P, tid = threadIdx.x, i = a.step;
    const float *tvec = a.tvec_all + (size_t)pc_time_row<SOLVER>(i) * HEADS;  // (class 0's row)
    const auto tv = heun_times(a);
    TrunkPre<P> pre;
    float sigma = 1.f;
    float sg[NSG];  // CLS: the sigma of the row of each score entry this thread stores
    if (i < a.nsteps) {
        trunk_begin<P>(net, pre, a.cvec, tvec, row0, a.nrows, a.kcand, tv);
        if constexpr (CLS) {
#pragma unroll
            for (int q = 0; q < NSG; ++q) {
                const int r = row0 + (tid + q * TrunkCfg<P>::NT) / POSE;
                sg[q] = heun_sched_row<SROW>(a, heun_row_class(a, r < a.nrows ? r : a.nrows - 1), i)[0];
                gp_pin(sg[q]);
            }
        } else {
            sigma = a.sched[(size_t)i * SROW + 0];  // requested now, used after the trunk
            gp_pin(sigma);
        }
    }
    if (i > 0) {
        if (tid < P) {
            const bool live = row0 + tid < a.nrows;
            const int r = live ? row0 + tid : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
            const float *sc0 = a.sched + (size_t)i * SROW, *sc = heun_sched_row<SROW>(a, heun_row_class(a, r), i);  // control flow from class 0, numbers from the row's class
            const int kind = (int)sc0[3];
            const float c = sc[1], h = sc[2];
            float xv[9], gr[9], dv[9], cen[3];
            if constexpr (SOLVER == SOLVER_DPM2M) {
                const bool has_d = (kind == DPM2M_STEP || kind == DPM2M_STEP_LAST) && sc0[5] != 0.f;
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    xv[j] = a.x[(size_t)r * 9 + j];
                    gr[j] = a.score[(size_t)r * 9 + j];
                    dv[j] = has_d ? a.d[(size_t)r * 9 + j] : 0.f;
                }
            } else {
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    xv[j] = a.x[(size_t)r * 9 + j];
                    gr[j] = a.score[(size_t)r * 9 + j];
                    dv[j] = kind == HEUN_CORRECT || kind == HEUN_CORRECT_LAST ? a.d[(size_t)r * 9 + j] : 0.f;
                }
            }
            const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
            cen[0] = cp[0], cen[1] = cp[1], cen[2] = cp[2];
            if constexpr (SOLVER == SOLVER_DPM2M)
                dpm2m_update_row(kind, xv, dv, gr, c, h, sc[4], sc[5]);
            else
                heun_update_row(kind, xv, dv, gr, c, h);
            if (live) heun_store_row<SOLVER>(a, kind, r, xv, dv, cen);
            // hand the evaluation point to the trunk through LDS (no global round trip)
            float *xr = lds + tid * L::LD0;
#pragma unroll
            for (int j = 0; j < 9; ++j) xr[j] = xv[j];
#pragma unroll
            for (int j = 9; j < 16; ++j) xr[j] = 0.f;
        }
        if (i == a.nsteps) return;
    } else {
        load_x_tile<P>(lds, a.x, row0, a.nrows);
    }
    __syncthreads();
    if constexpr (MODEL == 0) {
        trunk_ftheta<P, false, TrunkNoEmit, false, (P == 48)>(lds, net, a.cvec, tvec, row0, a.nrows, a.kcand, pre, TrunkNoEmit(), 0, tv);
        const float *F = lds + L::OFF_H1;
        if constexpr (CLS) {
#pragma unroll
            for (int q = 0; q < NSG; ++q) {
                const int e = tid + q * TrunkCfg<P>::NT, r = e / POSE, j = e - r * POSE;
                if (e < P * POSE && row0 + r < a.nrows) a.score[(size_t)(row0 + r) * POSE + j] = F[r * L::LDH + j] / (sg[q] + 1e-7f);
            }
        } else {
            for (int e = tid; e < P * POSE; e += TrunkCfg<P>::NT) {
                const int r = e / POSE, j = e - r * POSE;
                if (row0 + r < a.nrows) a.score[(size_t)(row0 + r) * POSE + j] = F[r * L::LDH + j] / (sigma + 1e-7f);
            }
        }
    } else {
        const float *F = gp_bwd::score_vjp_tile<gp_bwd::ENERGY>(lds, net, a.cvec, tvec, row0, a.nrows, a.kcand, pre, sigma);
        for (int e = tid; e < P * POSE; e += TrunkCfg<P>::NT) {
            const int r = e / POSE, j = e - r * POSE;
            if (row0 + r < a.nrows) a.score[(size_t)(row0 + r) * POSE + j] = F[r * gp_bwd::LDS_OUT + j];
        }
    }
}
template <int P, int MODEL = 0>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void heun_step_kernel(HeunArgs a, gp_scorenet net) {
    heun_step_tile<P, SOLVER_HEUN, MODEL>(a, net);
}
template <int P, int MODEL = 0>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void dpm2m_step_kernel(HeunArgs a, gp_scorenet net) {
    heun_step_tile<P, SOLVER_DPM2M, MODEL>(a, net);
}
template <int P>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void heun_step_classes_kernel(HeunClsArgs a, gp_scorenet net) {
    heun_step_tile<P, SOLVER_HEUN, 0>(a, net);
}
template <int P>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void dpm2m_step_classes_kernel(HeunClsArgs a, gp_scorenet net) {
    heun_step_tile<P, SOLVER_DPM2M, 0>(a, net);
}

// The same launch in the chain form (trunk_chain.h).  A wave owns 16 * PT rows from the sampler update to the score: every lane
// of a row's four lane groups carries the row's 9-vector (the update is ~150 VALU instructions per wave, computed redundantly by
// the four groups - cheaper than any exchange), lane group 0 stores.  One partial sum of |score| per WAVE; the batch-mean
// gradient norm is reduced from them by every wave in the same fixed order (identical in all waves: deterministic).
// MODEL 1: the ENERGY network - its score, the gradient of the inner-product energy, from the forward + vector-Jacobian chain of
// trunk_chain_vjp.h (cotangent u = x / sigma; score = f / sigma + J_f^T u, energynet.py:200-222) - what pc_step_kernel<16, 1> computes
// per 16-row tile through LDS.
// SEEDED (pc_step_chain_seeded_kernel): PcRows draws the noise (pc_rows.h).
// HEUN (heun_step_chain_kernel; Args = HeunArgs): a launch of the fixed-step Heun solver (samplers.py:230-290) - PcRows runs the row-local
// update, the score is stored, and there is no partial sum.  SOLVER_DPM2M (dpm2m_step_chain_kernel): the DPM-Solver++(2M) launch, the
// same through PcRows' other update; the time row is the launch's own index.  Both with MODEL 1 too (heun_step_chain_kernel<2, energy>,
// dpm2m_step_chain_kernel<2, energy>): the energy model's score drives the solver.
template <int PT, int MODEL, bool SEEDED, int SOLVER = SOLVER_PC, class Args = PcArgs>
__device__ __forceinline__ void pc_step_chain(const Args &a, const gp_scorenet &net) {
    constexpr bool HEUN = SOLVER != SOLVER_PC;
    static_assert(HEUN == std::is_same<Args, HeunArgs>::value && (!HEUN || !SEEDED), "HeunArgs drive the HEUN instantiations: no noise");
    using C = gp_chain::Cfg<PT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), pt = lane & 15, g = lane >> 4, i = a.step;
    const int wg_row0 = blockIdx.x * C::ROWS;
    gp_chain::State<PT> st;
    const int trow = i < a.nsteps ? i : 0;
    const float *tvec = a.tvec_all + (size_t)(SOLVER == SOLVER_HEUN ? (trow + 1) >> 1 : trow) * HEADS;  // HEUN: one row per evaluated time (HeunArgs)
    // ---- the rows' operands are requested first, the ring prologue behind them: one memory round trip covers both (PcRows, pc_rows.h)
    PcRows<PT, SEEDED, SOLVER> rs;
    rs.template request<gp_chain::NW>(a, wave, lane);
    auto &xv = rs.xv;
    const float sigma = rs.sigma;
    gp_chain::Staged<PT> sg;
    if (i < a.nsteps) gp_chain::begin_request<PT>(st, sg, net, a.cvec, tvec, wg_row0, a.nrows, a.kcand);
    __builtin_amdgcn_sched_barrier(0);
    if (rs.finish_previous(a, lane)) return;
    __builtin_amdgcn_sched_barrier(0);
    gp_chain::begin_deposit<PT>(sg, lds);
    f32x4 xf[PT];
#pragma unroll
    for (int p = 0; p < PT; ++p) xf[p] = gp_chain::pose_fragment(xv[p], g);
    float f[PT][POSE];
    float gx9[PT][POSE];  // MODEL 1: J_f^T u, every lane of a row holds all nine components
    if constexpr (MODEL == 0) {
        gp_chain::run<PT>(st, lds, net, xf, f);
    } else {
        float u[PT][POSE];
        f32x4 gx[PT];
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int j = 0; j < POSE; ++j) u[p][j] = xv[p][j] / sigma;
        gp_chain::store_cotangent<PT>(lds, u);
        gp_chain::run_vjp<PT>(st, lds, net, xf, f, gx);
        // lane (row, g) holds components 4g .. 4g+3: hand every lane of the row all nine
#pragma unroll
        for (int p = 0; p < PT; ++p)
#pragma unroll
            for (int j = 0; j < POSE; ++j) gx9[p][j] = __shfl(gx[p][j & 3], pt + 16 * (j >> 2), 64);
    }
    // (pc_rows.h's pc_store_score / pc_store_partial written out, in their order: through the helpers this kernel allocates one more
    // accumulator register and spills one more)
    float nsum = 0.f;
#pragma unroll
    for (int p = 0; p < PT; ++p) {
        float q = 0.f, sc9[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            sc9[j] = MODEL == 0 ? f[p][j] / (sigma + 1e-7f) : f[p][j] / sigma + gx9[p][j];
            q += sc9[j] * sc9[j];
        }
        if (rs.row[p] < a.nrows && g == 0) {
#pragma unroll
            for (int j = 0; j < 9; ++j) a.score[(size_t)rs.row[p] * 9 + j] = sc9[j];
            nsum += sqrtf(q);
        }
    }
    if constexpr (!HEUN) {
        nsum = wave_sum_f32(nsum);
        if (lane == 0) a.partials[(size_t)i * a.nparts + (size_t)blockIdx.x * gp_chain::NW + wave] = nsum;
    }
}

template <int PT, int MODEL>
__global__ __launch_bounds__(gp_chain::NT, 1) void pc_step_chain_kernel(PcArgs a, gp_scorenet net) {
    pc_step_chain<PT, MODEL, false>(a, net);
}
template <int PT>
__global__ __launch_bounds__(gp_chain::NT, 1) void pc_step_chain_seeded_kernel(PcArgs a, gp_scorenet net) {
    pc_step_chain<PT, 0, true>(a, net);
}
template <int PT, int MODEL = 0>
__global__ __launch_bounds__(gp_chain::NT, 1) void heun_step_chain_kernel(HeunArgs a, gp_scorenet net) {
    pc_step_chain<PT, MODEL, false, SOLVER_HEUN>(a, net);
}
template <int PT, int MODEL = 0>
__global__ __launch_bounds__(gp_chain::NT, 1) void dpm2m_step_chain_kernel(HeunArgs a, gp_scorenet net) {
    pc_step_chain<PT, MODEL, false, SOLVER_DPM2M>(a, net);
}

// The kernels of a host template's arguments.  PC: seeded or not, score model (the energy model has one tile kernel and no seeded one).
template <bool SEEDED, int P, bool SPLIT = false>
constexpr auto pc_tile_kernel = pc_step_kernel<P, 0, SPLIT>;
template <int P, bool SPLIT>
constexpr auto pc_tile_kernel<true, P, SPLIT> = pc_step_seeded_kernel<P, SPLIT>;
// The fixed-step solvers (SOLVER_HEUN / SOLVER_DPM2M): tile and chain form, score (MODEL 0) or energy model (MODEL 1: 16-row tiles and
// the chain form only).
template <int SOLVER, int P, int MODEL = 0>
constexpr auto fixed_step_kernel = heun_step_kernel<P, MODEL>;
template <int P, int MODEL>
constexpr auto fixed_step_kernel<SOLVER_DPM2M, P, MODEL> = dpm2m_step_kernel<P, MODEL>;
template <int SOLVER, int P>
constexpr auto fixed_classes_kernel = heun_step_classes_kernel<P>;
template <int P>
constexpr auto fixed_classes_kernel<SOLVER_DPM2M, P> = dpm2m_step_classes_kernel<P>;
template <int SOLVER, int PT, int MODEL = 0>
constexpr auto fixed_chain_kernel = heun_step_chain_kernel<PT, MODEL>;
template <int PT, int MODEL>
constexpr auto fixed_chain_kernel<SOLVER_DPM2M, PT, MODEL> = dpm2m_step_chain_kernel<PT, MODEL>;

}  // namespace

// rows per partial sum of |score| for a plan
static int pc_rows_per_partial(int P) { return P <= 64 ? P : P / gp_chain::NW; }  // tile form: per workgroup; chain form: per wave
static int pc_rows_per_wg(int P) { return P; }

// What gp_pc_step_plan and gp_pc_step_plan_seeded do behind their own argument checks: the layout, the head-split plan's rule, PcArgs
// and the launch.  z_lang carries the Langevin noise or, SEEDED, the seed state (PcArgs; z_pred is null then, model 0).
template <bool SEEDED>
static int pc_step_launch(int model, int tile, int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                          const float *tvec_all, const float *sched, const float *z_lang, const float *z_pred, const float *centre, float *x, float *mean_x,
                          float *score, float *partials, float *traj, const float *gn_ext, int gn_rows_total, hipStream_t st) {
    const int rg = nclouds_per_group * k, R = ngroups * rg;
    if (R == 0) return GP_OK;
    int P = 0, nparts = 0;
    const int rc = gp_pc_layout(model, tile, ngroups, nclouds_per_group, k, &P, &nparts);
    if (rc != GP_OK) return rc;
    if (model == 1 && (!net->w_headx_t || !net->w_pose2_t || !net->w_pose0_t)) return GP_EINVAL;
    const bool split = P == (16 | GP_PLAN_HEADSPLIT);
    if (split) {
        if (gn_ext) return GP_EINVAL;  // a sharded batch's callers sum whole-tile partials between the launches: tile plans only
        P = 16;
    }
    const int wgpg = (rg + pc_rows_per_wg(P) - 1) / pc_rows_per_wg(P);
    const PcArgs a = pc_args(ngroups, rg, k, step, nsteps, nparts, wgpg, cvec, tvec_all, sched, z_lang, z_pred, centre, x, mean_x, score, partials, traj, gn_ext,
                             gn_rows_total);
    const int nwg = a.wgpg * ngroups;
    const dim3 chain_blk(gp_chain::NT), blk16(TrunkCfg<16>::NT);
    if (P == 128) {
        if constexpr (SEEDED)
            return gp_launch<pc_step_chain_seeded_kernel<2>>(dim3(nwg), chain_blk, gp_chain::Cfg<2>::LDS_BYTES, st, a, *net);
        else if (model == 1)
            return gp_launch<pc_step_chain_kernel<2, 1>>(dim3(nwg), chain_blk, gp_chain::CfgV<2>::LDS_BYTES, st, a, *net);
        else
            return gp_launch<pc_step_chain_kernel<2, 0>>(dim3(nwg), chain_blk, gp_chain::Cfg<2>::LDS_BYTES, st, a, *net);
    }
    if (gp_prepare_lds<pc_tile_kernel<SEEDED, 16>, pc_tile_kernel<SEEDED, 16, true>>(trunk_lds_bytes<16>()) ||
        gp_prepare_lds<pc_tile_kernel<SEEDED, 32>>(trunk_lds_bytes<32>()) || gp_prepare_lds<pc_tile_kernel<SEEDED, 64>>(trunk_lds_bytes<64>()))
        return GP_ELAUNCH;
    if constexpr (!SEEDED) {
        if (gp_prepare_lds<pc_step_kernel<16, 1>>(gp_bwd::LDS_BYTES)) return GP_ELAUNCH;
        if (model == 1) return gp_launch<pc_step_kernel<16, 1>>(dim3(nwg), blk16, gp_bwd::LDS_BYTES, st, a, *net);
    }
    if (split) return gp_launch<pc_tile_kernel<SEEDED, 16, true>>(dim3(3 * nwg), blk16, trunk_lds_bytes<16>(), st, a, *net);
    return gp_with_tile(P, [&](auto tile_rows) {
        constexpr int T = decltype(tile_rows)::value;
        return gp_launch<pc_tile_kernel<SEEDED, T>>(dim3(nwg), dim3(TrunkCfg<T>::NT), trunk_lds_bytes<T>(), st, a, *net);
    });
}

// A launch of a fixed-step solver (gp_heun_step_plan, gp_dpm2m_step_plan and their _model forms; CLASSES: gp_heun_step_classes,
// gp_dpm2m_step_classes - schedule classes (pc_rows.h), the score model's tile plans only).
template <int SOLVER, bool CLASSES = false>
static int fixed_step_plan(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                           const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                           hipStream_t st, int ncls = 1, const int *cls = nullptr) {
    if ((model != 0 && model != 1) || ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || nsteps < 1 || launch < 0 ||
        launch >= fixed_launches<SOLVER>(nsteps, denoise) || !net || !cvec || !tvec_all || !sched || !centre || !x || !d || !score || !out)
        return GP_EINVAL;
    if (CLASSES && (model != 0 || ncls < 1 || ncls > GP_MAX_SCHED_CLASSES || !cls)) return GP_EINVAL;
    const int rg = nclouds_per_group * k, R = ngroups * rg;
    if (R == 0) return GP_OK;
    int P = 0;
    const int rc = gp_heun_layout_model(model, tile, ngroups, nclouds_per_group, k, &P);
    if (rc != GP_OK) return rc;
    if (model == 1 && (!net->w_headx_t || !net->w_pose2_t || !net->w_pose0_t)) return GP_EINVAL;
    const HeunArgs a = heun_args(R, k, launch, fixed_launches<SOLVER>(nsteps, denoise) - 1, cvec, tvec_all, sched, centre, x, d, score, out, traj);
    const int nwg = ngroups * ((rg + P - 1) / P);
    if constexpr (CLASSES) {  // (GP_EINVAL for plan 128: the chain form keeps its one time per launch)
        const HeunClsArgs ac = heun_cls_args(a, ncls, cls, nsteps + 1);
        return gp_with_tile(P, [&](auto tile_rows) {
            constexpr int T = decltype(tile_rows)::value;
            return gp_launch<fixed_classes_kernel<SOLVER, T>>(dim3(nwg), dim3(TrunkCfg<T>::NT), trunk_lds_bytes<T>(), st, ac, *net);
        });
    }
    if (model == 1) {  // the energy model: the forward + vector-Jacobian kernels, with their LDS (gp_heun_layout_model: 16 or 128)
        if (P == 128) return gp_launch<fixed_chain_kernel<SOLVER, 2, 1>>(dim3(nwg), dim3(gp_chain::NT), gp_chain::CfgV<2>::LDS_BYTES, st, a, *net);
        return gp_launch<fixed_step_kernel<SOLVER, 16, 1>>(dim3(nwg), dim3(TrunkCfg<16>::NT), gp_bwd::LDS_BYTES, st, a, *net);
    }
    if (P == 128) return gp_launch<fixed_chain_kernel<SOLVER, 2>>(dim3(nwg), dim3(gp_chain::NT), gp_chain::Cfg<2>::LDS_BYTES, st, a, *net);
    if (gp_prepare_lds<fixed_step_kernel<SOLVER, 16>>(trunk_lds_bytes<16>()) || gp_prepare_lds<fixed_step_kernel<SOLVER, 32>>(trunk_lds_bytes<32>()) ||
        gp_prepare_lds<fixed_step_kernel<SOLVER, 64>>(trunk_lds_bytes<64>()))
        return GP_ELAUNCH;
    return gp_with_tile(P, [&](auto tile_rows) {
        constexpr int T = decltype(tile_rows)::value;
        return gp_launch<fixed_step_kernel<SOLVER, T>>(dim3(nwg), dim3(TrunkCfg<T>::NT), trunk_lds_bytes<T>(), st, a, *net);
    });
}

extern "C" {

int gp_score_tile_rows(int nrows) { return score_tile_rows(nrows); }

int gp_cloud_embed(int b, const gp_scorenet *net, const float *pts_feat, float *cvec, gp_stream_t s) {
    if (b < 0 || !net || !pts_feat || !cvec) return GP_EINVAL;
    if (b == 0) return GP_OK;
    const size_t lds = (size_t)16 * (1024 + GP_LD_PAD) * sizeof(float);
    return gp_launch<cloud_embed_kernel>(dim3((b + 15) / 16, 3), dim3(256), lds, (hipStream_t)s, b, *net, pts_feat, cvec);
}

int gp_time_embed(int nt, const gp_scorenet *net, const float *t, float *tvec, gp_stream_t s) {
    if (nt < 0 || !net || !t || !tvec) return GP_EINVAL;
    if (nt == 0) return GP_OK;
    hipLaunchKernelGGL(time_embed_kernel, dim3(nt), dim3(256), 0, (hipStream_t)s, *net, t, (size_t)0, tvec);
    return gp_launch_status();
}

int gp_time_embed_strided(int nt, int ngroups, int64_t t_stride_floats, const gp_scorenet *net, const float *t, float *tvec, gp_stream_t s) {
    if (nt < 0 || ngroups < 0 || t_stride_floats < 0 || !net || !t || !tvec) return GP_EINVAL;
    if (nt == 0 || ngroups == 0) return GP_OK;
    hipLaunchKernelGGL(time_embed_kernel, dim3(nt, ngroups), dim3(256), 0, (hipStream_t)s, *net, t, (size_t)t_stride_floats, tvec);
    return gp_launch_status();
}

int gp_score_eval_plan(int tile, int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x,
                       const float *sigma_dev, int mode, float *out, gp_stream_t s) {
    if (nclouds < 0 || k <= 0 || !net || !cvec || !tvec || !x || !sigma_dev || !out || (mode != 0 && mode != 1)) return GP_EINVAL;
    const int R = nclouds * k;
    if (R == 0) return GP_OK;
    const int P = tile == 0 ? score_plan_rows(R, 0, k) : tile;
    hipStream_t st = (hipStream_t)s;
    if (P == 128) {
        using C = gp_chain::Cfg<2>;
        if (!C::fits(k)) return GP_EINVAL;
        return gp_launch<score_eval_chain_kernel<2>>(dim3((R + C::ROWS - 1) / C::ROWS), dim3(gp_chain::NT), C::LDS_BYTES, st, R, k, *net, cvec, tvec, x,
                                                     sigma_dev, mode, out);
    }
    if (P != 16 && P != 32 && P != 64) return GP_EINVAL;
    if (gp_prepare_lds<score_eval_kernel<16>>(trunk_lds_bytes<16>()) || gp_prepare_lds<score_eval_kernel<32>>(trunk_lds_bytes<32>()) ||
        gp_prepare_lds<score_eval_kernel<64>>(trunk_lds_bytes<64>()))
        return GP_ELAUNCH;
    return gp_with_tile(P, [&](auto tile) {
        constexpr int T = decltype(tile)::value;
        return gp_launch<score_eval_kernel<T>>(dim3((R + T - 1) / T), dim3(TrunkCfg<T>::NT), trunk_lds_bytes<T>(), st, R, k, *net, cvec, tvec, x, sigma_dev,
                                               mode, out);
    });
}

int gp_score_eval(int nclouds, int k, const gp_scorenet *net, const float *cvec, const float *tvec, const float *x, const float *sigma_dev, int mode,
                  float *out, gp_stream_t s) {
    return gp_score_eval_plan(0, nclouds, k, net, cvec, tvec, x, sigma_dev, mode, out, s);
}

int gp_pc_tile_rows(int ngroups, int nclouds_per_group, int k) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0) return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    int P = score_tile_rows(ngroups * rg);
    if (ngroups > 1 && rg % P != 0) P = 16;  // tiles must not straddle groups
    if (ngroups > 1 && rg % P != 0) return GP_EINVAL;
    return P;
}

int gp_pc_layout(int model, int tile, int ngroups, int nclouds_per_group, int k, int *tile_out, int *nparts_out) {
    if ((model != 0 && model != 1) || ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || !tile_out || !nparts_out) return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    int P = tile;
    if (model == 1) {  // the energy model's score needs the backward pass: 16-row tiles (score_bwd.h) or the 128-row chain form (trunk_chain_vjp.h)
        if (P == 0) P = score_plan_rows_vjp(ngroups * rg, ngroups > 1 ? rg : 0, k);
        if (P != 16 && P != 128) return GP_EINVAL;
    }
    if (P == 0) P = score_plan_latency(ngroups * rg, ngroups > 1 ? rg : 0, k);
    if (P == (16 | GP_PLAN_HEADSPLIT)) {  // three workgroups per 16-row tile, one head each: one partial per row and head (PcArgs)
        if (model != 0 || (ngroups > 1 && rg % 16 != 0)) return GP_EINVAL;
        *tile_out = P;
        *nparts_out = 21 * ngroups * rg;  // per step: row-and-head sums of squares [3R], score [9R], state [9R] (PcArgs)
        return GP_OK;
    }
    if (P != 16 && P != 32 && P != 64 && P != 128) return GP_EINVAL;
    if (P == 128 && !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    if (ngroups > 1 && rg % pc_rows_per_wg(P) != 0) return GP_EINVAL;  // a workgroup must not straddle two batches
    const int rpp = pc_rows_per_partial(P);
    *tile_out = P;
    *nparts_out = ngroups * ((rg + pc_rows_per_wg(P) - 1) / pc_rows_per_wg(P)) * (pc_rows_per_wg(P) / rpp);
    return GP_OK;
}

int gp_pc_step_plan(int model, int tile, int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                    const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x,
                    float *mean_x, float *score, float *partials, float *traj, const float *gn_ext, int gn_rows_total, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || step < 0 || step > nsteps || !net || !cvec || !tvec_all || !sched || !z_langevin ||
        !z_predictor || !centre || !x || !mean_x || !score || !partials || gn_rows_total < 0)
        return GP_EINVAL;
    return pc_step_launch<false>(model, tile, ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x, mean_x,
                                score, partials, traj, gn_ext, gn_rows_total, (hipStream_t)s);
}

int gp_pc_step_plan_seeded(int tile, int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                           const float *tvec_all, const float *sched, const void *seed_state, const float *centre, float *x, float *mean_x, float *score,
                           float *partials, float *traj, const float *gn_ext, int gn_rows_total, gp_stream_t s) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || step < 0 || step > nsteps || (uint32_t)nsteps >= gp_philox::MAX_STEPS || !net || !cvec ||
        !tvec_all || !sched || !seed_state || !centre || !x || !mean_x || !score || !partials || gn_rows_total < 0)
        return GP_EINVAL;
    // (the seed state travels in the argument block's z_lang slot: PcArgs)
    return pc_step_launch<true>(0, tile, ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, reinterpret_cast<const float *>(seed_state),
                               nullptr, centre, x, mean_x, score, partials, traj, gn_ext, gn_rows_total, (hipStream_t)s);
}

int gp_heun_launches(int nsteps, int denoise) { return nsteps < 1 ? GP_EINVAL : 2 * nsteps + 1 + (denoise ? 1 : 0); }

int gp_heun_layout(int tile, int ngroups, int nclouds_per_group, int k, int *tile_out) {
    if (ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || !tile_out) return GP_EINVAL;
    const int rg = nclouds_per_group * k;
    int P = tile;
    if (P == 0) {  // the PC planner's row thresholds; where it would split the heads (the latency regime) the Heun solver keeps whole 16-row tiles
        P = score_plan_latency(ngroups * rg, ngroups > 1 ? rg : 0, k);
        if (P == (16 | GP_PLAN_HEADSPLIT)) P = 16;
    }
    if (P != 16 && P != 32 && P != 64 && P != 128) return GP_EINVAL;  // (head-split included: there is no Heun kernel for it)
    if (P == 128 && !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    if (ngroups > 1 && rg % P != 0) return GP_EINVAL;  // a workgroup must not straddle two batches
    *tile_out = P;
    return GP_OK;
}

int gp_heun_layout_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int *tile_out) {
    if (model == 0) return gp_heun_layout(tile, ngroups, nclouds_per_group, k, tile_out);
    if (model != 1 || ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || !tile_out) return GP_EINVAL;
    // the energy model's score needs the backward pass: 16-row tiles (score_bwd.h) or the 128-row chain form (trunk_chain_vjp.h), as gp_pc_layout
    const int rg = nclouds_per_group * k;
    int P = tile;
    if (P == 0) P = score_plan_rows_vjp(ngroups * rg, ngroups > 1 ? rg : 0, k);
    if (P != 16 && P != 128) return GP_EINVAL;  // (32 / 64-row tiles and head-split included: the backward pass has none)
    if (P == 128 && !gp_chain::Cfg<2>::fits(k)) return GP_EINVAL;
    if (ngroups > 1 && rg % P != 0) return GP_EINVAL;  // a workgroup must not straddle two batches
    *tile_out = P;
    return GP_OK;
}

int gp_heun_step_plan(int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                      const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                      gp_stream_t s) {
    return fixed_step_plan<SOLVER_HEUN>(0, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out,
                                        traj, (hipStream_t)s);
}

int gp_heun_step_plan_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                            const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                            float *traj, gp_stream_t s) {
    return fixed_step_plan<SOLVER_HEUN>(model, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score,
                                        out, traj, (hipStream_t)s);
}

int gp_heun_step_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                         const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                         float *traj, int ncls, const int *cls, gp_stream_t s) {
    return fixed_step_plan<SOLVER_HEUN, true>(model, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d,
                                              score, out, traj, (hipStream_t)s, ncls, cls);
}

int gp_dpm2m_step_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                          const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                          float *traj, int ncls, const int *cls, gp_stream_t s) {
    return fixed_step_plan<SOLVER_DPM2M, true>(model, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d,
                                               score, out, traj, (hipStream_t)s, ncls, cls);
}

int gp_dpm2m_launches(int nsteps, int denoise) { return nsteps < 1 ? GP_EINVAL : nsteps + 1 + (denoise ? 1 : 0); }

int gp_dpm2m_step_plan(int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                       gp_stream_t s) {
    return fixed_step_plan<SOLVER_DPM2M>(0, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out,
                                         traj, (hipStream_t)s);
}

int gp_dpm2m_step_plan_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int launch, int nsteps, int denoise, const gp_scorenet *net,
                             const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out,
                             float *traj, gp_stream_t s) {
    return fixed_step_plan<SOLVER_DPM2M>(model, tile, ngroups, nclouds_per_group, k, launch, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score,
                                         out, traj, (hipStream_t)s);
}

int gp_pc_step_coupled(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor, const float *centre,
                       float *x, float *mean_x, float *score, float *partials, float *traj, const float *gn_ext, gp_stream_t s) {
    // the entry points that predate gp_pc_layout stay in the TILE form: `partials` keeps the size their contract states,
    // nsteps x ngroups x ceil(rows per group / gp_pc_tile_rows) - the chain form writes one partial per wave and is reached through
    // gp_pc_layout + gp_pc_step_plan only
    const int legacy_tile = gp_pc_tile_rows(ngroups, nclouds_per_group, k);
    if (legacy_tile < 0) return legacy_tile;
    return gp_pc_step_plan(0, legacy_tile, ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x, mean_x, score,
                           partials, traj, gn_ext, 0, s);
}

int gp_pc_step_grouped(int ngroups, int nclouds_per_group, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec,
                       const float *tvec_all, const float *sched, const float *z_langevin, const float *z_predictor, const float *centre,
                       float *x, float *mean_x, float *score, float *partials, float *traj, gp_stream_t s) {
    const int legacy_tile = gp_pc_tile_rows(ngroups, nclouds_per_group, k);
    if (legacy_tile < 0) return legacy_tile;
    return gp_pc_step_plan(0, legacy_tile, ngroups, nclouds_per_group, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x, mean_x,
                           score, partials, traj, nullptr, 0, s);
}

int gp_pc_step(int nclouds, int k, int step, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
               const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x,
               float *score, float *partials, float *traj, gp_stream_t s) {
    if (nclouds < 0 || k <= 0) return GP_EINVAL;
    return gp_pc_step_plan(0, score_tile_rows(nclouds * k), 1, nclouds, k, step, nsteps, net, cvec, tvec_all, sched, z_langevin, z_predictor, centre, x, mean_x,
                           score, partials, traj, nullptr, 0, s);
}

}  // extern "C"
