// The seeded PC sampler's noise as plain buffers (include/genpose_hip.h: gp_pc_noise_fill, gp_philox_raw): what the seeded step kernels
// draw in registers (philox.h: the same device function), written out - the bridge to the injected-noise path of gp_pc_step_plan /
// gp_pc_step_bf16x9 and a dump of a run's draws.  Replaces torch.randn_like of cond_pc_sampler (samplers.py:132,149).
// And the fixed-step tracker's prior (gp_track_warm_start, gp_track_prior_fill): the draw of samplers.py:180 on the prior's own counters
// (philox.h) with the warm start of evaluation_tracking.py:302-310 around it.
#include "gp_common.h"
#include "philox.h"

namespace {

// one thread per (step, row): z_lang / z_pred [nsteps][nrows][9]; the row of the launch is row0 + r
__global__ __launch_bounds__(256) void pc_noise_fill_kernel(const uint32_t *__restrict__ seed_state, int step0, int nsteps, long long row0, long long nrows,
                                                            float *__restrict__ z_lang, float *__restrict__ z_pred) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)nsteps * nrows) return;
    const long long s = e / nrows, r = e - s * nrows;
    const gp_philox::Seed sd = gp_philox::load_seed(seed_state);
    const uint64_t grow = sd.row_base + (uint64_t)(row0 + r);
    float z[9];
    if (z_lang) {
        gp_philox::draw9(sd, (uint32_t)(step0 + s), gp_philox::STREAM_LANGEVIN, grow, z);
#pragma unroll
        for (int j = 0; j < 9; ++j) z_lang[e * 9 + j] = z[j];
    }
    if (z_pred) {
        gp_philox::draw9(sd, (uint32_t)(step0 + s), gp_philox::STREAM_PREDICTOR, grow, z);
#pragma unroll
        for (int j = 0; j < 9; ++j) z_pred[e * 9 + j] = z[j];
    }
}

// The tracker's warm start, one thread per row (cloud i, candidate c): x0 = init_i + sigma * z, the product and the sum rounded separately (a
// host restatement in fp32 gives the same bits).  init_i = [R[:,0], R[:,1], t - centre[i]] of a row-major 4x4: the previous frame's
// aggregated pose src[i] when src[i] >= 0, else the cloud's own fallback (the jittered ground truth).
// CLASSES (track_start_classes_kernel, gp_track_start_classes): `sigma` is the solve's schedule block, class c's sigma(T0_c) at
// sigma[c * class_stride].  A cloud without a predecessor is ACQUIRED when `acquire` is set: x0 = sigma_1 * z, the pure prior (samplers.py:180
// with init_x = None) on the same draw, and no pose is read for it.  The first row of every cloud writes the cloud's class for the solve.
template <bool CLASSES>
__device__ __forceinline__ void track_start_row(int n, int k, const uint32_t *__restrict__ seed_state, const float *__restrict__ sigma, int class_stride,
                                                const float *__restrict__ prev_sRT, const int *__restrict__ src, const float *__restrict__ fallback_sRT,
                                                const float *__restrict__ centre, float *__restrict__ x0, int *__restrict__ cls_out, int acquire) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int i = (int)(e / k);
    const int sp = src[i];
    auto draw = [&](float (&z)[9]) {  // the prior's draw of this row
        const gp_philox::Seed sd = gp_philox::load_seed(seed_state);
        gp_philox::draw9(sd, gp_philox::PRIOR_STEP, gp_philox::STREAM_LANGEVIN, sd.row_base + (uint64_t)e, z);
    };
    if constexpr (CLASSES) {
        const bool prior = acquire && sp < 0;
        if (e == (long long)i * k) cls_out[i] = prior ? 1 : 0;
        if (prior) {
            float z[9];
            draw(z);
            const float s1 = sigma[class_stride];
#pragma unroll
            for (int j = 0; j < 9; ++j) x0[e * 9 + j] = __fmul_rn(s1, z[j]);
            return;
        }
    }
    const float *m = sp >= 0 ? prev_sRT + (size_t)sp * 16 : fallback_sRT + (size_t)i * 16;
    const float *cp = centre + (size_t)i * 3;
    const float init[9] = {m[0], m[4], m[8], m[1], m[5], m[9], m[3] - cp[0], m[7] - cp[1], m[11] - cp[2]};
    float z[9];
    draw(z);
    const float sg = *sigma;
#pragma unroll
    for (int j = 0; j < 9; ++j) x0[e * 9 + j] = __fadd_rn(init[j], __fmul_rn(sg, z[j]));
}
__global__ __launch_bounds__(256) void track_warm_start_kernel(int n, int k, const uint32_t *__restrict__ seed_state, const float *__restrict__ sigma,
                                                               const float *__restrict__ prev_sRT, const int *__restrict__ src,
                                                               const float *__restrict__ fallback_sRT, const float *__restrict__ centre,
                                                               float *__restrict__ x0) {
    track_start_row<false>(n, k, seed_state, sigma, 0, prev_sRT, src, fallback_sRT, centre, x0, nullptr, 0);
}
__global__ __launch_bounds__(256) void track_start_classes_kernel(int n, int k, const uint32_t *__restrict__ seed_state, const float *__restrict__ sched,
                                                                  int class_stride, const float *__restrict__ prev_sRT, const int *__restrict__ src,
                                                                  const float *__restrict__ fallback_sRT, const float *__restrict__ centre,
                                                                  float *__restrict__ x0, int *__restrict__ cls_out, int acquire) {
    track_start_row<true>(n, k, seed_state, sched, class_stride, prev_sRT, src, fallback_sRT, centre, x0, cls_out, acquire);
}

// the prior's draws as a buffer: z_out [nrows][9], the row of the launch is row0 + r
__global__ __launch_bounds__(256) void track_prior_fill_kernel(const uint32_t *__restrict__ seed_state, long long row0, long long nrows, float *__restrict__ z_out) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r >= nrows) return;
    const gp_philox::Seed sd = gp_philox::load_seed(seed_state);
    float z[9];
    gp_philox::draw9(sd, gp_philox::PRIOR_STEP, gp_philox::STREAM_LANGEVIN, sd.row_base + (uint64_t)(row0 + r), z);
#pragma unroll
    for (int j = 0; j < 9; ++j) z_out[r * 9 + j] = z[j];
}

// raw Philox4x32-10 blocks: counters [n][4], keys [n][2] -> out [n][4]
__global__ __launch_bounds__(256) void philox_raw_kernel(long long n, const uint32_t *__restrict__ ctr, const uint32_t *__restrict__ key,
                                                         uint32_t *__restrict__ out) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    uint32_t c[4] = {ctr[4 * e], ctr[4 * e + 1], ctr[4 * e + 2], ctr[4 * e + 3]};
    gp_philox::philox4x32_10(c, key[2 * e], key[2 * e + 1]);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[4 * e + j] = c[j];
}

}  // namespace

extern "C" {

int gp_pc_noise_fill(const void *seed_state, int step0, int nsteps, int64_t row0, int64_t nrows, float *z_lang_out, float *z_pred_out, gp_stream_t s) {
    if (!seed_state || step0 < 0 || nsteps < 0 || row0 < 0 || nrows < 0 || (!z_lang_out && !z_pred_out) ||
        (uint64_t)step0 + (uint64_t)nsteps > gp_philox::MAX_STEPS)
        return GP_EINVAL;
    const long long n = (long long)nsteps * nrows;
    if (n == 0) return GP_OK;
    if ((n + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(pc_noise_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, (const uint32_t *)seed_state, step0, nsteps,
                       (long long)row0, (long long)nrows, z_lang_out, z_pred_out);
    return gp_launch_status();
}

int gp_track_warm_start(int n, int k, const void *seed_state, const float *sigma, const float *prev_sRT, const int *src, const float *fallback_sRT,
                        const float *centre, float *x0, gp_stream_t s) {
    if (n < 0 || k <= 0 || !seed_state || !sigma || !prev_sRT || !src || !fallback_sRT || !centre || !x0) return GP_EINVAL;
    const long long rows = (long long)n * k;
    if (rows == 0) return GP_OK;
    if ((rows + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(track_warm_start_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)s, n, k, (const uint32_t *)seed_state, sigma,
                       prev_sRT, src, fallback_sRT, centre, x0);
    return gp_launch_status();
}

int gp_track_start_classes(int n, int k, const void *seed_state, const float *sched, int class_stride, const float *prev_sRT, const int *src,
                           const float *fallback_sRT, const float *centre, float *x0, int *cls_out, int acquire, gp_stream_t s) {
    if (n < 0 || k <= 0 || class_stride < 1 || !seed_state || !sched || !prev_sRT || !src || (!fallback_sRT && !acquire) || !centre || !x0 || !cls_out)
        return GP_EINVAL;
    const long long rows = (long long)n * k;
    if (rows == 0) return GP_OK;
    if ((rows + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(track_start_classes_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)s, n, k, (const uint32_t *)seed_state, sched,
                       class_stride, prev_sRT, src, fallback_sRT, centre, x0, cls_out, acquire);
    return gp_launch_status();
}

int gp_track_prior_fill(const void *seed_state, int64_t row0, int64_t nrows, float *z_out, gp_stream_t s) {
    if (!seed_state || row0 < 0 || nrows < 0 || !z_out) return GP_EINVAL;
    if (nrows == 0) return GP_OK;
    if ((nrows + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(track_prior_fill_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, (hipStream_t)s, (const uint32_t *)seed_state,
                       (long long)row0, (long long)nrows, z_out);
    return gp_launch_status();
}

int gp_philox_raw(int64_t n, const void *counters, const void *keys, void *out, gp_stream_t s) {
    if (n < 0 || !counters || !keys || !out) return GP_EINVAL;
    if (n == 0) return GP_OK;
    if ((n + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(philox_raw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, (long long)n, (const uint32_t *)counters,
                       (const uint32_t *)keys, (uint32_t *)out);
    return gp_launch_status();
}

}  // extern "C"
