// The seeded PC sampler's noise as plain buffers (include/genpose_hip.h: gp_pc_noise_fill, gp_philox_raw): what the seeded step kernels
// draw in registers (philox.h: the same device function), written out - the bridge to the injected-noise path of gp_pc_step_plan /
// gp_pc_step_bf16x9 and a dump of a run's draws.  Replaces torch.randn_like of cond_pc_sampler (samplers.py:132,149).
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

int gp_philox_raw(int64_t n, const void *counters, const void *keys, void *out, gp_stream_t s) {
    if (n < 0 || !counters || !keys || !out) return GP_EINVAL;
    if (n == 0) return GP_OK;
    if ((n + 255) / 256 > 0x7fffffffLL) return GP_EINVAL;
    hipLaunchKernelGGL(philox_raw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, (long long)n, (const uint32_t *)counters,
                       (const uint32_t *)keys, (uint32_t *)out);
    return gp_launch_status();
}

}  // extern "C"
