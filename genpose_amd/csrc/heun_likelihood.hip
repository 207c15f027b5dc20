// Fixed-step Heun solve of the exact-divergence likelihood ODE (cond_ode_likelihood, networks/gf_algorithms/samplers.py:22-99): the
// ten-component system [x; logp] integrated in sigma from sigma(eps) up to sigma(T) - -g^2/2 dt = -sigma dsigma, so the slope is
//     d = -sigma [score(x, t); div_x score(x, t)]
// with score and the EXACT divergence from score_div_exact_tile (score_bwd.h, called unchanged: gp_score_div_exact's bits).  The launch
// structure is the Heun sampler's (scorenet.hip: heun_step_tile): a launch applies the row update that the previous evaluation completes
// and evaluates at the next point, which it hands to the trunk through LDS.  x and the slopes are fp32 (heun_update_row, score_trunk.h:
// the sampler's arithmetic, written once); the log-density change is accumulated in float64.  Row-local: no noise, no batch statistic, no
// atomic, no wait on another workgroup - the result of a row is a function of (cloud, row, schedule) alone.
//
//   launch 0        evaluates (x_0, t_0)
//   launch 2i + 1   d_i = c [score; div] -> d [R,10];  evaluates (x_i + h d_i[x], t_{i+1})                     (HEUN_PREDICT)
//   launch 2i + 2   x, l += h (0.5 d_i + 0.5 c [score; div]) -> x, logp;  evaluates (x_{i+1}, t_{i+1})         (HEUN_CORRECT)
//   launch 2N       the same update -> z_out, logp; evaluates nothing                                          (HEUN_CORRECT_LAST)
// l_0 = 0 is part of the chain: launch 2 does not read logp.  LDS: score_div_exact_tile's own block (LDS_BYTES_EXACT = 127 872 bytes, one
// workgroup per CU); the row update lives in the registers of the first DP threads and needs no row of its own.
#include "score_bwd.h"

namespace {

using namespace gp_bwd;

constexpr int LD_D = 10;  // d [R][10]: the nine pose slopes and the log-density slope of the stored predictor stage

struct HeunLikArgs {
    int nrows, kcand, launch, last;  // last = 2 nsteps: the launch that finishes and evaluates nothing
    const float *cvec, *tvec_all;    // tvec_all [nsteps + 1][768]: launch l evaluates at row (l + 1) / 2
    const float *sched;              // [launches][4]: sigma of the launch's evaluation, slope factor c, step h, kind (HEUN_*)
    float *x, *d, *score, *div;
    double *logp;
    float *z_out;
};

__global__ __launch_bounds__(DNT) void heun_likelihood_step_kernel(HeunLikArgs a, gp_scorenet net) {
    using L = TrunkLds<DP, true>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int row0 = blockIdx.x * DP, tid = threadIdx.x, i = a.launch;
    const float *tvec = a.tvec_all + (size_t)((i + 1) >> 1) * HEADS;
    TrunkPre<DP> pre;
    float sigma = 1.f;
    if (i < a.last) {
        trunk_begin<DP>(net, pre, a.cvec, tvec, row0, a.nrows, a.kcand);
        sigma = a.sched[(size_t)i * 4 + 0];  // requested now, used after the trunk
        gp_pin(sigma);
    }
    if (i > 0) {
        if (tid < DP) {
            const bool live = row0 + tid < a.nrows;
            const int r = live ? row0 + tid : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
            const float *sc = a.sched + (size_t)i * 4;
            const int kind = (int)sc[3];
            const float c = sc[1], h = sc[2];
            const bool correct = kind == HEUN_CORRECT || kind == HEUN_CORRECT_LAST;
            float xv[9], gr[9], dv[9];
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                xv[j] = a.x[(size_t)r * 9 + j];
                gr[j] = a.score[(size_t)r * 9 + j];
                dv[j] = correct ? a.d[(size_t)r * LD_D + j] : 0.f;
            }
            const float gd = a.div[r];
            heun_update_row(kind, xv, dv, gr, c, h);
            if (kind == HEUN_PREDICT) {
                const float dl = c * gd;
                if (live) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) a.d[(size_t)r * LD_D + j] = dv[j];
                    a.d[(size_t)r * LD_D + 9] = dl;
                }
            } else if (correct) {
                // the log-density component of the same update: slopes in fp32, the running sum in float64 (l_0 = 0: launch 2 starts it)
                const float dl = a.d[(size_t)r * LD_D + 9], dlp = c * gd;
                const double l0 = i == 2 ? 0.0 : a.logp[r];
                const double l1 = l0 + (double)h * (double)(0.5f * dl + 0.5f * dlp);
                if (live) {
                    a.logp[r] = l1;
                    float *xo = (kind == HEUN_CORRECT_LAST ? a.z_out : a.x) + (size_t)r * 9;
#pragma unroll
                    for (int j = 0; j < 9; ++j) xo[j] = xv[j];
                }
            }
            // hand the evaluation point to the trunk through LDS (no global round trip)
            float *xr = lds + tid * L::LD0;
#pragma unroll
            for (int j = 0; j < 9; ++j) xr[j] = xv[j];
#pragma unroll
            for (int j = 9; j < 16; ++j) xr[j] = 0.f;
        }
        if (i == a.last) return;
    } else {
        load_x_tile<DP>(lds, a.x, row0, a.nrows);
    }
    __syncthreads();
    const float *out = score_div_exact_tile(lds, net, a.cvec, tvec, row0, a.nrows, a.kcand, pre, sigma);
    for (int e = tid; e < DP * POSE; e += DNT) {
        const int r = e / POSE, j = e - r * POSE;
        if (row0 + r < a.nrows) a.score[(size_t)(row0 + r) * POSE + j] = out[r * LDS_OUT + j];
    }
    if (tid < DP && row0 + tid < a.nrows) a.div[row0 + tid] = out[tid * LDS_OUT + 9];
}

}  // namespace

extern "C" int gp_heun_likelihood_launches(int nsteps) { return nsteps < 1 ? GP_EINVAL : 2 * nsteps + 1; }

extern "C" int gp_heun_likelihood_step(int nclouds, int k, int launch, int nsteps, const gp_scorenet *net, const float *cvec, const float *tvec_all,
                                       const float *sched, float *x, float *d, float *score, float *div, double *logp, float *z_out, gp_stream_t s) {
    if (nclouds < 0 || k <= 0 || nsteps < 1 || launch < 0 || launch >= gp_heun_likelihood_launches(nsteps) || !net || !cvec || !tvec_all || !sched || !x ||
        !d || !score || !div || !logp || !z_out)
        return GP_EINVAL;
    if (!net->w_headx_t || !net->w_pose2_t || !net->w_pose0_t) return GP_EINVAL;
    const long long R = (long long)nclouds * k;
    if (R == 0) return GP_OK;
    if (R > 0x7fffffffLL / LD_D) return GP_EINVAL;  // row and element indices are ints up to R * 10
    HeunLikArgs a;
    a.nrows = (int)R, a.kcand = k, a.launch = launch, a.last = 2 * nsteps;
    a.cvec = cvec, a.tvec_all = tvec_all, a.sched = sched;
    a.x = x, a.d = d, a.score = score, a.div = div, a.logp = logp, a.z_out = z_out;
    return gp_launch<heun_likelihood_step_kernel>(dim3((unsigned)((R + DP - 1) / DP)), dim3(DNT), LDS_BYTES_EXACT, (hipStream_t)s, a, *net);
}
