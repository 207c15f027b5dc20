// The whole fixed-step Heun solve of the probability-flow ODE (cond_edm_sampler's method, samplers.py:230-290; HeunArgs, pc_rows.h) in ONE
// launch, tile plans.  The update is row-local, so between two evaluations a workgroup's tile depends on no other workgroup: the
// workgroup that owns rows [blockIdx.x * P, +P) takes them through every launch index l = 0 .. last of the per-launch chain
// (scorenet.hip: heun_step_tile) itself.  Per index it runs that launch's code - heun_update_row, heun_store_row's effects on x, out and
// traj, the hand-over of the evaluation point through LDS, trunk_begin / trunk_ftheta, the score divided by sigma + 1e-7f - on the same
// operands in the same order, so the result is the chain's bit for bit (tests/test_gpu_heun_solve.py).  What the chain passes from launch
// to launch through global memory stays on chip: x_i, d_i and the cloud centre in a private LDS slot of the row's thread (tid < P) behind
// the trunk's block (21 floats per row, component-major: kept in registers they stay live across the whole trunk and the 64-row tile
// spills), the score in the trunk's block itself, where the row thread divides it.  No global store of this kernel is read back by it, so nothing here needs an ordering
// beyond the workgroup barriers below.  d and score are not written.
// SOLVER_DPM2M (dpm2m_solve_kernel, gp_dpm2m_solve_tile): the same loop over the launch indices of the DPM-Solver++(2M) chain (pc_rows.h;
// dpm2m_step_kernel) - its schedule rows, dpm2m_update_row, the time row of the index itself; the slot of d_i holds D_{i-1}.
// MODEL 1 (heun_solve_kernel<16, energy>, dpm2m_solve_kernel<16, energy>; gp_*_solve_tile_model): the ENERGY network's score drives the
// solve (energynet.py:200-222) - score_vjp_tile<ENERGY> (score_bwd.h) in trunk_ftheta's place, as heun_step_tile<16, SOLVER, 1> has it.  The
// row thread's slot sits behind the backward pass's block (gp_bwd::LDS_FLOATS); the previous score is read from the pass's output rows
// (gp_bwd::OFF_U, stride LDS_OUT: behind the trunk's block and G3, so apart from X0) as it is - the chain stores these words undivided -
// before the row thread writes its X0 row, and the barrier below orders that read before score_vjp_tile's seed loop rewrites the block.
// Measured (profiles/fixed_step_energy.txt): the chain's bits, and 0.92 - 0.94x the chain's speed - for this model the chain is the faster form.
#include "pc_rows.h"
#include "score_bwd.h"

namespace {

using namespace gp_trunk;

// A pointer the compiler knows nothing about from here on.  Every index re-requests the trunk's weights, biases and epilogue operands as its
// launch of the chain does; without this the loads that do not depend on the index are hoisted out of the loop and stay live across the
// whole trunk (256 VGPRs and up to 118 spilled registers per lane, against the per-launch kernels' 128 - 184 and none).
__device__ __forceinline__ void opaque(const float *&p) { asm volatile("" : "+s"(p)); }

// Args = HeunClsArgs (heun_solve_classes_kernel, dpm2m_solve_classes_kernel; gp_*_solve_classes): SCHEDULE CLASSES (pc_rows.h), as
// heun_step_tile has them - the row thread's schedule rows (sigma_prev among them) are its cloud's class's, the trunk adds the class's time
// embedding per cloud, the kind and DPM2M's first-step flag come from class 0.
template <int P, int SOLVER, int MODEL = 0, class Args = HeunArgs>
__device__ __forceinline__ void heun_solve(Args a, const gp_scorenet &net0) {
    static_assert(MODEL == 0 || P == gp_bwd::DP, "the backward pass runs on 16-row tiles");
    static_assert(MODEL == 0 || std::is_same<Args, HeunArgs>::value, "schedule classes: the score model");
    using L = TrunkLds<P, MODEL == 1>;
    constexpr int SROW = fixed_sched_row<SOLVER>();
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int row0 = blockIdx.x * P, tid = threadIdx.x, last = a.nsteps;
    const bool live = row0 + tid < a.nrows;
    const int r = live ? row0 + tid : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
    const int rcls = heun_row_class(a, r);           // the row's schedule class (0 without classes)
    float *mine = lds + (MODEL == 1 ? gp_bwd::LDS_FLOATS : L::TOTAL) + tid;  // this row thread's slot: x_i at [j * P], d_i at [(9 + j) * P], the cloud centre at [(18 + j) * P]
    if (tid < P) {
#pragma unroll
        for (int j = 0; j < 9; ++j) mine[j * P] = a.x[(size_t)r * 9 + j];
        const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
#pragma unroll
        for (int j = 0; j < 3; ++j) mine[(18 + j) * P] = cp[j];
    }
    float sigma_prev = 1.f;  // the divisor of the score that sits in LDS
    for (int l = 0; l <= last; ++l) {
        const float *tvec = a.tvec_all + (size_t)pc_time_row<SOLVER>(l) * HEADS;
        gp_scorenet net = net0;
        opaque(net.w_pose0), opaque(net.b_pose0), opaque(net.w_pose2), opaque(net.b_pose2), opaque(net.w_headx), opaque(net.w_out), opaque(net.b_out);
        if constexpr (MODEL == 1) opaque(net.w_headx_t), opaque(net.w_pose2_t), opaque(net.w_pose0_t);
        opaque(a.cvec);
        TrunkPre<P> pre;
        float sigma = 1.f;
        if (l < last) {
            trunk_begin<P>(net, pre, a.cvec, tvec, row0, a.nrows, a.kcand, heun_times(a));
            sigma = heun_sched_row<SROW>(a, rcls, l)[0];  // requested now, used after the trunk
            gp_pin(sigma);
        }
        if (tid < P) {
            float ev[9];  // x_i in, the point this index evaluates out
#pragma unroll
            for (int j = 0; j < 9; ++j) ev[j] = mine[j * P];
            if (l > 0) {
                const float *sc0 = a.sched + (size_t)l * SROW, *sc = heun_sched_row<SROW>(a, rcls, l);  // control flow from class 0
                const int kind = (int)sc0[3];
                const float c = sc[1], h = sc[2];
                // the previous index's f_theta (all of trunk_ftheta's barriers are behind us); the chain stores this quotient and reloads it
                // (MODEL 1: the previous index's score itself, in the backward pass's output rows)
                const float *F = MODEL == 1 ? lds + gp_bwd::OFF_U + tid * gp_bwd::LDS_OUT : lds + L::OFF_H1 + tid * L::LDH;
                float gr[9], dv[9];
                if constexpr (SOLVER == SOLVER_DPM2M) {
                    const bool has_d = (kind == DPM2M_STEP || kind == DPM2M_STEP_LAST) && sc0[5] != 0.f;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        gr[j] = MODEL == 1 ? F[j] : F[j] / (sigma_prev + 1e-7f);
                        dv[j] = has_d ? mine[(9 + j) * P] : 0.f;
                    }
                    dpm2m_update_row(kind, ev, dv, gr, c, h, sc[4], sc[5]);
                    if (kind == DPM2M_STEP) {  // parks D_{l-1} for the next index
#pragma unroll
                        for (int j = 0; j < 9; ++j) mine[(9 + j) * P] = dv[j];
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        gr[j] = MODEL == 1 ? F[j] : F[j] / (sigma_prev + 1e-7f);
                        dv[j] = kind == HEUN_CORRECT || kind == HEUN_CORRECT_LAST ? mine[(9 + j) * P] : 0.f;
                    }
                    heun_update_row(kind, ev, dv, gr, c, h);
                }
                if (SOLVER == SOLVER_HEUN && kind == HEUN_PREDICT) {  // keeps x_i (the chain never stores the Euler point) and parks d_i
#pragma unroll
                    for (int j = 0; j < 9; ++j) mine[(9 + j) * P] = dv[j];
                } else {
                    if (kind != HEUN_DENOISE) {
#pragma unroll
                        for (int j = 0; j < 9; ++j) mine[j * P] = ev[j];
                    }
                    if (live) {
                        const float cen[3] = {mine[18 * P], mine[19 * P], mine[20 * P]};
                        HeunArgs al = a;
                        al.step = l, al.d = nullptr;
                        heun_store_row<SOLVER>(al, kind, r, ev, dv, cen);
                    }
                }
            }
            // hand the evaluation point to the trunk through LDS
            float *xr = lds + tid * L::LD0;
#pragma unroll
            for (int j = 0; j < 9; ++j) xr[j] = ev[j];
#pragma unroll
            for (int j = 9; j < 16; ++j) xr[j] = 0.f;
        }
        if (l == last) break;
        __syncthreads();  // X0 is complete, and the row threads have read the previous f_theta out of H1, before layer 1 overwrites it
        if constexpr (MODEL == 1)
            gp_bwd::score_vjp_tile<gp_bwd::ENERGY>(lds, net, a.cvec, tvec, row0, a.nrows, a.kcand, pre, sigma);  // (ends on a barrier too)
        else
            trunk_ftheta<P, false, TrunkNoEmit, false, (P == 48)>(lds, net, a.cvec, tvec, row0, a.nrows, a.kcand, pre, TrunkNoEmit(), 0, heun_times(a));  // (ends on a barrier: f_theta is visible to the row threads)
        sigma_prev = sigma;
    }
}

template <int P, int MODEL = 0>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void heun_solve_kernel(HeunArgs a, const gp_scorenet net0) {
    heun_solve<P, SOLVER_HEUN, MODEL>(a, net0);
}
template <int P, int MODEL = 0>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void dpm2m_solve_kernel(HeunArgs a, const gp_scorenet net0) {
    heun_solve<P, SOLVER_DPM2M, MODEL>(a, net0);
}
template <int P>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void heun_solve_classes_kernel(HeunClsArgs a, const gp_scorenet net0) {
    heun_solve<P, SOLVER_HEUN, 0>(a, net0);
}
template <int P>
__global__ __launch_bounds__(TrunkCfg<P>::NT) void dpm2m_solve_classes_kernel(HeunClsArgs a, const gp_scorenet net0) {
    heun_solve<P, SOLVER_DPM2M, 0>(a, net0);
}

// the trunk's block and 21 floats per row behind it
template <int P>
constexpr size_t solve_lds_bytes() {
    return trunk_lds_bytes<P>() + (size_t)21 * P * sizeof(float);
}

template <int SOLVER, int P, int MODEL = 0>
constexpr auto solve_kernel = heun_solve_kernel<P, MODEL>;
template <int P, int MODEL>
constexpr auto solve_kernel<SOLVER_DPM2M, P, MODEL> = dpm2m_solve_kernel<P, MODEL>;
template <int SOLVER, int P>
constexpr auto solve_classes_kernel = heun_solve_classes_kernel<P>;
template <int P>
constexpr auto solve_classes_kernel<SOLVER_DPM2M, P> = dpm2m_solve_classes_kernel<P>;

// A whole solve as one launch (gp_heun_solve_tile, gp_dpm2m_solve_tile and their _model forms: model 1 on plan 16 only; CLASSES:
// gp_heun_solve_classes, gp_dpm2m_solve_classes - schedule classes, the score model).
template <int SOLVER, bool CLASSES = false>
int solve_tile(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net, const float *cvec, const float *tvec_all,
               const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj, hipStream_t st, int ncls = 1,
               const int *cls = nullptr) {
    if ((model != 0 && model != 1) || ngroups <= 0 || nclouds_per_group < 0 || k <= 0 || nsteps < 1 || !net || !cvec || !tvec_all || !sched || !centre || !x ||
        !d || !score || !out)
        return GP_EINVAL;
    if (CLASSES && (model != 0 || ncls < 1 || ncls > GP_MAX_SCHED_CLASSES || !cls)) return GP_EINVAL;
    const long long rg = (long long)nclouds_per_group * k, R = ngroups * rg;
    if (R > 0x7fffffffLL / 9) return GP_EINVAL;  // row and element indices are ints up to R * 9
    if (R == 0) return GP_OK;
    int P = 0;
    const int rc = gp_heun_layout_model(model, tile, ngroups, nclouds_per_group, k, &P);
    if (rc != GP_OK) return rc;
    const HeunArgs a = heun_args((int)R, k, 0, fixed_launches<SOLVER>(nsteps, denoise) - 1, cvec, tvec_all, sched, centre, x, d, score, out, traj);
    if (model == 1) {
        if (P != 16 || !net->w_headx_t || !net->w_pose2_t || !net->w_pose0_t) return GP_EINVAL;  // (plan 128 keeps its per-launch kernels)
        constexpr size_t lds = gp_bwd::LDS_BYTES + (size_t)21 * 16 * sizeof(float);  // the backward pass's block and 21 floats per row behind it
        return gp_launch<solve_kernel<SOLVER, 16, 1>>(dim3(ngroups * (int)((rg + 15) / 16)), dim3(TrunkCfg<16>::NT), lds, st, a, *net);
    }
    return gp_with_tile(P, [&](auto tile_rows) {  // (GP_EINVAL for plan 128: the chain form keeps its per-launch kernels)
        constexpr int T = decltype(tile_rows)::value;
        const int nwg = ngroups * (int)((rg + T - 1) / T);
        if constexpr (CLASSES)
            return gp_launch<solve_classes_kernel<SOLVER, T>>(dim3(nwg), dim3(TrunkCfg<T>::NT), solve_lds_bytes<T>(), st, heun_cls_args(a, ncls, cls, nsteps + 1), *net);
        else
            return gp_launch<solve_kernel<SOLVER, T>>(dim3(nwg), dim3(TrunkCfg<T>::NT), solve_lds_bytes<T>(), st, a, *net);
    });
}

}  // namespace

extern "C" int gp_heun_solve_tile(int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                                  const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                                  gp_stream_t s) {
    return solve_tile<SOLVER_HEUN>(0, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj, (hipStream_t)s);
}

extern "C" int gp_dpm2m_solve_tile(int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net, const float *cvec,
                                   const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score, float *out, float *traj,
                                   gp_stream_t s) {
    return solve_tile<SOLVER_DPM2M>(0, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj, (hipStream_t)s);
}

extern "C" int gp_heun_solve_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                                     const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                                     float *out, float *traj, int ncls, const int *cls, gp_stream_t s) {
    return solve_tile<SOLVER_HEUN, true>(model, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                         (hipStream_t)s, ncls, cls);
}

extern "C" int gp_dpm2m_solve_classes(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                                      const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                                      float *out, float *traj, int ncls, const int *cls, gp_stream_t s) {
    return solve_tile<SOLVER_DPM2M, true>(model, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                          (hipStream_t)s, ncls, cls);
}

extern "C" int gp_heun_solve_tile_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                                        const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                                        float *out, float *traj, gp_stream_t s) {
    return solve_tile<SOLVER_HEUN>(model, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                   (hipStream_t)s);
}

extern "C" int gp_dpm2m_solve_tile_model(int model, int tile, int ngroups, int nclouds_per_group, int k, int nsteps, int denoise, const gp_scorenet *net,
                                         const float *cvec, const float *tvec_all, const float *sched, const float *centre, float *x, float *d, float *score,
                                         float *out, float *traj, gp_stream_t s) {
    return solve_tile<SOLVER_DPM2M>(model, tile, ngroups, nclouds_per_group, k, nsteps, denoise, net, cvec, tvec_all, sched, centre, x, d, score, out, traj,
                                    (hipStream_t)s);
}
