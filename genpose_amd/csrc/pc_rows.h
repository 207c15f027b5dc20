// The predictor-corrector (PC) sampler step's contract (cond_pc_sampler, samplers.py:102-160), in ONE place for the three kernels in
// which a WAVE owns its rows from the sampler update to the score (128 rows per workgroup):
//     pc_step_chain_kernel<2, MODEL>  (scorenet.hip, fp32 MFMA)    PT = 2 row tiles per wave, NW = 4 waves
//     pc_step_chain_kernel_bf16x9     (trunk_bf16x9.hip)           PT = 2, NW = 4
//     pc_step_bf16x3_kernel           (trunk_bf16x3.hip)           PT = 1, NW = 8
// The launch for step i (0 <= i <= nsteps): i > 0 finishes step i-1 for the wave's rows (Langevin corrector + Euler-Maruyama
// predictor) using score_{i-1} and the batch-mean gradient norm; i < nsteps evaluates score_i and writes one partial sum of |score_i|
// per WAVE; i == nsteps finishes only and post-processes mean_x.  What lives here and nowhere else: the argument block, the clamped
// ragged rows, the fixed order of the gradient-norm sum (results are bit-reproducible across plans), the statistic from outside
// (gn_ext), the trajectory's centre offset, and the score / partial stores.  Each kernel keeps its own matrix core and weight ring.
// The tile kernel pc_step_kernel<P, MODEL, SPLIT> (row work on tid < P, the norm through LDS) is a different shape: it shares PcArgs
// and pc_update_row only.
#pragma once
#include <type_traits>

#include "philox.h"
#include "score_trunk.h"

namespace gp_trunk {

struct PcArgs {
    int nrows, kcand, step, nsteps;
    int nparts, ppg, rows_per_group;  // partial sums of |score| per step / per batch (group): the batch-mean gradient norm is per group
    int wgpg;                         // workgroups per group
    const float *cvec, *tvec_all;    // tvec_all [nsteps][768]
    const float *sched;              // [nsteps][4]: sigma(t_i), g(t_i), step_size, sqrt(step_size)  (f32, host schedule)
    const float *z_lang, *z_pred;    // [nsteps][R][9]; the SEEDED instantiations (philox.h) draw in registers instead and find their seed
                                     //   state (gp_philox::SEED_WORDS words) behind z_lang, z_pred is null
    const float *centre;             // [R/k... per cloud][3]
    float *x, *mean_x, *score, *partials, *traj;  // x,mean_x,score [R,9]; partials [nsteps][nparts]; traj [nsteps][R][9] or null
    const float *gn_ext;             // [nsteps][ngroups] or null: the batch's gradient-norm statistic supplied from outside (a batch that is
    int ngroups;                     //   sharded over several GPUs, all-reduced between the launches): the SUM of |score| over all its
    float gn_rows;                   //   rows when gn_rows > 0 (= that row count), else the mean itself
    // head-split plan (GP_PLAN_HEADSPLIT): workgroup 3 t + h evaluates head h of 16-row tile t and owns components 3 h .. 3 h + 2 of the
    // score.  THREE workgroups read a tile's state and score and each writes a part of them, so nothing a launch reads may be written by
    // the same launch: every step keeps its own copies in its row of `partials` (nparts = 21 * nrows floats per step):
    //     [0, 3R)     sum of squares of row r's three components of head h at 3 r + h (a row's norm needs all nine: the NEXT launch puts
    //                 sqrt(p[3r] + p[3r+1] + p[3r+2]) together and reduces it over its batch's rows)
    //     [3R, 12R)   score_i [R][9], read by launch i + 1
    //     [12R, 21R)  the state after launch i's update [R][9], read by launch i + 1 (launch 1 reads the initial state from `x`, which
    //                 this plan never writes)
    // (wgpg counts TILES per group.)
};

// The arguments every plan shares (wgpg = workgroups, or head-split tiles, per group of rg rows).
static inline PcArgs pc_args(int ngroups, int rg, int k, int step, int nsteps, int nparts, int wgpg, const float *cvec, const float *tvec_all,
                             const float *sched, const float *z_langevin, const float *z_predictor, const float *centre, float *x, float *mean_x,
                             float *score, float *partials, float *traj, const float *gn_ext, int gn_rows_total) {
    PcArgs a;
    a.nrows = ngroups * rg, a.kcand = k, a.step = step, a.nsteps = nsteps;
    a.nparts = nparts, a.ppg = nparts / ngroups, a.rows_per_group = rg, a.wgpg = wgpg;
    a.cvec = cvec, a.tvec_all = tvec_all, a.sched = sched, a.z_lang = z_langevin, a.z_pred = z_predictor, a.centre = centre;
    a.x = x, a.mean_x = mean_x, a.score = score, a.partials = partials, a.traj = traj;
    a.gn_ext = gn_ext, a.ngroups = ngroups, a.gn_rows = (float)gn_rows_total;
    return a;
}

// The fixed-step Heun solver of the probability-flow ODE (cond_edm_sampler's second-order method, samplers.py:230-290, on the VE score
// model): the same launch shape with a ROW-LOCAL update (heun_update_row, score_trunk.h) - no noise operands, no partial sums, no gn; one
// more [R,9] buffer holds the slope d_i between a step's two launches.  `step` is the LAUNCH index and `nsteps` the index of the last
// launch, which finishes only - so `step > 0` (there is an update), `step < nsteps` (there is an evaluation) and `step == nsteps` read as
// they do in PcArgs.  With N steps: launch 0 evaluates score(x_0, t_0); launch 2i+1 forms and stores d_i, evaluates the Euler point at
// t_{i+1}; launch 2i+2 forms and stores x_{i+1}, evaluates it at t_{i+1}; launch 2N's evaluation at (x_N, eps) is the denoising one and
// launch 2N+1 applies it (without denoising launch 2N finishes).  The kernels know nothing about the grid: everything comes from `sched`.
struct HeunArgs {
    int nrows, kcand, step, nsteps;
    const float *cvec, *tvec_all;  // tvec_all [N+1][768]: one row per evaluated time, launch l evaluates at row (l + 1) / 2
    const float *sched;            // [launches][4]: sigma of the launch's evaluation (the score's divisor), slope factor c, step h, kind (HEUN_*)
    const float *centre;           // [clouds][3]
    float *x, *d, *score, *out, *traj;  // x, d, score, out [R,9]; traj [N][R][9] or null: x_1 .. x_N, rotations normalised, centres added
};
static inline HeunArgs heun_args(int nrows, int k, int launch, int last_launch, const float *cvec, const float *tvec_all, const float *sched,
                                 const float *centre, float *x, float *d, float *score, float *out, float *traj) {
    HeunArgs a;
    a.nrows = nrows, a.kcand = k, a.step = launch, a.nsteps = last_launch;
    a.cvec = cvec, a.tvec_all = tvec_all, a.sched = sched, a.centre = centre;
    a.x = x, a.d = d, a.score = score, a.out = out, a.traj = traj;
    return a;
}
// SCHEDULE CLASSES (the tile kernels heun_step_tile / heun_solve with HeunClsArgs; gp_*_step_classes, gp_*_solve_classes): a solve whose clouds
// start from different times in the same launches.  `cls [clouds]` gives every cloud's class, clamped into [0, ncls - 1] on the device;
// sched is [ncls][launches][row] and tvec_all [ncls][N+1][768].  Row r reads its cloud's class's schedule row (the score's divisor and the
// update's coefficients) and adds that class's time embedding; the launch kind - and DPM2M's "there is a previous denoiser" - is read from
// class 0 (the host keeps the kind column identical in every class), so control flow stays uniform and a row's bits are those of a uniform
// solve on its class's tables.
struct HeunClsArgs : HeunArgs {
    const int *cls;  // [clouds]
    int ncls;
    int tstride;     // floats between two classes' blocks of tvec_all: (N + 1) * 768
};
static inline HeunClsArgs heun_cls_args(const HeunArgs &u, int ncls, const int *cls, int ntimes) {
    HeunClsArgs a;
    static_cast<HeunArgs &>(a) = u;
    a.cls = cls, a.ncls = ncls, a.tstride = ntimes * HEADS;
    return a;
}
// how a row's cloud picks its time embedding, row r's class, and the schedule row (SROW floats) of launch l for a class
__device__ __forceinline__ TrunkOneTime heun_times(const HeunArgs &) { return TrunkOneTime(); }
__device__ __forceinline__ TrunkClassTime heun_times(const HeunClsArgs &a) { return TrunkClassTime{a.cls, a.ncls, (size_t)a.tstride}; }
__device__ __forceinline__ int heun_row_class(const HeunArgs &, int) { return 0; }
__device__ __forceinline__ int heun_row_class(const HeunClsArgs &a, int r) { return heun_times(a).cloud_class(r / a.kcand); }
template <int SROW>
__device__ __forceinline__ const float *heun_sched_row(const HeunArgs &a, int c, int l) {
    return a.sched + ((size_t)c * (a.nsteps + 1) + l) * SROW;
}

// The DPM-Solver++(2M) fixed-step solver (dpm2m_update_row, score_trunk.h) runs on the same launch shape, arguments and buffers: SOLVER
// below is a template value of the kernels' shared code, HeunArgs serve both.  With N steps there are N + 1 launches (+ 1 with denoise):
// launch 0 evaluates score(x_0, t_0); launch i = 1 .. N forms x_i from the stored score, x_{i-1} and D_{i-2}, stores x_i, D_{i-1} (in `d`,
// whose role between launches that is) and traj[i-1] and evaluates at (x_i, t_i) - unless it is the last; with denoise launch N's
// evaluation at (x_N, eps) is the denoising one and launch N + 1 applies it.  The time row a launch evaluates is its own index.  Its
// schedule is a table of its own, one row of DPM2M_SCHED floats per launch:
//     [0] sigma of the launch's evaluation (the score's divisor)   [3] kind (DPM2M_*)
//     [1] sigma_{i-1}^2             (DPM2M_DENOISE: g(eps))           [4] the weight of D_{i-1} times -expm1(-h_{i-1})
//     [2] sigma_i / sigma_{i-1}     (DPM2M_DENOISE: the step)         [5] the weight of D_{i-2} times -expm1(-h_{i-1}); 0: there is none
// (launch i's update is step i-1 of the method).  A zero in [5] marks the first step: D_{i-2} does not exist and `d` is not read.
enum { SOLVER_PC = 0, SOLVER_HEUN = 1, SOLVER_DPM2M = 2 };
constexpr int DPM2M_SCHED = 8;
template <int SOLVER>
constexpr int fixed_sched_row() {
    static_assert(SOLVER == SOLVER_HEUN || SOLVER == SOLVER_DPM2M, "the fixed-step solvers");
    return SOLVER == SOLVER_DPM2M ? DPM2M_SCHED : 4;
}
// launches of a solve (the host side of the two solvers is written once over SOLVER; each file names its kernels beside them)
template <int SOLVER>
static inline int fixed_launches(int nsteps, int denoise) {
    static_assert(SOLVER == SOLVER_HEUN || SOLVER == SOLVER_DPM2M, "the fixed-step solvers");
    return SOLVER == SOLVER_DPM2M ? gp_dpm2m_launches(nsteps, denoise) : gp_heun_launches(nsteps, denoise);
}
// the row of tvec_all a launch evaluates at (a bool reads as SOLVER_PC / SOLVER_HEUN)
template <int SOLVER>
__device__ __forceinline__ int pc_time_row(int step) {
    return SOLVER == SOLVER_HEUN ? (step + 1) >> 1 : step;
}
// what a Heun launch stores for a live row after heun_update_row (one thread per row); SOLVER_DPM2M: after dpm2m_update_row - D_{i-1} for
// the next launch (the one-launch solve keeps it on chip: d null), the trajectory row of its own index
template <int SOLVER = SOLVER_HEUN>
__device__ __forceinline__ void heun_store_row(const HeunArgs &a, int kind, int r, const float (&xv)[9], const float (&dv)[9], const float (&cen)[3]) {
    if constexpr (SOLVER == SOLVER_DPM2M) {
        if (kind == DPM2M_STEP && a.d) {
#pragma unroll
            for (int j = 0; j < 9; ++j) a.d[(size_t)r * 9 + j] = dv[j];
        }
    } else if (kind == HEUN_PREDICT) {
#pragma unroll
        for (int j = 0; j < 9; ++j) a.d[(size_t)r * 9 + j] = dv[j];
        return;
    }
    float o[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) o[j] = xv[j];
    normalize_rot6(o);
#pragma unroll
    for (int j = 0; j < 3; ++j) o[6 + j] += cen[j];
    if (kind != HEUN_DENOISE) {
#pragma unroll
        for (int j = 0; j < 9; ++j) a.x[(size_t)r * 9 + j] = xv[j];
        if (a.traj) {
            float *tr = a.traj + ((size_t)(SOLVER == SOLVER_DPM2M ? a.step - 1 : (a.step - 2) >> 1) * a.nrows + r) * 9;
#pragma unroll
            for (int j = 0; j < 9; ++j) tr[j] = o[j];
        }
    }
    if (kind != HEUN_CORRECT) {
#pragma unroll
        for (int j = 0; j < 9; ++j) a.out[(size_t)r * 9 + j] = o[j];
    }
}

// A wave's rows through one launch: lane (pt, g) = (lane & 15, lane >> 4) carries row 16 * (wave * PT + p) + pt of the workgroup for
// each tile p.  Every lane of a row's four lane groups carries the row's 9-vector (the update is ~150 VALU instructions per wave,
// computed redundantly by the four groups - cheaper than any exchange), lane group 0 stores.  The three phases keep one issue order
// on purpose (memory returns in order): request() asks for what the sampler update needs, the caller issues its ring prologue behind
// it, finish_previous() then runs the update while the weights are still on their way.
// SEEDED: the two 9-vectors of noise are not loaded but drawn (gp_philox::draw9: seed state behind a.z_lang, global row = its row base
// + the row of the launch) right before the update - the same values gp_pc_noise_fill writes, the same update expression after them.
// SOLVER_HEUN: the Heun solver's launches (HeunArgs) - the overloads of request / finish_previous below; zz1 carries d_i, gdiff the slope
// factor, dt the step.  SOLVER_DPM2M: the DPM-Solver++(2M) launches through the same overloads; zz1 carries D_{i-2}, gdiff / dt / sqdt / gn
// the schedule row's [1] / [2] / [4] / [5].
struct PcNoSeed {};
template <int PT, bool SEEDED = false, int SOLVER = SOLVER_PC>
struct PcRows {
    static constexpr bool HEUN = SOLVER != SOLVER_PC;
    static_assert(!(SEEDED && HEUN), "the fixed-step updates draw no noise");
    int row[PT];
    float xv[PT][9], gr[PT][9], zz1[PT][9], zz2[PT][9], cen[PT][3];
    typename std::conditional<SEEDED, gp_philox::Seed, PcNoSeed>::type seed;
    float gdiff, dt, sqdt, gn, sigma;
    float psum[4];    // the batch's first 256 partial sums, one per lane and quarter
    const float *pp;  // the batch's partial sums of step i-1
    int kind;         // HEUN: the launch's kind (HEUN_* / DPM2M_*)

    // (1) the rows' operands, then the schedule and the batch's partial sums (or the statistic from outside), then sigma(t_i)
    template <int NW>
    __device__ __forceinline__ void request(const PcArgs &a, int wave, int lane) {
        const int i = a.step, pt = lane & 15, wg_row0 = blockIdx.x * (16 * PT * NW);
#pragma unroll
        for (int p = 0; p < PT; ++p) row[p] = wg_row0 + (wave * PT + p) * 16 + pt;
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int r = row[p] < a.nrows ? row[p] : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
#pragma unroll
            for (int j = 0; j < 9; ++j) xv[p][j] = a.x[(size_t)r * 9 + j];
            if (i > 0) {
                if constexpr (SEEDED) {
#pragma unroll
                    for (int j = 0; j < 9; ++j) gr[p][j] = a.score[(size_t)r * 9 + j];
                } else {
                    const float *z1 = a.z_lang + ((size_t)(i - 1) * a.nrows + r) * 9;
                    const float *z2 = a.z_pred + ((size_t)(i - 1) * a.nrows + r) * 9;
#pragma unroll
                    for (int j = 0; j < 9; ++j) {
                        gr[p][j] = a.score[(size_t)r * 9 + j];
                        zz1[p][j] = z1[j];
                        zz2[p][j] = z2[j];
                    }
                }
                const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
                cen[p][0] = cp[0], cen[p][1] = cp[1], cen[p][2] = cp[2];
            }
        }
        if constexpr (SEEDED) {
            if (i > 0) seed = gp_philox::load_seed(reinterpret_cast<const uint32_t *>(a.z_lang));
        }
        const int grp = blockIdx.x / a.wgpg;
        pp = a.partials + (size_t)(i > 0 ? i - 1 : 0) * a.nparts + (size_t)grp * a.ppg;
        // (locals, assigned to the members once: two branches that store to different members of one object keep it out of registers)
        float gdiff_ = 0.f, dt_ = 0.f, sqdt_ = 0.f, gn_ = 1.f, sigma_ = 1.f, psum_[4] = {0.f, 0.f, 0.f, 0.f};
        if (i > 0) {
            const float *sc = a.sched + (size_t)(i - 1) * 4;
            gdiff_ = sc[1], dt_ = sc[2], sqdt_ = sc[3];
            if (a.gn_ext) {
                gn_ = a.gn_ext[(size_t)(i - 1) * a.ngroups + grp];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u) psum_[u] = lane + 64 * u < a.ppg ? pp[lane + 64 * u] : 0.f;
            }
        }
        if (i < a.nsteps) sigma_ = a.sched[(size_t)i * 4 + 0];
        gdiff = gdiff_, dt = dt_, sqdt = sqdt_, gn = gn_, sigma = sigma_;
#pragma unroll
        for (int u = 0; u < 4; ++u) psum[u] = psum_[u];
    }

    // (3) finish step i-1: the batch mean of |score_{i-1}| - every wave reduces its batch's partial sums in the same fixed order
    // (identical in all waves: deterministic) - then the update and the stores.  True when the launch is the finish-only one: the
    // caller returns.
    __device__ __forceinline__ bool finish_previous(const PcArgs &a, int lane) {
        const int i = a.step, g = lane >> 4;
        if (i == 0) return false;
        if (a.gn_ext) {
            if (a.gn_rows > 0.f) gn = gn / a.gn_rows;
        } else {
            float s = ((psum[0] + psum[1]) + psum[2]) + psum[3];  // the order of `for (q = lane; q < ppg; q += 64) s += pp[q]`
            for (int q = lane + 256; q < a.ppg; q += 64) s += pp[q];
            gn = wave_sum_f32(s) / (float)a.rows_per_group;
        }
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            float mx[9];
            if constexpr (SEEDED) {
                const uint64_t grow = seed.row_base + (uint64_t)(row[p] < a.nrows ? row[p] : a.nrows - 1);
                gp_philox::draw9(seed, (uint32_t)(i - 1), gp_philox::STREAM_LANGEVIN, grow, zz1[p]);
                gp_philox::draw9(seed, (uint32_t)(i - 1), gp_philox::STREAM_PREDICTOR, grow, zz2[p]);
            }
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
        return i == a.nsteps;
    }

    // HEUN (1): the rows' state, the stored score and, for a corrector launch, d_i; the launch's row of the schedule
    template <int NW>
    __device__ __forceinline__ void request(const HeunArgs &a, int wave, int lane) {
        static_assert(HEUN, "HeunArgs drive the HEUN instantiations");
        const int i = a.step, pt = lane & 15, wg_row0 = blockIdx.x * (16 * PT * NW);
        const float *sc = a.sched + (size_t)i * fixed_sched_row<SOLVER>();
        const int kind_ = (int)sc[3];
#pragma unroll
        for (int p = 0; p < PT; ++p) row[p] = wg_row0 + (wave * PT + p) * 16 + pt;
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            const int r = row[p] < a.nrows ? row[p] : a.nrows - 1;  // rows past the end: clamped duplicates (computed, never stored)
#pragma unroll
            for (int j = 0; j < 9; ++j) xv[p][j] = a.x[(size_t)r * 9 + j];
            if (i > 0) {
#pragma unroll
                for (int j = 0; j < 9; ++j) gr[p][j] = a.score[(size_t)r * 9 + j];
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    if constexpr (SOLVER == SOLVER_DPM2M)  // D_{i-2}, unless this is the first step (no such denoiser: weight 0)
                        zz1[p][j] = (kind_ == DPM2M_STEP || kind_ == DPM2M_STEP_LAST) && sc[5] != 0.f ? a.d[(size_t)r * 9 + j] : 0.f;
                    else
                        zz1[p][j] = kind_ == HEUN_CORRECT || kind_ == HEUN_CORRECT_LAST ? a.d[(size_t)r * 9 + j] : 0.f;
                }
                const float *cp = a.centre + (size_t)(r / a.kcand) * 3;
                cen[p][0] = cp[0], cen[p][1] = cp[1], cen[p][2] = cp[2];
            }
        }
        sigma = sc[0], gdiff = sc[1], dt = sc[2], kind = kind_;
        if constexpr (SOLVER == SOLVER_DPM2M) sqdt = sc[4], gn = sc[5];
    }

    // HEUN (3): the update and the stores.  True when the launch is the finish-only one: the caller returns.
    __device__ __forceinline__ bool finish_previous(const HeunArgs &a, int lane) {
        static_assert(HEUN, "HeunArgs drive the HEUN instantiations");
        if (a.step == 0) return false;
#pragma unroll
        for (int p = 0; p < PT; ++p) {
            if constexpr (SOLVER == SOLVER_DPM2M)
                dpm2m_update_row(kind, xv[p], zz1[p], gr[p], gdiff, dt, sqdt, gn);
            else
                heun_update_row(kind, xv[p], zz1[p], gr[p], gdiff, dt);
            if (row[p] < a.nrows && (lane >> 4) == 0) heun_store_row<SOLVER>(a, kind, row[p], xv[p], zz1[p], cen[p]);
        }
        return a.step == a.nsteps;
    }
};

// Components j0 .. j0 + N - 1 of a row's score are final: stored by lane group 0, their squares summed into q in component order.
template <int N, class Args>
__device__ __forceinline__ void pc_store_score(const Args &a, int row, int lane, int j0, const float (&sc)[N], float &q) {
#pragma unroll
    for (int c = 0; c < N; ++c) q += sc[c] * sc[c];
    if (row < a.nrows && lane < 16) {
#pragma unroll
        for (int c = 0; c < N; ++c) a.score[(size_t)row * 9 + j0 + c] = sc[c];
    }
}

// The wave's partial sum of |score_i| over its live rows (q: the rows' sums of squares).
template <int PT, int NW>
__device__ __forceinline__ void pc_store_partial(const PcArgs &a, const int (&row)[PT], const float (&q)[PT], int wave, int lane) {
    float nsum = 0.f;
#pragma unroll
    for (int p = 0; p < PT; ++p)
        if (row[p] < a.nrows && lane < 16) nsum += sqrtf(q[p]);
    nsum = wave_sum_f32(nsum);
    if (lane == 0) a.partials[(size_t)a.step * a.nparts + (size_t)blockIdx.x * NW + wave] = nsum;
}

}  // namespace gp_trunk
