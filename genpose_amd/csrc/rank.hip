// Energy ranking and top-k pose aggregation, one wave per cloud.
// Reference: sort_poses_by_energy (networks/reward.py:131-155: rotation and translation are ranked INDEPENDENTLY by
// their own energy channel), sort_sRT_by_energy(..., ratio, 'average') (utils/sgpa_utils.py:897-954) ==
// cal_average_sRT (runners/evaluation_tracking.py:60-77): 6-D -> matrix (Gram-Schmidt) -> quaternion (pytorch3d
// matrix_to_quaternion) -> sign-align w>0 -> A = mean(q q^T) -> eigenvector of the largest eigenvalue
// (utils/misc.py:227-249) + mean translation.  The reference does this through .cpu().numpy().tolist() index lists
// and torch.linalg.eigh; here it is one launch (4x4 Jacobi in f64 registers).
#include "gp_common.h"

namespace {

template <typename T>
__device__ __forceinline__ void rot6_to_matrix(const T *p, double R[3][3]) {
    // get_rot_matrix('rot_matrix') (utils/misc.py:136): columns b1, b2, b3 = b1 x b2
    double a1[3] = {(double)p[0], (double)p[1], (double)p[2]}, a2[3] = {(double)p[3], (double)p[4], (double)p[5]};
    double n1 = sqrt(a1[0] * a1[0] + a1[1] * a1[1] + a1[2] * a1[2]);
    n1 = n1 > 1e-12 ? n1 : 1e-12;
    double b1[3] = {a1[0] / n1, a1[1] / n1, a1[2] / n1};
    double d = b1[0] * a2[0] + b1[1] * a2[1] + b1[2] * a2[2];
    double c[3] = {a2[0] - d * b1[0], a2[1] - d * b1[1], a2[2] - d * b1[2]};
    double n2 = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    n2 = n2 > 1e-12 ? n2 : 1e-12;
    double b2[3] = {c[0] / n2, c[1] / n2, c[2] / n2};
    double b3[3] = {b1[1] * b2[2] - b1[2] * b2[1], b1[2] * b2[0] - b1[0] * b2[2], b1[0] * b2[1] - b1[1] * b2[0]};
    for (int i = 0; i < 3; ++i) R[i][0] = b1[i], R[i][1] = b2[i], R[i][2] = b3[i];
}

__device__ __forceinline__ void matrix_to_quat(const double m[3][3], double q[4]) {
    // pytorch3d v0.7.2 matrix_to_quaternion: candidate with the largest |q_i|, divisor floored at 0.1
    // (every array index below is a compile-time constant: the arrays live in registers, no scratch)
    double qa[4] = {1.0 + m[0][0] + m[1][1] + m[2][2], 1.0 + m[0][0] - m[1][1] - m[2][2], 1.0 - m[0][0] + m[1][1] - m[2][2],
                    1.0 - m[0][0] - m[1][1] + m[2][2]};
#pragma unroll
    for (int i = 0; i < 4; ++i) qa[i] = qa[i] > 0 ? sqrt(qa[i]) : 0.0;
    int best = 0;
    double qb = qa[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (qa[i] > qb) best = i, qb = qa[i];
    double c[4];
    if (best == 0) {
        c[0] = qa[0] * qa[0], c[1] = m[2][1] - m[1][2], c[2] = m[0][2] - m[2][0], c[3] = m[1][0] - m[0][1];
    } else if (best == 1) {
        c[0] = m[2][1] - m[1][2], c[1] = qa[1] * qa[1], c[2] = m[1][0] + m[0][1], c[3] = m[0][2] + m[2][0];
    } else if (best == 2) {
        c[0] = m[0][2] - m[2][0], c[1] = m[1][0] + m[0][1], c[2] = qa[2] * qa[2], c[3] = m[1][2] + m[2][1];
    } else {
        c[0] = m[1][0] - m[0][1], c[1] = m[2][0] + m[0][2], c[2] = m[2][1] + m[1][2], c[3] = qa[3] * qa[3];
    }
    const double den = 2.0 * (qb > 0.1 ? qb : 0.1);
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = c[i] / den;
}

// eigenvector of the largest eigenvalue of a symmetric 4x4 (cyclic Jacobi).  The (p, q) sweeps are unrolled: A and V are indexed by
// constants only and stay in registers (round 5's dynamically indexed form cost 64 scratch instructions on the tracking path).
__device__ __forceinline__ void top_eigvec4(double (&A)[4][4], double (&v)[4]) {
    double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += A[p][q] * A[p][q];
        if (off < 1e-60) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double bv = A[0][0];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = V[i][0];
#pragma unroll
    for (int b = 1; b < 4; ++b)
        if (A[b][b] > bv) {
            bv = A[b][b];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = V[i][b];
        }
}

// [7] (w, x, y, z, t) f32 -> [4][4] f32: pytorch3d quaternion_to_matrix (two_s = 2 / |q|^2) + the translation
__device__ __forceinline__ void quat_trans_to_rt(const float *q, float *o) {
    const float r = q[0], a = q[1], b = q[2], c = q[3];
    const float two_s = 2.0f / (((r * r + a * a) + b * b) + c * c);
    o[0] = 1.f - two_s * (b * b + c * c), o[1] = two_s * (a * b - c * r), o[2] = two_s * (a * c + b * r), o[3] = q[4];
    o[4] = two_s * (a * b + c * r), o[5] = 1.f - two_s * (a * a + c * c), o[6] = two_s * (b * c - a * r), o[7] = q[5];
    o[8] = two_s * (a * c - b * r), o[9] = two_s * (b * c + a * r), o[10] = 1.f - two_s * (a * a + b * b), o[11] = q[6];
    o[12] = o[13] = o[14] = 0.f, o[15] = 1.f;
}

// Ranking, sorted copies and aggregation of one cloud by one wave, from the energies already in LDS: e [k][2], ord [k][2] (candidate index
// at each rank) and quat [sel][4] are the caller's LDS, `poses` the cloud's own [k][9].  The callers put a barrier between the last write
// of e and this.  Optional outputs (any may be NULL): sorted_rt [k][4][4] f64 = gp_pose9_to_rt of the sorted poses, avg_rt [4][4] f32 =
// gp_quat_trans_to_rt of avg_pose (same arithmetic, same bits).
template <typename T>
__device__ __forceinline__ void rank_aggregate_cloud(int b, int k, int sel, const T *__restrict__ poses, const float *e, int *ord, double *quat,
                                                     T *__restrict__ sorted_poses, float *__restrict__ sorted_energy, int32_t *__restrict__ order,
                                                     float *__restrict__ avg_pose, double *__restrict__ sorted_rt, float *__restrict__ avg_rt) {
    const int tid = threadIdx.x;
    // stable descending rank by counting (torch.sort(descending=True, stable=True); ties keep candidate order).  The order is
    // torch's: every NaN ranks above +inf and NaNs tie with each other, -0.0 ties with +0.0.  With the plain `>` / `==` a NaN
    // compares false both ways, two candidates share a rank and some ord slots stay unwritten (read below as pose indices).
    for (int i = tid; i < k; i += 64) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float ei = e[2 * i + c];
            const bool ni = isnan(ei);
            int r = 0;
            for (int j = 0; j < k; ++j) {
                const float ej = e[2 * j + c];
                const bool nj = isnan(ej);
                const bool above = (nj && !ni) || (ej > ei);
                const bool tie = (nj && ni) || (ej == ei);
                r += above || (tie && j < i);
            }
            ord[2 * r + c] = i;
        }
    }
    __syncthreads();
    for (int r = tid; r < k; r += 64) {
        const int ir = ord[2 * r + 0], it = ord[2 * r + 1];
        const size_t o = ((size_t)b * k + r);
        if (order) {
            order[o * 2 + 0] = ir;
            order[o * 2 + 1] = it;
        }
        if (sorted_energy) {
            sorted_energy[o * 2 + 0] = e[2 * ir + 0];
            sorted_energy[o * 2 + 1] = e[2 * it + 1];
        }
        T sp[9];
#pragma unroll
        for (int j = 0; j < 6; ++j) sp[j] = poses[(size_t)ir * 9 + j];
#pragma unroll
        for (int j = 6; j < 9; ++j) sp[j] = poses[(size_t)it * 9 + j];
        if (sorted_poses) {
#pragma unroll
            for (int j = 0; j < 9; ++j) sorted_poses[o * 9 + j] = sp[j];
        }
        if (sorted_rt) {
            double R[3][3];
            rot6_to_matrix<T>(sp, R);
            double *m = sorted_rt + o * 16;
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                m[4 * rr + 0] = R[rr][0], m[4 * rr + 1] = R[rr][1], m[4 * rr + 2] = R[rr][2];
                m[4 * rr + 3] = (double)sp[6 + rr];
            }
            m[12] = m[13] = m[14] = 0.0, m[15] = 1.0;
        }
    }
    if (!avg_pose) return;
    for (int r = tid; r < sel; r += 64) {
        double R[3][3], q[4];
        rot6_to_matrix<T>(poses + (size_t)ord[2 * r + 0] * 9, R);
        matrix_to_quat(R, q);
        const double sgn = q[0] > 0 ? 1.0 : -1.0;  // ((q_w > 0) - 0.5) * 2  (misc.py:242)
#pragma unroll
        for (int i = 0; i < 4; ++i) quat[4 * r + i] = sgn * q[i];
    }
    __syncthreads();
    // A = mean(q q^T): lane l < 16 sums element (l / 4, l % 4) over the selected candidates in rank order (the order the serial loop of
    // rounds 1-5 used: same bits); every lane then holds all of A (wave shuffles) and runs the Jacobi iteration redundantly
    double mine = 0.0;
    {
        const int i = (tid >> 2) & 3, j = tid & 3;
        for (int r = 0; r < sel; ++r) mine += quat[4 * r + i] * quat[4 * r + j];
        mine /= (double)sel;
    }
    double A[4][4], v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) A[i][j] = __shfl(mine, 4 * i + j, 64);
    top_eigvec4(A, v);
    const double sgn = v[0] > 0 ? 1.0 : -1.0;
    // mean translation: lanes 0..2, one component each, candidates in rank order of the translation energy
    double tm = 0.0;
    if (tid < 3) {
        for (int r = 0; r < sel; ++r) tm += (double)poses[(size_t)ord[2 * r + 1] * 9 + 6 + tid];
        tm /= (double)sel;
    }
    float qt[7];
#pragma unroll
    for (int i = 0; i < 4; ++i) qt[i] = (float)(sgn * v[i]);
#pragma unroll
    for (int i = 0; i < 3; ++i) qt[4 + i] = (float)__shfl(tm, i, 64);
    if (tid == 0) {
        float *o = avg_pose + (size_t)b * 7;
#pragma unroll
        for (int i = 0; i < 7; ++i) o[i] = qt[i];
        if (avg_rt) quat_trans_to_rt(qt, avg_rt + (size_t)b * 16);
    }
}

// One wave per cloud: ranking, sorted copies, aggregation - and (optional) the 4x4 forms the runners hand on, so that the ranking step of a
// tracking frame is this ONE launch.
template <typename T>
__global__ __launch_bounds__(64) void rank_aggregate_kernel(int k, int sel, const T *__restrict__ poses, const float *__restrict__ energy,
                                                            T *__restrict__ sorted_poses, float *__restrict__ sorted_energy,
                                                            int32_t *__restrict__ order, float *__restrict__ avg_pose,
                                                            double *__restrict__ sorted_rt, float *__restrict__ avg_rt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *e = reinterpret_cast<float *>(smem);                   // [k][2]
    int *ord = reinterpret_cast<int *>(e + 2 * k);                // [k][2]: candidate index at each rank
    double *quat = reinterpret_cast<double *>(ord + 2 * k);  // [sel][4] (offset 16k bytes: 8-byte aligned)
    const int b = blockIdx.x, tid = threadIdx.x;
    poses += (size_t)b * k * 9;
    energy += (size_t)b * k * 2;
    for (int i = tid; i < 2 * k; i += 64) e[i] = energy[i];
    __syncthreads();
    rank_aggregate_cloud<T>(b, k, sel, poses, e, ord, quat, sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
}

// ---------------------------------------------------------------------------------------------- consensus score
// Ranks a cloud's candidates by their mutual agreement (ours; no network): the score of candidate i is minus the mean distance to the
// cloud's other finite candidates, column 0 by rotation, column 1 by translation (include/genpose_hip.h, section D).  LDS per candidate:
// its Gram-Schmidt matrix (row-major) and translation, 12 f64, written once, and a finiteness flag.
constexpr int CONS_F64 = 12;
constexpr size_t CONS_LDS_PER_K = CONS_F64 * sizeof(double) + sizeof(int);

template <typename T>
__device__ __forceinline__ void consensus_stage(int k, const T *__restrict__ poses, double *rt, int *fin) {
    for (int i = threadIdx.x; i < k; i += 64) {
        T p[9];
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            p[j] = poses[(size_t)i * 9 + j];
            ok = ok && isfinite((double)p[j]);
        }
        double R[3][3];
        rot6_to_matrix<T>(p, R);
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) rt[CONS_F64 * i + 3 * r + c] = R[r][c];
#pragma unroll
        for (int r = 0; r < 3; ++r) rt[CONS_F64 * i + 9 + r] = (double)p[6 + r];
        fin[i] = ok;
    }
}

// Lanes stride over i; the loop over j is serial and ascending in every lane, which fixes the order of the sums and so the bits.  d_ij is
// bitwise symmetric: the element differences (exact negatives of each other for (i, j) and (j, i)) are squared and summed in one order.
// Writes the float32 scores to e_lds [k][2] and / or e_out [k][2] (either may be NULL).
template <bool SYM>
__device__ __forceinline__ void consensus_score(int k, const double *rt, const int *fin, float *e_lds, float *__restrict__ e_out) {
    for (int i = threadIdx.x; i < k; i += 64) {
        float s0 = -__builtin_inff(), s1 = -__builtin_inff();
        if (fin[i]) {
            double a[CONS_F64];
#pragma unroll
            for (int c = 0; c < CONS_F64; ++c) a[c] = rt[CONS_F64 * i + c];
            double sr = 0.0, st = 0.0;
            int cnt = 0;
            for (int j = 0; j < k; ++j) {
                if (j == i || !fin[j]) continue;
                const double *q = rt + CONS_F64 * j;
                double x;
                if (SYM) {  // the object's y axis: the second column
                    const double d0 = a[1] - q[1], d1 = a[4] - q[4], d2 = a[7] - q[7];
                    x = sqrt((d0 * d0 + d1 * d1) + d2 * d2) / 2.0;
                } else {
                    double ss = 0.0;
#pragma unroll
                    for (int c = 0; c < 9; ++c) {
                        const double d = a[c] - q[c];
                        ss += d * d;
                    }
                    x = sqrt(ss) / 2.8284271247461903;  // 2 sqrt 2
                }
                sr += 2.0 * asin(x < 1.0 ? x : 1.0);
                const double t0 = a[9] - q[9], t1 = a[10] - q[10], t2 = a[11] - q[11];
                st += sqrt((t0 * t0 + t1 * t1) + t2 * t2);
                ++cnt;
            }
            const double den = (double)(cnt > 1 ? cnt : 1);
            s0 = (float)(-(sr / den));
            s1 = (float)(-(st / den));
        }
        if (e_lds) e_lds[2 * i + 0] = s0, e_lds[2 * i + 1] = s1;
        if (e_out) e_out[2 * i + 0] = s0, e_out[2 * i + 1] = s1;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void consensus_energy_kernel(int k, const T *__restrict__ poses, const int8_t *__restrict__ sym,
                                                              float *__restrict__ energy_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *rt = reinterpret_cast<double *>(smem);       // [k][12]
    int *fin = reinterpret_cast<int *>(rt + CONS_F64 * k);  // [k]
    const int b = blockIdx.x;
    consensus_stage<T>(k, poses + (size_t)b * k * 9, rt, fin);
    __syncthreads();
    if (sym && sym[b])
        consensus_score<true>(k, rt, fin, nullptr, energy_out + (size_t)b * k * 2);
    else
        consensus_score<false>(k, rt, fin, nullptr, energy_out + (size_t)b * k * 2);
}

// The score and everything rank_aggregate_kernel does, one launch.  LDS: e [k][2] f32, then the candidates' matrices; once every lane has
// its scores the matrices are dead and ord / quat take their place (8 k + 32 sel <= 40 k bytes of the 100 k).
template <typename T>
__global__ __launch_bounds__(64) void consensus_rank_aggregate_kernel(int k, int sel, const T *__restrict__ poses, const int8_t *__restrict__ sym,
                                                                      float *__restrict__ energy_out, T *__restrict__ sorted_poses,
                                                                      float *__restrict__ sorted_energy, int32_t *__restrict__ order,
                                                                      float *__restrict__ avg_pose, double *__restrict__ sorted_rt,
                                                                      float *__restrict__ avg_rt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *e = reinterpret_cast<float *>(smem);                   // [k][2]
    double *rt = reinterpret_cast<double *>(e + 2 * k);          // [k][12] (offset 8k bytes)
    int *fin = reinterpret_cast<int *>(rt + CONS_F64 * k);        // [k]
    int *ord = reinterpret_cast<int *>(e + 2 * k);                // [k][2], over rt
    double *quat = reinterpret_cast<double *>(ord + 2 * k);  // [sel][4], over rt
    const int b = blockIdx.x;
    poses += (size_t)b * k * 9;
    consensus_stage<T>(k, poses, rt, fin);
    __syncthreads();
    float *eo = energy_out ? energy_out + (size_t)b * k * 2 : nullptr;
    if (sym && sym[b])
        consensus_score<true>(k, rt, fin, e, eo);
    else
        consensus_score<false>(k, rt, fin, e, eo);
    __syncthreads();  // every score is in e, and no lane reads rt / fin any more
    rank_aggregate_cloud<T>(b, k, sel, poses, e, ord, quat, sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
}

// ---------------------------------------------------------------------------------------------- mode-seeking aggregation
// Kernel density over a cloud's candidates and a mean shift from the densest one (ours; include/genpose_hip.h, section D), the rotation
// (column 0) and the translation (column 1) independently.  LDS per candidate: consensus_stage's matrix, translation and flag, and its
// two effective weights: 108 bytes, 55 296 at k = GP_CONSENSUS_MAX_K.  The quaternions are NOT staged (32 bytes more per candidate would
// pass the 64 KB default at k = 512): every mean-shift iteration recomputes them from the matrices.
constexpr size_t MODE_LDS_PER_K = CONS_LDS_PER_K + 2 * sizeof(float);

// consensus_score's distances between two staged poses a and q (the same expressions in the same order: bitwise symmetric)
template <bool SYM>
__device__ __forceinline__ double mode_rot_dist(const double *a, const double *q) {
    double x;
    if (SYM) {
        const double d0 = a[1] - q[1], d1 = a[4] - q[4], d2 = a[7] - q[7];
        x = sqrt((d0 * d0 + d1 * d1) + d2 * d2) / 2.0;
    } else {
        double ss = 0.0;
#pragma unroll
        for (int c = 0; c < 9; ++c) {
            const double d = a[c] - q[c];
            ss += d * d;
        }
        x = sqrt(ss) / 2.8284271247461903;  // 2 sqrt 2
    }
    return 2.0 * asin(x < 1.0 ? x : 1.0);
}

__device__ __forceinline__ double mode_trans_dist(const double *a, const double *q) {
    const double t0 = a[9] - q[9], t1 = a[10] - q[10], t2 = a[11] - q[11];
    return sqrt((t0 * t0 + t1 * t1) + t2 * t2);
}

__device__ __forceinline__ double mode_kernel(double d, double h) { return exp(-(d * d) / (2.0 * h * h)); }

// the sum over the wave, the same bits in every lane (a + b == b + a at every level of the butterfly)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// (w, x, y, z) -> row-major 3x3 in float64 (pytorch3d quaternion_to_matrix: two_s = 2 / |q|^2)
__device__ __forceinline__ void quat_to_matrix(const double q[4], double *o) {
    const double r = q[0], a = q[1], b = q[2], c = q[3];
    const double two_s = 2.0 / (((r * r + a * a) + b * b) + c * c);
    o[0] = 1.0 - two_s * (b * b + c * c), o[1] = two_s * (a * b - c * r), o[2] = two_s * (a * c + b * r);
    o[3] = two_s * (a * b + c * r), o[4] = 1.0 - two_s * (a * a + c * c), o[5] = two_s * (b * c - a * r);
    o[6] = two_s * (a * c - b * r), o[7] = two_s * (b * c + a * r), o[8] = 1.0 - two_s * (a * a + b * b);
}

// row-major 3x3 -> (w, x, y, z) with w >= 0
__device__ __forceinline__ void matrix_to_quat_pos(const double *m9, double q[4]) {
    double R[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) R[r][c] = m9[3 * r + c];
    matrix_to_quat(R, q);
    const double sgn = q[0] < 0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] *= sgn;
}

// One cloud by one wave.  Sums over j that decide a ranking (the density) run serially and ascending in the lane that owns i; sums that
// feed the centre (mean shift, mass, W) are lane partials over j = lane, lane + 64, ... folded by wave_sum - every lane then holds the same
// centre and carries it on redundantly, as rank_aggregate_cloud does with its Jacobi iteration.
template <bool SYM>
__device__ __forceinline__ void mode_cloud(int b, int k, const double *rt, const int *fin, const float *w, double hr, double ht,
                                           int iters, float *__restrict__ density, float *__restrict__ mode_pose, float *__restrict__ mode_rt,
                                           float *__restrict__ mass, int32_t *__restrict__ start) {
    const int tid = threadIdx.x;
    double Wr = 0.0, Wt = 0.0;
    for (int j = tid; j < k; j += 64) Wr += (double)w[2 * j], Wt += (double)w[2 * j + 1];
    Wr = wave_sum(Wr), Wt = wave_sum(Wt);
    // density, and the lane's best candidate per column (strict >: the lowest index of a lane's ascending i wins its ties)
    double best_r = -1.0, best_t = -1.0;
    int ir = -1, it = -1;
    for (int i = tid; i < k; i += 64) {
        double d0 = -__builtin_inf(), d1 = -__builtin_inf();
        if (fin[i]) {
            double a[CONS_F64];
#pragma unroll
            for (int c = 0; c < CONS_F64; ++c) a[c] = rt[CONS_F64 * i + c];
            double sr = 0.0, st = 0.0;
            for (int j = 0; j < k; ++j) {
                const double wr = (double)w[2 * j], wt = (double)w[2 * j + 1];
                if (wr == 0.0 && wt == 0.0) continue;  // (every non-finite j is here)
                const double *q = rt + CONS_F64 * j;
                if (wr > 0.0) sr += wr * mode_kernel(mode_rot_dist<SYM>(a, q), hr);
                if (wt > 0.0) st += wt * mode_kernel(mode_trans_dist(a, q), ht);
            }
            d0 = Wr > 0.0 ? sr / Wr : 0.0;
            d1 = Wt > 0.0 ? st / Wt : 0.0;
            if (w[2 * i] > 0.f && d0 > best_r) best_r = d0, ir = i;
            if (w[2 * i + 1] > 0.f && d1 > best_t) best_t = d1, it = i;
        }
        if (density) density[((size_t)b * k + i) * 2 + 0] = (float)d0, density[((size_t)b * k + i) * 2 + 1] = (float)d1;
    }
    // start: the highest float64 density among the weighted candidates, the lowest index among equals
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double o_r = __shfl_xor(best_r, m, 64), o_t = __shfl_xor(best_t, m, 64);
        const int j_r = __shfl_xor(ir, m, 64), j_t = __shfl_xor(it, m, 64);
        if (j_r >= 0 && (ir < 0 || o_r > best_r || (o_r == best_r && j_r < ir))) best_r = o_r, ir = j_r;
        if (j_t >= 0 && (it < 0 || o_t > best_t || (o_t == best_t && j_t < it))) best_t = o_t, it = j_t;
    }
    if (start && tid == 0) start[(size_t)b * 2 + 0] = ir, start[(size_t)b * 2 + 1] = it;
    if (!mode_pose && !mode_rt && !mass) return;
    // the centre in consensus_stage's layout: [0..8] the rotation (SYM: only the y axis, [1], [4], [7], is read), [9..11] the translation
    double cen[CONS_F64] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0}, qc[4] = {1, 0, 0, 0};
    if (ir >= 0) {
#pragma unroll
        for (int c = 0; c < 9; ++c) cen[c] = rt[CONS_F64 * ir + c];
        matrix_to_quat_pos(cen, qc);
    }
    if (it >= 0) {
#pragma unroll
        for (int c = 9; c < 12; ++c) cen[c] = rt[CONS_F64 * it + c];
    }
    double mr = 0.0, mt = 0.0;
    for (int step = 0; step <= iters; ++step) {  // `iters` shifts, then one more pass for the mass at the final centre
        double acc[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, ta[3] = {0, 0, 0}, sur = 0.0, sut = 0.0;
        for (int j = tid; j < k; j += 64) {
            const double wr = (double)w[2 * j], wt = (double)w[2 * j + 1];
            if (wr == 0.0 && wt == 0.0) continue;
            const double *q = rt + CONS_F64 * j;
            if (wr > 0.0) {
                const double u = wr * mode_kernel(mode_rot_dist<SYM>(cen, q), hr);
                sur += u;
                if (SYM) {
                    acc[0] += u * q[1], acc[1] += u * q[4], acc[2] += u * q[7];
                } else if (step < iters) {
                    double qj[4];
                    matrix_to_quat_pos(q, qj);
                    acc[0] += u * (qj[0] * qj[0]), acc[1] += u * (qj[0] * qj[1]), acc[2] += u * (qj[0] * qj[2]), acc[3] += u * (qj[0] * qj[3]);
                    acc[4] += u * (qj[1] * qj[1]), acc[5] += u * (qj[1] * qj[2]), acc[6] += u * (qj[1] * qj[3]);
                    acc[7] += u * (qj[2] * qj[2]), acc[8] += u * (qj[2] * qj[3]), acc[9] += u * (qj[3] * qj[3]);
                }
            }
            if (wt > 0.0) {
                const double u = wt * mode_kernel(mode_trans_dist(cen, q), ht);
                sut += u;
                ta[0] += u * q[9], ta[1] += u * q[10], ta[2] += u * q[11];
            }
        }
        sur = wave_sum(sur), sut = wave_sum(sut);
        if (step == iters) {
            mr = Wr > 0.0 ? sur / Wr : 0.0;
            mt = Wt > 0.0 ? sut / Wt : 0.0;
            break;
        }
#pragma unroll
        for (int c = 0; c < (SYM ? 3 : 10); ++c) acc[c] = wave_sum(acc[c]);
#pragma unroll
        for (int c = 0; c < 3; ++c) ta[c] = wave_sum(ta[c]);
        if (sut > 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) cen[9 + c] = ta[c] / sut;
        }
        if (sur > 0.0) {
            if (SYM) {
                const double n = sqrt((acc[0] * acc[0] + acc[1] * acc[1]) + acc[2] * acc[2]);
                if (n >= 1e-12) cen[1] = acc[0] / n, cen[4] = acc[1] / n, cen[7] = acc[2] / n;
            } else {
                double A[4][4] = {{acc[0] / sur, acc[1] / sur, acc[2] / sur, acc[3] / sur},
                                  {acc[1] / sur, acc[4] / sur, acc[5] / sur, acc[6] / sur},
                                  {acc[2] / sur, acc[5] / sur, acc[7] / sur, acc[8] / sur},
                                  {acc[3] / sur, acc[6] / sur, acc[8] / sur, acc[9] / sur}};
                double v[4];
                top_eigvec4(A, v);
                const double sgn = v[0] < 0 ? -1.0 : 1.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) qc[i] = sgn * v[i];
                quat_to_matrix(qc, cen);
            }
        }
    }
    if (SYM && iters > 0 && ir >= 0) {
        // the start candidate's R turned by the minimal rotation that takes its y axis ys onto the centre's y:
        // M = I + [v]x + [v]x^2 / (1 + c), v = ys x y, c = ys . y; opposite axes (1 + c < 1e-12): the half turn about R's x axis
        const double *Rs = rt + CONS_F64 * ir;
        const double ys[3] = {Rs[1], Rs[4], Rs[7]}, y[3] = {cen[1], cen[4], cen[7]};
        const double v[3] = {ys[1] * y[2] - ys[2] * y[1], ys[2] * y[0] - ys[0] * y[2], ys[0] * y[1] - ys[1] * y[0]};
        const double c1 = 1.0 + ((ys[0] * y[0] + ys[1] * y[1]) + ys[2] * y[2]);
        double M[9];
        if (c1 < 1e-12) {
            const double x[3] = {Rs[0], Rs[3], Rs[6]};
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) M[3 * r + c] = 2.0 * x[r] * x[c] - (r == c ? 1.0 : 0.0);
        } else {
            const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) M[3 * r + c] = (v[r] * v[c] - (r == c ? vv : 0.0)) / c1 + (r == c ? 1.0 : 0.0);  // I + [v]x^2 / (1 + c)
            M[1] -= v[2], M[2] += v[1], M[3] += v[2], M[5] -= v[0], M[6] -= v[1], M[7] += v[0];                        // + [v]x
        }
        double R[9];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) R[3 * r + c] = (M[3 * r] * Rs[c] + M[3 * r + 1] * Rs[3 + c]) + M[3 * r + 2] * Rs[6 + c];
        matrix_to_quat_pos(R, qc);
    }
    if (tid == 0) {
        float qt[7];
#pragma unroll
        for (int i = 0; i < 4; ++i) qt[i] = (float)qc[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) qt[4 + i] = (float)cen[9 + i];
        if (mode_pose) {
#pragma unroll
            for (int i = 0; i < 7; ++i) mode_pose[(size_t)b * 7 + i] = qt[i];
        }
        if (mode_rt) quat_trans_to_rt(qt, mode_rt + (size_t)b * 16);
        if (mass) mass[(size_t)b * 2 + 0] = (float)mr, mass[(size_t)b * 2 + 1] = (float)mt;
    }
}

template <typename T>
__global__ __launch_bounds__(64) void mode_aggregate_kernel(int k, const T *__restrict__ poses, const int8_t *__restrict__ sym,
                                                            const float *__restrict__ weight, double hr, double ht, int iters,
                                                            float *__restrict__ density, float *__restrict__ mode_pose,
                                                            float *__restrict__ mode_rt, float *__restrict__ mass, int32_t *__restrict__ start) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *rt = reinterpret_cast<double *>(smem);          // [k][12]
    float *w = reinterpret_cast<float *>(rt + CONS_F64 * k);  // [k][2] effective weights
    int *fin = reinterpret_cast<int *>(w + 2 * k);          // [k]
    const int b = blockIdx.x;
    consensus_stage<T>(k, poses + (size_t)b * k * 9, rt, fin);
    for (int i = threadIdx.x; i < k; i += 64) {  // (the lane that staged candidate i reads its own flag)
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float wi = weight ? weight[((size_t)b * k + i) * 2 + c] : 1.f;
            w[2 * i + c] = (fin[i] && wi > 0.f) ? wi : 0.f;
        }
    }
    __syncthreads();
    if (sym && sym[b])
        mode_cloud<true>(b, k, rt, fin, w, hr, ht, iters, density, mode_pose, mode_rt, mass, start);
    else
        mode_cloud<false>(b, k, rt, fin, w, hr, ht, iters, density, mode_pose, mode_rt, mass, start);
}

}  // namespace

// [n][9] poses (two rotation columns + translation) -> [n][4][4] f64 homogeneous matrices (evaluation_single.py:325-332: get_rot_matrix
// on float64 rows, translation in the last column)
template <typename T>
__global__ void pose9_to_rt_kernel(int n, const T *__restrict__ pose, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double R[3][3];
    rot6_to_matrix<T>(pose + (size_t)i * 9, R);
    double *o = out + (size_t)i * 16;
    for (int r = 0; r < 3; ++r) {
        o[4 * r + 0] = R[r][0], o[4 * r + 1] = R[r][1], o[4 * r + 2] = R[r][2];
        o[4 * r + 3] = (double)pose[(size_t)i * 9 + 6 + r];
    }
    o[12] = o[13] = o[14] = 0.0, o[15] = 1.0;
}

// [n][7] (w, x, y, z, t) f32 -> [n][4][4] f32 (quat_trans_to_rt above)
__global__ void quat_trans_to_rt_kernel(int n, const float *__restrict__ qt, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    quat_trans_to_rt(qt + (size_t)i * 7, out + (size_t)i * 16);
}

extern "C" {

int gp_pose9_to_rt(int n, int is_f64, const void *pose, double *out, gp_stream_t s) {
    if (n < 0 || !pose || !out) return GP_EINVAL;
    if (n == 0) return GP_OK;
    if (is_f64)
        hipLaunchKernelGGL(pose9_to_rt_kernel<double>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, n, (const double *)pose, out);
    else
        hipLaunchKernelGGL(pose9_to_rt_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, n, (const float *)pose, out);
    return gp_launch_status();
}

int gp_quat_trans_to_rt(int n, const float *quat_trans, float *out, gp_stream_t s) {
    if (n < 0 || !quat_trans || !out) return GP_EINVAL;
    if (n == 0) return GP_OK;
    hipLaunchKernelGGL(quat_trans_to_rt_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)s, n, quat_trans, out);
    return gp_launch_status();
}

int gp_rank_aggregate_rt(int b, int k, int sel, int is_f64, const void *poses, const float *energy, void *sorted_poses, float *sorted_energy,
                         int32_t *order, float *avg_pose, double *sorted_rt, float *avg_rt, gp_stream_t s) {
    if (b < 0 || k <= 0 || k > GP_RANK_MAX_K || !poses || !energy) return GP_EINVAL;
    if (avg_pose && (sel <= 0 || sel > k)) return GP_EINVAL;
    if (avg_rt && !avg_pose) return GP_EINVAL;
    if (b == 0) return GP_OK;
    const size_t lds = (size_t)k * 16 + 16 + (size_t)(avg_pose ? sel : 0) * 32;
    // sel = k >= 1366 is above the 64 KB default.  Both kernels get the LARGEST request this entry point serves, whatever this call's own
    // size and dtype: the first call - a runner's warm-up, outside any stream capture - then covers every later one.
    constexpr size_t lds_max = (size_t)GP_RANK_MAX_K * (16 + 32) + 16;
    static_assert(lds_max <= 160 * 1024, "the largest ranking must fit the CU's LDS");
    if (gp_prepare_lds<rank_aggregate_kernel<float>, rank_aggregate_kernel<double>>(lds_max)) return GP_ELAUNCH;
    if (is_f64)
        hipLaunchKernelGGL(rank_aggregate_kernel<double>, dim3(b), dim3(64), lds, (hipStream_t)s, k, sel, (const double *)poses, energy,
                           (double *)sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
    else
        hipLaunchKernelGGL(rank_aggregate_kernel<float>, dim3(b), dim3(64), lds, (hipStream_t)s, k, sel, (const float *)poses, energy,
                           (float *)sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
    return gp_launch_status();
}

int gp_rank_aggregate(int b, int k, int sel, int is_f64, const void *poses, const float *energy, void *sorted_poses, float *sorted_energy,
                      int32_t *order, float *avg_pose, gp_stream_t s) {
    return gp_rank_aggregate_rt(b, k, sel, is_f64, poses, energy, sorted_poses, sorted_energy, order, avg_pose, nullptr, nullptr, s);
}

int gp_consensus_energy(int b, int k, int is_f64, const void *poses, const int8_t *sym, float *energy_out, gp_stream_t s) {
    if (b < 0 || k <= 0 || k > GP_CONSENSUS_MAX_K || !poses || !energy_out) return GP_EINVAL;
    if (b == 0) return GP_OK;
    const size_t lds = (size_t)k * CONS_LDS_PER_K;
    if (is_f64)
        hipLaunchKernelGGL(consensus_energy_kernel<double>, dim3(b), dim3(64), lds, (hipStream_t)s, k, (const double *)poses, sym, energy_out);
    else
        hipLaunchKernelGGL(consensus_energy_kernel<float>, dim3(b), dim3(64), lds, (hipStream_t)s, k, (const float *)poses, sym, energy_out);
    return gp_launch_status();
}

int gp_consensus_rank_aggregate_rt(int b, int k, int sel, int is_f64, const void *poses, const int8_t *sym, float *energy_out, void *sorted_poses,
                                   float *sorted_energy, int32_t *order, float *avg_pose, double *sorted_rt, float *avg_rt, gp_stream_t s) {
    if (b < 0 || k <= 0 || k > GP_CONSENSUS_MAX_K || !poses) return GP_EINVAL;
    if (avg_pose && (sel <= 0 || sel > k)) return GP_EINVAL;
    if (avg_rt && !avg_pose) return GP_EINVAL;
    if (b == 0) return GP_OK;
    const size_t lds = (size_t)k * (8 + CONS_LDS_PER_K);  // at most 108 * GP_CONSENSUS_MAX_K = 55 296 bytes: below the 64 KB default
    if (is_f64)
        hipLaunchKernelGGL(consensus_rank_aggregate_kernel<double>, dim3(b), dim3(64), lds, (hipStream_t)s, k, sel, (const double *)poses, sym,
                           energy_out, (double *)sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
    else
        hipLaunchKernelGGL(consensus_rank_aggregate_kernel<float>, dim3(b), dim3(64), lds, (hipStream_t)s, k, sel, (const float *)poses, sym,
                           energy_out, (float *)sorted_poses, sorted_energy, order, avg_pose, sorted_rt, avg_rt);
    return gp_launch_status();
}

int gp_mode_aggregate(int b, int k, int is_f64, const void *poses, const int8_t *sym, const float *weight, double bw_rot, double bw_trans,
                      int iters, float *density, float *mode_pose, float *mode_rt, float *mass, int32_t *start, gp_stream_t s) {
    if (b < 0 || k <= 0 || k > GP_CONSENSUS_MAX_K || !poses || iters < 0 || iters > GP_MODE_MAX_ITERS) return GP_EINVAL;
    if (!(bw_rot > 0.0 && bw_rot < __builtin_huge_val()) || !(bw_trans > 0.0 && bw_trans < __builtin_huge_val())) return GP_EINVAL;  // (NaN fails both)
    if (b == 0) return GP_OK;
    const size_t lds = (size_t)k * MODE_LDS_PER_K;  // at most 108 * GP_CONSENSUS_MAX_K = 55 296 bytes: below the 64 KB default
    if (is_f64)
        hipLaunchKernelGGL(mode_aggregate_kernel<double>, dim3(b), dim3(64), lds, (hipStream_t)s, k, (const double *)poses, sym, weight, bw_rot,
                           bw_trans, iters, density, mode_pose, mode_rt, mass, start);
    else
        hipLaunchKernelGGL(mode_aggregate_kernel<float>, dim3(b), dim3(64), lds, (hipStream_t)s, k, (const float *)poses, sym, weight, bw_rot,
                           bw_trans, iters, density, mode_pose, mode_rt, mass, start);
    return gp_launch_status();
}

}  // extern "C"
