// What the two split-bf16 set-abstraction kernels (sa_bf16x3.hip: hi / lo, sa_bf16x9.hip: hi / mid / lo) share around their dense layers:
// the fp32 operands staged in LDS, the schedule of 32-row units over the persistent waves with its index and coordinate prefetch, layer 1 on
// the fp32 VALU for one k-block, and the pooled bias + ReLU + store.  A = the kernel's argument block (n, np, zstride, zoff, xyz, new_xyz,
// z, idx, wxyz, b1, b2, b3, out, cout_total, cout_off).  Rings, accumulator layouts, the buffering of the hoisted feature rows and the
// launchers stay with each kernel; the prefetched indices and coordinates live in the caller's locals.
#pragma once
#include "gp_common.h"

namespace gp_sa_rows {

// layer-1 rows (wx, wy, wz, b1) and the two biases -> LDS, by NTH threads
template <int C1, int KB2, int C3, int NTH, class A>
__device__ __forceinline__ void stage_operands(const A &a, f32x4 *w1l, float *b2l, float *b3l, int tid) {
    for (int e = tid; e < C1; e += NTH) {
        f32x4 w = *reinterpret_cast<const f32x4 *>(a.wxyz + e * 4);
        w.w = a.b1[e];
        w1l[e] = w;
    }
    for (int e = tid; e < 32 * KB2; e += NTH) b2l[e] = a.b2[e];
    for (int e = tid; e < C3; e += NTH) b3l[e] = a.b3[e];
}

// Unit `it` of a wave: 32 consecutive (centre, sample) rows = sub-chunks s = 0, 1 of 16 rows (one neighbourhood of NS = 32 or two of 16),
// dealt round-robin over all waves of the grid; iterations past the wave's last unit compute on unit 0 and store nothing.
template <int NS>
struct Units {
    int wave_global, nwaves, my_units;
    __device__ __forceinline__ Units(int nunits_total, int nwv, int tid)
        : wave_global(blockIdx.x * nwv + __builtin_amdgcn_readfirstlane(tid >> 6)), nwaves(gridDim.x * nwv),  // (scalar, as in the fp32 chain kernels)
          my_units(wave_global < nunits_total ? (nunits_total - wave_global + nwaves - 1) / nwaves : 0) {}
    __device__ __forceinline__ int unit_of(int it) const { return it < my_units ? wave_global + it * nwaves : 0; }
    __device__ __forceinline__ int centre_of(int it, int s) const { return (unit_of(it) * 32 + 16 * s) / NS; }
    // iterations of the longest wave: with a ring every wave runs this many, so that the barrier counts match
    __device__ __forceinline__ int nits_all(int nunits_total) const { return (nunits_total + nwaves - 1) / nwaves; }

    template <class A>
    __device__ __forceinline__ void load_idx(const A &a, int it, int pt, int (&j)[2]) const {
        const size_t r0 = (size_t)unit_of(it) * 32;
#pragma unroll
        for (int s = 0; s < 2; ++s) j[s] = a.idx[r0 + 16 * s + pt];
    }
    template <class A>
    __device__ __forceinline__ void load_d(const A &a, int it, const int (&j)[2], float (&d)[2][3]) const {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int cc = centre_of(it, s), bcl = cc / a.np;
            const float *xyz = a.xyz + (size_t)bcl * a.n * 3;
            const float *cp = a.new_xyz + (size_t)cc * 3;
            d[s][0] = xyz[j[s] * 3 + 0] - cp[0];  // grouped_xyz -= new_xyz (pointnet2_utils.py:253)
            d[s][1] = xyz[j[s] * 3 + 1] - cp[1];
            d[s][2] = xyz[j[s] * 3 + 2] - cp[2];
        }
    }
    // the hoisted feature rows of the unit's two points, at this lane group's four channels
    template <class A>
    __device__ __forceinline__ void z_rows(const A &a, int it, const int (&j)[2], int g4, const float *(&zrow)[2]) const {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int bcl = centre_of(it, s) / a.np;
            zrow[s] = a.z + ((size_t)bcl * a.n + j[s]) * a.zstride + a.zoff + g4;
        }
    }
    // The two-deep prefetch behind layers 1 + 2: the next unit's indices were requested an iteration ago - its coordinates now, the
    // indices of the one after.
    template <class A>
    __device__ __forceinline__ void advance(const A &a, int it, int pt, int (&jcur)[2], int (&jn)[2], float (&dcur)[2][3]) const {
        load_d(a, it + 1, jn, dcur);
        jcur[0] = jn[0], jcur[1] = jn[1];
        load_idx(a, it + 2, pt, jn);
    }
};

// Layer 1 of one point for k-block kb (chunks 2 kb, 2 kb + 1): hoisted feature half zz + W_xyz . d + b1, ReLU - the fp32 kernels' arithmetic
__device__ __forceinline__ void layer1(const f32x4 *w1l, const f32x4 (&zz)[2], const float (&d)[3], int kb, int g4, f32x4 (&h)[2]) {
    const float dx = d[0], dy = d[1], dz = d[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int q = 2 * kb + c;
        const f32x4 r0 = w1l[16 * q + g4 + 0], r1 = w1l[16 * q + g4 + 1], r2 = w1l[16 * q + g4 + 2], r3 = w1l[16 * q + g4 + 3];
        f32x4 v = zz[c];
        v.x += (r0.x * dx + r0.y * dy + r0.z * dz) + r0.w;
        v.y += (r1.x * dx + r1.y * dy + r1.z * dz) + r1.w;
        v.z += (r2.x * dx + r2.y * dy + r2.z * dz) + r2.w;
        v.w += (r3.x * dx + r3.y * dy + r3.z * dz) + r3.w;
        h[c] = relu4(v);
    }
}

// Pooling over the points of one transposed output chunk (lane = channel ch; acc0 / acc1 = the two sub-chunks): max_i relu(x_i + b) =
// relu(max_i x_i + b), so bias and ReLU once per channel, after the pooling; lane group 0 stores, one row (NS = 32) or two (NS = 16).
template <int NS, class A>
__device__ __forceinline__ void pooled_store(const A &a, const float *b3l, const f32x4 &acc0, const f32x4 &acc1, int ch, int unit, bool store) {
    const float m0 = points16_max_t(acc0), m1 = points16_max_t(acc1);
    const float b = b3l[ch];
    if (store) {
        if (NS == 32) {
            a.out[(size_t)unit * a.cout_total + a.cout_off + ch] = fmaxf(fmaxf(m0, m1) + b, 0.f);
        } else {
            a.out[(size_t)(2 * unit) * a.cout_total + a.cout_off + ch] = fmaxf(m0 + b, 0.f);
            a.out[(size_t)(2 * unit + 1) * a.cout_total + a.cout_off + ch] = fmaxf(m1 + b, 0.f);
        }
    }
}

}  // namespace gp_sa_rows
