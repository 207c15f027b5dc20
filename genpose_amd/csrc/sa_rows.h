// What the set-abstraction chain kernels share around their dense layers: the fp32 operands staged in LDS, layer 1 on the fp32 VALU, the
// schedules of rows over the persistent waves with their index and coordinate prefetch, the fp32 ring's fragment-group step and the pooled
// bias + ReLU + store.  Users: the fp32 kernels of sa_mlp.hip (16-row Chunks) and the two split-bf16 kernels (sa_bf16x3.hip: hi / lo,
// sa_bf16x9.hip: hi / mid / lo; 32-row Units).  A = the kernel's argument block (n, np, zstride, zoff, xyz, new_xyz, z, idx, wxyz, b1, b2,
// b3, out, cout_total, cout_off).  Rings, accumulator layouts, the buffering of the hoisted feature rows and the launchers stay with each
// kernel; the prefetched indices and coordinates live in the caller's locals.
#pragma once
#include <initializer_list>

#include "gp_common.h"

namespace gp_sa_rows {

// Host side: what the per-scale entry points of the three split-bf16 kernels require of their arguments before their own shape check -
// every pointer present (`ptrs`: the kernel's operands), output and z columns float4-aligned and inside their rows, whole 32-row units
// with row indices that fit an int.
inline bool units_args_ok(int b, int n, int np, int ns, int c1, int c3, int zstride, int zoff, int cout_total, int cout_off,
                          std::initializer_list<const void *> ptrs) {
    if (b < 0 || n <= 0 || np <= 0) return false;
    for (const void *p : ptrs)
        if (!p) return false;
    if ((cout_total & 3) || (cout_off & 3) || cout_off < 0 || cout_off + c3 > cout_total || (zstride & 3) || (zoff & 3) || zoff < 0 || zoff + c1 > zstride)
        return false;
    return !(((size_t)b * np * ns) % 32 || ((size_t)b * np * ns) / 32 > 0x3ffffffu);
}

// layer-1 rows (wx, wy, wz, b1), NB2 floats of the layer-2 bias and NB3 of the layer-3 bias -> LDS, by NTH threads (a count of 0: that bias
// stays in the kernel's registers)
template <int C1, int NB2, int NB3, int NTH, class A>
__device__ __forceinline__ void stage_operands(const A &a, f32x4 *w1l, float *b2l, float *b3l, int tid) {
    for (int e = tid; e < C1; e += NTH) {
        f32x4 w = *reinterpret_cast<const f32x4 *>(a.wxyz + e * 4);
        w.w = a.b1[e];
        w1l[e] = w;
    }
    for (int e = tid; e < NB2; e += NTH) b2l[e] = a.b2[e];
    for (int e = tid; e < NB3; e += NTH) b3l[e] = a.b3[e];
}

// Layer 1 = hoisted feature half z + W_xyz . d + b1, ReLU.  The xyz half of a channel (row r = (wx, wy, wz, .)) is xyz_dot():
// (wx dx + wy dy) + wz dz everywhere; the three terms are then summed in one of three orders, each a bit-exactness contract of its kernels:
//   (b1 + z) + dot   the tile kernel sa_pre_mlp_kernel (b1 from global memory, z only where the level has input features)
//   b1 + dot         sa0_chain_kernel (level 0: no z)
//   z + (dot + b1)   layer1() below: sa_chain_lds, sa_chain_ring, sa_groupall_ring and the two split-bf16 kernels (b1 = the staged row's .w)
__device__ __forceinline__ float xyz_dot(const f32x4 &r, float dx, float dy, float dz) { return r.x * dx + r.y * dy + r.z * dz; }
// the chain form for one point and the lane group's four channels 16 q + g4 + 0..3 of chunk q, from the staged rows
__device__ __forceinline__ f32x4 layer1(const f32x4 *w1l, int q, int g4, const f32x4 &z, float dx, float dy, float dz) {
    const f32x4 r0 = w1l[16 * q + g4 + 0], r1 = w1l[16 * q + g4 + 1], r2 = w1l[16 * q + g4 + 2], r3 = w1l[16 * q + g4 + 3];
    f32x4 v = z;
    v.x += xyz_dot(r0, dx, dy, dz) + r0.w;
    v.y += xyz_dot(r1, dx, dy, dz) + r1.w;
    v.z += xyz_dot(r2, dx, dy, dz) + r2.w;
    v.w += xyz_dot(r3, dx, dy, dz) + r3.w;
    return relu4(v);
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

// The fp32 chain kernels' schedule: a wave walks 16-row chunks, iteration `it` = chunk it % PT of its (it / PT)-th neighbourhood, the
// neighbourhoods dealt round-robin over all waves of the grid - so the register footprint of an iteration is one chunk whatever the
// neighbourhood size.  SPLITP: the chunks themselves are dealt out (iteration it = the wave's it-th chunk).  `wave_in_wg` is the caller's:
// scalar (readfirstlane) keeps the centre index and everything addressed through it on the scalar unit; sa_chain_ring at NS = 16 passes
// the vector form (measured there, see the kernel).  Iterations past the wave's last (it >= nits) load clamped rows and store nothing.
template <int NS, bool SPLITP = false>
struct Chunks {
    static constexpr int PT = NS / 16;
    int wave_global, nwaves, nits;
    __device__ __forceinline__ Chunks(int ncentres_total, int nwv, int wave_in_wg) : wave_global(blockIdx.x * nwv + wave_in_wg), nwaves(gridDim.x * nwv) {
        const int nunits = nunits_of(ncentres_total);  // what the waves share out: chunks or whole neighbourhoods
        const int my_units = wave_global < nunits ? (nunits - wave_global + nwaves - 1) / nwaves : 0;
        nits = SPLITP ? my_units : my_units * PT;
    }
    __device__ __forceinline__ static int nunits_of(int ncentres_total) { return SPLITP ? ncentres_total * PT : ncentres_total; }
    // iterations of the longest wave: with a ring every wave runs this many, so that the barrier counts match
    __device__ __forceinline__ int nits_all(int ncentres_total) const { return ((nunits_of(ncentres_total) + nwaves - 1) / nwaves) * (SPLITP ? 1 : PT); }
    // first (centre, sample) row of chunk `it` and its centre c
    __device__ __forceinline__ size_t chunk_row0(int it, int &c) const {
        if constexpr (SPLITP) {
            const int u = wave_global + it * nwaves;
            c = u / PT;
            return (size_t)c * NS + (size_t)(u % PT) * 16;
        }
        c = wave_global + (it / PT) * nwaves;
        return (size_t)c * NS + (size_t)(it % PT) * 16;
    }
    __device__ __forceinline__ int centre_of(int it) const {
        int c;
        chunk_row0(it, c);
        return it < nits ? c : 0;
    }
    template <class A>
    __device__ __forceinline__ int load_idx(const A &a, int it, int pt) const {
        int c;
        const size_t r0 = chunk_row0(it, c);
        return it < nits ? a.idx[r0 + pt] : 0;
    }
    // operands of one chunk: xyz deltas and the gathered rows of Z (lane group g's channels 16 q + 4 g + 0..3)
    template <int Q1, class A>
    __device__ __forceinline__ void load_ops(const A &a, int it, int j, int g, float (&d)[3], f32x4 (&zz)[Q1]) const {
        const int cc = centre_of(it), bcl = cc / a.np;
        const float *xyz = a.xyz + (size_t)bcl * a.n * 3;
        const float *zb = a.z + (size_t)bcl * a.n * a.zstride + a.zoff;
        const float *cp = a.new_xyz + (size_t)cc * 3;
        d[0] = xyz[j * 3 + 0] - cp[0];  // grouped_xyz -= new_xyz (pointnet2_utils.py:253)
        d[1] = xyz[j * 3 + 1] - cp[1];
        d[2] = xyz[j * 3 + 2] - cp[2];
#pragma unroll
        for (int q = 0; q < Q1; ++q) zz[q] = *reinterpret_cast<const f32x4 *>(zb + (size_t)j * a.zstride + 16 * q + 4 * g);
    }
};

// One fragment group of an fp32 ring step: the four fragments requested a group ago (wpre) multiply k-steps jj < njj of activation fragment
// h into four accumulators while the next four (`next`: the following group of this slot, or the first group of the next slot) are requested.
// TRANSPOSED: activations as the A operand (lane = channel).  Users: layers 2 and 3 of sa_groupall_ring_kernel; sa_chain_ring_kernel's layer 3
// keeps the same block written out (measured, see there).
template <bool TRANSPOSED>
__device__ __forceinline__ void ring_group(f32x4 (&wpre)[4], const f32x4 *next, int lo, const f32x4 &h, int njj, f32x4 *acc) {
    f32x4 wf[4], wn[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) wf[u] = wpre[u];
#pragma unroll
    for (int u = 0; u < 4; ++u) wn[u] = next[u * 64 + lo];
#pragma unroll
    for (int jj = 0; jj < njj; ++jj)
#pragma unroll
        for (int u = 0; u < 4; ++u)
            acc[u] = TRANSPOSED ? __builtin_amdgcn_mfma_f32_16x16x4f32(h[jj], wf[u][jj], acc[u], 0, 0, 0)
                                : __builtin_amdgcn_mfma_f32_16x16x4f32(wf[u][jj], h[jj], acc[u], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < 4; ++u) wpre[u] = wn[u];
}

// Whole-neighbourhood pooling of the fp32 chain kernels (last layer transposed: lane = channel 16 n + pt, res[n] = the running max of the
// PRE-bias output over the neighbourhood's rows): max_i relu(x_i + b) = relu(max_i x_i + b), so bias and ReLU come once per channel,
// after the pooling (exact: rounding is monotone); lane group 0 stores.  bias(n) = this lane's bias of chunk n.
template <int Q3, class Bias>
__device__ __forceinline__ void pooled_store_chunks(float *o, const float (&res)[Q3], Bias bias, int pt, bool store) {
#pragma unroll
    for (int n = 0; n < Q3; ++n)
        if (store) o[16 * n + pt] = fmaxf(res[n] + bias(n), 0.f);
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
