// Grouping level 1 of the light / dense encoders (hoisted first layer -> 64 -> 64 | 96 -> 128 -> max over the neighbourhood) with the two dense
// layers as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h: every fp32 operand is hi + mid + lo; SIX of the nine cross products
// are formed as the project builds it, NPROD = SA_NPROD = GP_SA_X9_PRODUCTS = 6 - all but lo.lo, lo.mid and mid.lo, together at most
// (2^-23 + 2^-32) |a b| per multiply, below the fp32 accumulation's own rounding; 8 and 9 are measurement builds - each
// exact in fp32, and only the fp32 accumulation rounds) - the error class of sa_chain_lds_kernel<C1, C2, C3, NS> (sa_mlp.hip), whose job, inputs and
// [B, np, C3] output columns per scale this kernel takes over (Pointnet2EncoderHIP(level1 = 'bf16x9'); the fp32 kernel stays the default of the
// class).  Furthest point sampling and the ball queries see coordinates only: centres and neighbourhoods are bit-identical either way.
//
// Form: sa_bf16x3.hip's without the ring (the row front and back end is sa_rows.h's, the products are bf16x9.h's) - the level is small enough
// that BOTH layers' weights stay LDS-resident as hi / mid / lo (64-64-128: 24 + 48 KB, 64-96-128: 36 + 72 KB), copied once per workgroup
// before ONE __syncthreads(); the persistent loop over 32-row units has no barrier, so the waves of a SIMD drift apart and fill each other's
// gaps.  32 rows per wave and iteration (one neighbourhood of 32 or two of 16): every weight fragment read from LDS feeds two B tiles =
// 16 MFMAs.  Activations stay in registers from the gather to the pooled output; layer 1 on the fp32 VALU with the fp32 kernel's arithmetic,
// z + (dot + b1); the D fragment of a layer IS the next layer's operand (two chunks = one k-block, weights.py: pack_bf16x9's k order); layer
// 3 transposed (activations as the A operand, lane = channel), max over the points before bias + ReLU.  The hoisted feature rows of k-block
// kb + 1 are requested while kb is multiplied, those of the NEXT unit's first k-block while layer 3 is.
// C2 = 64 | 96 and C3 = 128 are whole chunks and whole k-blocks: no padding anywhere, no skipped or zero MFMAs.
// Budget per 32-row unit (MI355X: v_mfma_f32_16x16x32_bf16 16 cycles): (KB1 NC2 + KB2 8) x 16 MFMAs = 384 (64-64-128) | 576 (64-96-128)
// = 6.1 k | 9.2 k cycles (all nine products: 432 | 648 = 6.9 k | 10.4 k); LDS fragment reads 3 KB per 16 MFMAs and wave: 8-12 waves x
// 3 KB / 128 B/clk = 190-290 cycles beside 2-3 x 256 cycles of MFMA per SIMD - the matrix pipe bounds it.
#include "bf16x9.h"
#include "sa_rows.h"

namespace {

using namespace gp_bf16x9;

struct SALX9Args {
    int n, np, zstride, zoff;
    const float *xyz, *new_xyz, *z;
    const int32_t *idx;
    const float *wxyz, *b1;  // layer 1 stays on the fp32 VALU (three FMAs per channel on top of the hoisted feature half)
    const bf16x8 *w2;        // [KB1][NC2][3 = hi, mid, lo][64 lanes] (weights.py: pack_bf16x9(W2, NC2, KB1))
    const float *b2;         // [C2]
    const bf16x8 *w3;        // [KB2][C3 / 16][3][64 lanes] (pack_bf16x9(W3, C3 / 16, KB2))
    const float *b3;         // [C3]
    float *out;
    int cout_total, cout_off;
};

template <int C1, int C2, int C3>
struct SALX9Geom {
    static constexpr int KB1 = C1 / 32, NC2 = C2 / 16, KB2 = C2 / 32, NC3 = C3 / 16;
    static constexpr int W2N = KB1 * NC2 * 3 * 64, W3N = KB2 * NC3 * 3 * 64;  // bf16x8 (16 B) each
    static constexpr size_t LDS = (size_t)(W2N + W3N + C1) * 16 + (size_t)(C2 + C3) * sizeof(float);
    static_assert(C1 % 32 == 0 && C2 % 32 == 0 && C3 == 128, "whole k-blocks, layer 3 as one group of eight output chunks");
    static_assert(LDS <= 160 * 1024, "both layers LDS-resident as three terms");
};

// the three terms of output chunk `chunk` of a resident layer ([chunk][3][64])
__device__ __forceinline__ void salx_frag(bf16x8 (&wf)[3], const bf16x8 *w, int chunk, int lane) {
#pragma unroll
    for (int t = 0; t < 3; ++t) wf[t] = w[(chunk * 3 + t) * 64 + lane];
}

// NWV waves per workgroup, WPE of them per SIMD once the CU is full (the register budget: 512 / WPE)
template <int C1, int C2, int C3, int NS, int NWV, int WPE>
__global__ __launch_bounds__(64 * NWV) __attribute__((amdgpu_waves_per_eu(WPE, WPE))) void sa_lds_bf16x9_kernel(SALX9Args a, int nunits_total) {
    using G = SALX9Geom<C1, C2, C3>;
    constexpr int KB1 = G::KB1, NC2 = G::NC2, KB2 = G::KB2, NC3 = G::NC3, NTH = 64 * NWV;
    static_assert(NS == 16 || NS == 32, "a 32-row unit is one neighbourhood or two");
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *w2l = reinterpret_cast<bf16x8 *>(lds);        // [KB1][NC2][3][64]
    bf16x8 *w3l = w2l + G::W2N;                           // [KB2][NC3][3][64]
    f32x4 *w1l = reinterpret_cast<f32x4 *>(w3l + G::W3N);  // [C1] rows (wx, wy, wz, b1)
    float *b2l = reinterpret_cast<float *>(w1l + C1);     // [C2]
    float *b3l = b2l + C2;                                // [C3]
    constexpr bool AHEAD = WPE < (C2 > 64 ? 3 : 4);  // where the registers allow (no scratch): fragments one chunk, feature rows one unit ahead
    const int tid = threadIdx.x, lane = tid & 63, pt = lane & 15, g = lane >> 4;
    for (int e = tid; e < G::W2N; e += NTH) w2l[e] = a.w2[e];
    for (int e = tid; e < G::W3N; e += NTH) w3l[e] = a.w3[e];
    gp_sa_rows::stage_operands<C1, C2, C3, NTH>(a, w1l, b2l, b3l, tid);
    __syncthreads();  // the only barrier: every wave walks its own units from here on
    const gp_sa_rows::Units<NS> un(nunits_total, NWV, tid);
    int jcur[2], jn[2];
    float dcur[2][3];
    un.load_idx(a, 0, pt, jcur);
    un.load_d(a, 0, jcur, dcur);
    un.load_idx(a, 1, pt, jn);
    // the hoisted feature rows of the unit's two points (this lane group's four channels) and their first k-block, one unit ahead
    const float *zrow[2];
    f32x4 z0[2][2];  // [sub][chunk of k-block 0]
    if constexpr (AHEAD) {
        un.z_rows(a, 0, jcur, 4 * g, zrow);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c) z0[s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 16 * c);
    }
#pragma unroll 1
    for (int it = 0; it < un.my_units; ++it) {
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));  // keep the LDS operand reads inside the loop (see sa_chain_lds_kernel)
        const int g4 = (lo_ >> 4) * 4;
        // ---- layers 1 + 2: k-block by k-block; the hoisted feature rows of k-block kb + 1 are requested while kb is multiplied
        f32x4 zz[2][2];
        if constexpr (!AHEAD) un.z_rows(a, it, jcur, g4, zrow);
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c) zz[s][c] = AHEAD ? z0[s][c] : *reinterpret_cast<const f32x4 *>(zrow[s] + 16 * c);
        f32x4 acc2[NC2][2];  // layer-2 accumulators [chunk][sub], opened by the first k-block
#pragma unroll
        for (int kb = 0; kb < KB1; ++kb) {
            Split8 xs[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f32x4 h[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) h[c] = gp_sa_rows::layer1(w1l, 2 * kb + c, g4, zz[s][c], dcur[s][0], dcur[s][1], dcur[s][2]);  // chunks 2 kb, 2 kb + 1
                xs[s] = split8(h[0], h[1]);
            }
            // (into the registers layer 1 has just consumed)
            if (kb + 1 < KB1) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int c = 0; c < 2; ++c) zz[s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 32 * (kb + 1) + 16 * c);
            }
            bf16x8 wf[2][3];
            if (AHEAD) salx_frag(wf[0], w2l + kb * NC2 * 3 * 64, 0, lo_);
#pragma unroll
            for (int n = 0; n < NC2; ++n) {
                if (!AHEAD) salx_frag(wf[n & 1], w2l + kb * NC2 * 3 * 64, n, lo_);
                else if (n + 1 < NC2) salx_frag(wf[(n + 1) & 1], w2l + kb * NC2 * 3 * 64, n + 1, lo_);
                mma9<2, false, SA_NPROD>(wf[n & 1], xs, acc2[n], kb == 0);
                __builtin_amdgcn_sched_barrier(0);  // one chunk per region: the optimiser would hoist every fragment read of the layer
            }
        }
        const int unit = un.unit_of(it);
        un.advance(a, it, pt, jcur, jn, dcur);
        // the next unit's rows (past the wave's last unit: unit 0's, read and dropped) - its first k-block travels under layer 3
        if constexpr (AHEAD) {
            un.z_rows(a, it + 1, jcur, g4, zrow);
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int c = 0; c < 2; ++c) z0[s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 16 * c);
        }
        // ---- bias + ReLU of the hidden layer, in place in fp32; split one k-block (chunks 2 m, 2 m + 1) at a time as layer 3 consumes it
#pragma unroll
        for (int n = 0; n < NC2; ++n) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(b2l + 16 * n + g4);
#pragma unroll
            for (int s = 0; s < 2; ++s) acc2[n][s] = relu4(acc2[n][s] + bv);
        }
        // ---- layer 3 (transposed: lane = channel, registers x lane groups = the 16 points of a sub-chunk), all eight output chunks
        f32x4 acc3[NC3][2];
#pragma unroll
        for (int kb = 0; kb < KB2; ++kb) {
            Split8 xs[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) xs[s] = split8(acc2[2 * kb][s], acc2[2 * kb + 1][s]);
            bf16x8 wf[2][3];
            if (AHEAD) salx_frag(wf[0], w3l + kb * NC3 * 3 * 64, 0, lo_);
#pragma unroll
            for (int n = 0; n < NC3; ++n) {
                if (!AHEAD) salx_frag(wf[n & 1], w3l + kb * NC3 * 3 * 64, n, lo_);
                else if (n + 1 < NC3) salx_frag(wf[(n + 1) & 1], w3l + kb * NC3 * 3 * 64, n + 1, lo_);
                mma9<2, true, SA_NPROD>(wf[n & 1], xs, acc3[n], kb == 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // pooling over the points, bias + ReLU, store
#pragma unroll
        for (int n = 0; n < NC3; ++n) gp_sa_rows::pooled_store<NS>(a, b3l, acc3[n][0], acc3[n][1], 16 * n + (lo_ & 15), unit, g == 0);
    }
}

// Workgroup geometry of an instance: waves per workgroup and workgroups per CU (75 KB of LDS fits twice, 111 KB once), chosen by the
// stand-alone timings at 640 clouds (profiles/sa_lds_bf16x9.txt, us): 64-64-128 12 x 1 394, 8 x 1 413, 6 x 2 498 (8 x 2 needs 128 registers:
// 40 B of scratch, not run); 64-96-128 8 x 1 1 073, 12 x 1 1 088.  The macros are for tuning builds.
#ifndef SALX9_NARROW_WAVES
#define SALX9_NARROW_WAVES 12
#endif
#ifndef SALX9_NARROW_PER_CU
#define SALX9_NARROW_PER_CU 1
#endif
#ifndef SALX9_WIDE_WAVES
#define SALX9_WIDE_WAVES 8
#endif
template <int C2>
struct SALX9Plan {
    static constexpr int NWV = C2 <= 64 ? SALX9_NARROW_WAVES : SALX9_WIDE_WAVES;
    static constexpr int PER_CU = C2 <= 64 ? SALX9_NARROW_PER_CU : 1;
    static constexpr int WPE = NWV * PER_CU / 4;
    static_assert(NWV * PER_CU % 4 == 0 && WPE >= 1 && WPE <= 4 && PER_CU * SALX9Geom<64, C2, 128>::LDS <= 160 * 1024, "whole waves per SIMD, LDS");
};

template <int C1, int C2, int C3, int NS>
int launch_lds_bf16x9(const SALX9Args &a, int b, hipStream_t st) {
    using P = SALX9Plan<C2>;
    const int nunits = (int)(((size_t)b * a.np * NS) / 32);
    int blocks = (nunits + P::NWV - 1) / P::NWV;
    if (blocks > gp_num_cus() * P::PER_CU) blocks = gp_num_cus() * P::PER_CU;  // persistent
    return gp_launch<sa_lds_bf16x9_kernel<C1, C2, C3, NS, P::NWV, P::WPE>>(dim3(blocks), dim3(64 * P::NWV), SALX9Geom<C1, C2, C3>::LDS, st, a, nunits);
}

}  // namespace

extern "C" {

int gp_sa_lds_bf16x9(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx, const float *z,
                     int zstride, int zoff, const float *wxyz, const float *bias1, const void *w2_x9, const float *bias2, const void *w3_x9,
                     const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s) {
    if (!gp_sa_rows::units_args_ok(b, n, np, ns, c1, c3, zstride, zoff, cout_total, cout_off,
                                   {xyz, new_xyz, idx, z, wxyz, bias1, w2_x9, bias2, w3_x9, bias3, out}))
        return GP_EINVAL;
    const bool s0 = c1 == 64 && c2 == 64 && c3 == 128 && ns == 16, s1 = c1 == 64 && c2 == 96 && c3 == 128 && ns == 32;
    if (!s0 && !s1) return GP_EINVAL;  // grouping level 1 of the light / dense encoders
    if (b == 0) return GP_OK;
    const SALX9Args a{n, np, zstride, zoff, xyz, new_xyz, z, idx, wxyz, bias1, reinterpret_cast<const bf16x8 *>(w2_x9), bias2,
                      reinterpret_cast<const bf16x8 *>(w3_x9), bias3, out, cout_total, cout_off};
    return s0 ? launch_lds_bf16x9<64, 64, 128, 16>(a, b, (hipStream_t)s) : launch_lds_bf16x9<64, 96, 128, 32>(a, b, (hipStream_t)s);
}

}  // extern "C"
