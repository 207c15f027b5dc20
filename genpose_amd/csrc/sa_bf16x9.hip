// Grouping level 2 of the light / dense / lighter encoders (hoisted first layer -> 128 -> 196 -> 256 -> max over the neighbourhood) with the two
// dense layers as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h): every fp32 operand is hi + mid + lo, all nine cross products are
// exact in fp32 and only the fp32 accumulation rounds - the error class of sa_chain_ring_kernel<128, 196, 256, NS> (sa_mlp.hip), whose job,
// inputs and [B, 128, 256] output per scale this kernel takes over (encoder precision 'bf16x9'; the fp32 kernel stays selectable as 'f32').
// Furthest point sampling and the ball queries see coordinates only: centres and neighbourhoods are bit-identical either way.
//
// Form: sa_bf16x3.hip's - 8 waves per workgroup, one persistent workgroup per CU, 32 rows per wave and iteration (one neighbourhood of 32 or
// two of 16: every weight fragment read from LDS feeds two B tiles), activations register-resident from the gather to the pooled output,
// layer 1 on the fp32 VALU with the fp32 kernel's arithmetic, layer 3 transposed (activations as the A operand, lane = channel) in halves of
// eight output chunks, max over the points before bias + ReLU - except that three terms per weight do not leave layer 2 LDS-resident
// (128 x 208 x 3 x 2 B = 160 KB), so BOTH layers stream through a 2-slot LDS ring in 22 slices of 24 KB = (one 32-wide k-block) x (8 output
// chunks) x (hi, mid, lo): layer 2 as (k-block, chunk half) = 8 slices (13 chunks padded to 16 with zero weights; the MFMAs of the padding
// chunks are skipped), layer 3 as (half, k-block) = 14.  Slice s + 1 (held in registers since step s - 1) is written into the other slot
// while slot s is multiplied, slice s + 2 is requested, one barrier per slice; the slice in flight stays in flight across the barrier.
// Hidden activations stay in fp32 registers and are split one k-block at a time as the next layer consumes them.
// The 196-wide layer is padded to 208 outputs (zero weights, zero bias: ReLU(0) = 0) and 224 layer-3 inputs (chunk 13 is a literal zero).
// Budget per workgroup iteration (256 rows; MI355X: v_mfma_f32_16x16x32_bf16 16 cycles, LDS 128 B/clk/CU):
//   MFMA                (4 x 13 + 7 x 16) chunks x 9 products x 2 tiles = 2 952 per wave x 16 cycles x 2 waves per SIMD = 94 k cycles
//   LDS fragment reads  (52 + 112) KB x 3 terms x 8 waves = 3.9 MB -> 31 k cycles;  ring writes 528 KB
// so the matrix pipe bounds it.
#include "bf16x9.h"

namespace {

using namespace gp_bf16x9;

struct SAX9Args {
    int n, np, zstride, zoff;
    const float *xyz, *new_xyz, *z;
    const int32_t *idx;
    const float *wxyz, *b1;  // layer 1 stays on the fp32 VALU (three FMAs per channel on top of the hoisted feature half)
    const bf16x8 *w;         // [22 slices][8 chunks][3 = hi, mid, lo][64 lanes] (weights.py: pack_sa_bf16x9)
    const float *b2;         // [224] (zero padded)
    const float *b3;         // [256]
    float *out;
    int cout_total, cout_off;
};

constexpr int SX_C1 = 128, SX_C2 = 196, SX_C3 = 256;
constexpr int SX_KB1 = SX_C1 / 32, SX_NC2 = (SX_C2 + 15) / 16, SX_KB2 = (SX_NC2 + 1) / 2, SX_NCS = 8, SX_NHALF = SX_C3 / 128;
constexpr int SX_NWV = 8, SX_NTH = 64 * SX_NWV;
constexpr int SX_SLICE = SX_NCS * 3 * 64;  // bf16x8 (16 B) per slice = 24 KB
constexpr int SX_PER_T = SX_SLICE / SX_NTH;
constexpr int SX_NSL = 2 * SX_KB1 + SX_NHALF * SX_KB2;  // slices per iteration: 8 + 14
constexpr size_t SX_LDS = (size_t)(2 * SX_SLICE + SX_C1) * 16 + (size_t)(32 * SX_KB2 + SX_C3) * sizeof(float);
static_assert(SX_NC2 > SX_NCS && SX_NC2 <= 2 * SX_NCS && SX_NC2 - SX_NCS >= SX_PER_T && SX_PER_T * SX_NTH == SX_SLICE, "slice geometry");
static_assert(SX_LDS <= 160 * 1024, "LDS");

// End of a ring step: this wave's LDS writes of the step have completed (lgkmcnt), then the bare barrier.  No vmcnt wait: the slice in
// flight to the registers stays in flight across it (trunk_bf16x9.hip's x9_barrier).
__device__ __forceinline__ void sx_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// Keeps a value's uses behind this point (no instruction: the optimiser may not move what is computed from it further up).
__device__ __forceinline__ void sx_pin(f32x4 &v) { asm volatile("" : "+v"(v)); }

// mma9 (bf16x9.h) transposed: acc[p] += X[p] . W with the activations as the A operand - the same nine products in the same order
__device__ __forceinline__ void mma9t(const bf16x8 (&w)[3], const Split8 (&x)[2], f32x4 (&acc)[2]) {
    constexpr int WA[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0};
    constexpr int XB[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int p = 0; p < 2; ++p) acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(x[p].t[XB[q]], w[WA[q]], acc[p], 0, 0, 0);
}

struct SXRing {
    bf16x8 *ring;
    const bf16x8 *w;
    int par, snext;  // slot of the slice being multiplied; slice to request next
};

// One ring step over the current slot: for chunk n < NCH of the slice (output chunk N0 + n of acc), the three weight terms (read one chunk
// ahead) x the two row tiles' split k-block = 18 MFMAs; beside chunk n < PER_T, element n of the next slice goes from the registers to the
// other slot (last read one step ago) and element n of the slice after it is requested; one barrier.
template <bool TRANSPOSED, int N0, int NCH, int NA>
__device__ __forceinline__ void sx_step(SXRing &r, bf16x8 (&hold)[SX_PER_T], const Split8 (&xs)[2], f32x4 (&acc)[2][NA], int tid, int lane) {
    static_assert(NCH >= SX_PER_T && NCH <= SX_NCS && N0 + NCH <= NA, "every slice element moves beside a chunk");
    const bf16x8 *slot = r.ring + r.par * SX_SLICE;
    bf16x8 *dst = r.ring + (r.par ^ 1) * SX_SLICE;
    const bf16x8 *src = r.w + (size_t)r.snext * SX_SLICE;
    bf16x8 wf[2][3];
#pragma unroll
    for (int t = 0; t < 3; ++t) wf[0][t] = slot[t * 64 + lane];
#pragma unroll
    for (int n = 0; n < NCH; ++n) {
        if (n + 1 < NCH) {
#pragma unroll
            for (int t = 0; t < 3; ++t) wf[(n + 1) & 1][t] = slot[((n + 1) * 3 + t) * 64 + lane];
        }
        if (n < SX_PER_T) {
            dst[tid + n * SX_NTH] = hold[n];
            hold[n] = src[tid + n * SX_NTH];
        }
        f32x4 an[2] = {acc[0][N0 + n], acc[1][N0 + n]};
        if constexpr (TRANSPOSED) mma9t(wf[n & 1], xs, an);
        else mma9<2>(wf[n & 1], xs, an);
        acc[0][N0 + n] = an[0], acc[1][N0 + n] = an[1];
        __builtin_amdgcn_sched_barrier(0);  // one chunk per region: the optimiser would hoist every fragment read of the step
    }
    r.par ^= 1;
    r.snext = r.snext + 1 == SX_NSL ? 0 : r.snext + 1;
    sx_barrier();
}

template <int NS>
__global__ __launch_bounds__(SX_NTH) void sa_chain_bf16x9_kernel(SAX9Args a, int nunits_total) {
    static_assert(NS == 16 || NS == 32, "a 32-row unit is one neighbourhood or two");
    constexpr int C1 = SX_C1, C3 = SX_C3, KB1 = SX_KB1, NC2 = SX_NC2, KB2 = SX_KB2, NCS = SX_NCS, NHALF = SX_NHALF, NWV = SX_NWV, NTH = SX_NTH;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);                 // [2][SLICE]
    f32x4 *w1l = reinterpret_cast<f32x4 *>(ring + 2 * SX_SLICE);    // [C1] rows (wx, wy, wz, b1)
    float *b2l = reinterpret_cast<float *>(w1l + C1);               // [32 KB2]
    float *b3l = b2l + 32 * KB2;                                    // [C3]
    const int tid = threadIdx.x, lane = tid & 63, pt = lane & 15, g = lane >> 4;
    for (int e = tid; e < C1; e += NTH) {
        f32x4 w = *reinterpret_cast<const f32x4 *>(a.wxyz + e * 4);
        w.w = a.b1[e];
        w1l[e] = w;
    }
    for (int e = tid; e < 32 * KB2; e += NTH) b2l[e] = a.b2[e];
    for (int e = tid; e < C3; e += NTH) b3l[e] = a.b3[e];
    // ring prologue: slice 0 into slot 0; slice 1 held in registers (written during step 0)
    bf16x8 hold[SX_PER_T];
#pragma unroll
    for (int u = 0; u < SX_PER_T; ++u) {
        ring[tid + u * NTH] = a.w[tid + u * NTH];
        hold[u] = a.w[SX_SLICE + tid + u * NTH];
    }
    __syncthreads();
    SXRing rg = {ring, a.w, 0, 2};
    const int wave_global = blockIdx.x * NWV + __builtin_amdgcn_readfirstlane(tid >> 6), nwaves = gridDim.x * NWV;
    const int my_units = wave_global < nunits_total ? (nunits_total - wave_global + nwaves - 1) / nwaves : 0;
    // every wave runs the same number of iterations (idle ones compute on clamped rows and store nothing): barrier counts match
    const int nits_wg = (nunits_total + nwaves - 1) / nwaves;
    // unit `it` of this wave: 32 consecutive (centre, sample) rows = sub-chunks s = 0, 1 of 16 rows
    auto unit_of = [&](int it) { return it < my_units ? wave_global + it * nwaves : 0; };
    auto load_idx = [&](int it, int (&j)[2]) {
        const size_t r0 = (size_t)unit_of(it) * 32;
#pragma unroll
        for (int s = 0; s < 2; ++s) j[s] = a.idx[r0 + 16 * s + pt];
    };
    auto centre_of = [&](int it, int s) { return (unit_of(it) * 32 + 16 * s) / NS; };
    auto load_d = [&](int it, const int (&j)[2], float (&d)[2][3]) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int cc = centre_of(it, s), bcl = cc / a.np;
            const float *xyz = a.xyz + (size_t)bcl * a.n * 3;
            const float *cp = a.new_xyz + (size_t)cc * 3;
            d[s][0] = xyz[j[s] * 3 + 0] - cp[0];  // grouped_xyz -= new_xyz (pointnet2_utils.py:253)
            d[s][1] = xyz[j[s] * 3 + 1] - cp[1];
            d[s][2] = xyz[j[s] * 3 + 2] - cp[2];
        }
    };
    int jcur[2], jn[2];
    float dcur[2][3];
    load_idx(0, jcur);
    load_d(0, jcur, dcur);
    load_idx(1, jn);
#pragma unroll 1
    for (int it = 0; it < nits_wg; ++it) {
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));  // keep the LDS operand reads inside the loop (see sa_chain_lds_kernel)
        const int g4 = (lo_ >> 4) * 4;
        // ---- layers 1 + 2: k-block by k-block; the hoisted feature rows of k-block kb + 1 are requested while kb is multiplied
        const float *zrow[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int bcl = centre_of(it, s) / a.np;
            zrow[s] = a.z + ((size_t)bcl * a.n + jcur[s]) * a.zstride + a.zoff + g4;
        }
        f32x4 zz[2][2];  // [sub][chunk of the k-block]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c) zz[s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 16 * c);
        f32x4 acc2[2][NC2];  // layer-2 accumulators, then (bias + ReLU in place) the hidden layer in fp32
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int n = 0; n < NC2; ++n) acc2[s][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB1; ++kb) {
            Split8 xs[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const float dx = dcur[s][0], dy = dcur[s][1], dz = dcur[s][2];
                f32x4 h[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const int q = 2 * kb + c;
                    const f32x4 r0 = w1l[16 * q + g4 + 0], r1 = w1l[16 * q + g4 + 1], r2 = w1l[16 * q + g4 + 2], r3 = w1l[16 * q + g4 + 3];
                    f32x4 v = zz[s][c];
                    v.x += (r0.x * dx + r0.y * dy + r0.z * dz) + r0.w;  // the fp32 kernels' layer-1 arithmetic
                    v.y += (r1.x * dx + r1.y * dy + r1.z * dz) + r1.w;
                    v.z += (r2.x * dx + r2.y * dy + r2.z * dz) + r2.w;
                    v.w += (r3.x * dx + r3.y * dy + r3.z * dz) + r3.w;
                    h[c] = relu4(v);
                }
                xs[s] = split8(h[0], h[1]);
            }
            // (into the registers layer 1 has just consumed: the two ring steps cover the latency)
            if (kb + 1 < KB1) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int c = 0; c < 2; ++c) zz[s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 32 * (kb + 1) + 16 * c);
            }
            sx_step<false, 0, NCS>(rg, hold, xs, acc2, tid, lo_);
            sx_step<false, NCS, NC2 - NCS>(rg, hold, xs, acc2, tid, lo_);
        }
        // the next unit's indices were requested an iteration ago: its coordinates now, the indices of the one after
        const int cur_valid = it < my_units;
        const int unit = unit_of(it);
        load_d(it + 1, jn, dcur);
        jcur[0] = jn[0], jcur[1] = jn[1];
        load_idx(it + 2, jn);
        // ---- bias + ReLU of the hidden layer, kept in fp32 (bias zero on the padding channels of chunk 12: they stay zero)
#pragma unroll
        for (int n = 0; n < NC2; ++n) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(b2l + 16 * n + g4);
#pragma unroll
            for (int s = 0; s < 2; ++s) acc2[s][n] = relu4(acc2[s][n] + bv);
        }
        // ---- layer 3 (transposed: lane = channel, registers x lane groups = the 16 points of a sub-chunk), eight output chunks at a time
#pragma unroll 1
        for (int half = 0; half < NHALF; ++half) {
            f32x4 acc3[2][NCS];
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int n = 0; n < NCS; ++n) acc3[s][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB2; ++kb) {
                Split8 xs[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    // (pinned: the split does not depend on `half`, and hoisted out of that loop all 14 of them would live in registers)
                    sx_pin(acc2[s][2 * kb]);
                    if (2 * kb + 1 < NC2) sx_pin(acc2[s][2 * kb + 1]);
                    xs[s] = split8(acc2[s][2 * kb], 2 * kb + 1 < NC2 ? acc2[s][2 * kb + 1] : f32x4{0.f, 0.f, 0.f, 0.f});  // (chunk 13: the zero k-padding)
                }
                sx_step<true, 0, NCS>(rg, hold, xs, acc3, tid, lo_);
            }
            // pooling over the points (max_i relu(x_i + b) = relu(max_i x_i + b): bias and ReLU once per channel, after the pooling)
#pragma unroll
            for (int n = 0; n < NCS; ++n) {
                const float m0 = points16_max_t(acc3[0][n]), m1 = points16_max_t(acc3[1][n]);
                const int ch = 16 * (half * NCS + n) + (lo_ & 15);
                const float b = b3l[ch];
                if (cur_valid && g == 0) {
                    if (NS == 32) {
                        a.out[(size_t)unit * a.cout_total + a.cout_off + ch] = fmaxf(fmaxf(m0, m1) + b, 0.f);
                    } else {
                        a.out[(size_t)(2 * unit) * a.cout_total + a.cout_off + ch] = fmaxf(m0 + b, 0.f);
                        a.out[(size_t)(2 * unit + 1) * a.cout_total + a.cout_off + ch] = fmaxf(m1 + b, 0.f);
                    }
                }
            }
        }
    }
}

template <int NS>
int launch_bf16x9(const SAX9Args &a, int b, hipStream_t st) {
    auto kern = sa_chain_bf16x9_kernel<NS>;
    static bool done = false;
    if (!done) {
        if (set_lds(kern, SX_LDS)) return GP_ELAUNCH;
        done = true;
    }
    const int nunits = (int)(((size_t)b * a.np * NS) / 32);
    int blocks = (nunits + SX_NWV - 1) / SX_NWV;
    if (blocks > gp_num_cus()) blocks = gp_num_cus();  // persistent: one 8-wave workgroup per CU
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(SX_NTH), SX_LDS, st, a, nunits);
    return gp_launch_status();
}

}  // namespace

extern "C" {

int gp_sa_pre_mlp_max_bf16x9(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                             const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const void *w23_x9, const float *bias2,
                             const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s) {
    if (b < 0 || n <= 0 || np <= 0 || !xyz || !new_xyz || !idx || !z || !wxyz || !bias1 || !w23_x9 || !bias2 || !bias3 || !out) return GP_EINVAL;
    if (c1 != SX_C1 || c2 != SX_C2 || c3 != SX_C3 || (ns != 16 && ns != 32)) return GP_EINVAL;  // grouping level 2
    if ((cout_total & 3) || (cout_off & 3) || cout_off < 0 || cout_off + c3 > cout_total || (zstride & 3) || (zoff & 3) || zoff < 0 || zoff + c1 > zstride)
        return GP_EINVAL;
    if (((size_t)b * np * ns) % 32 || ((size_t)b * np * ns) / 32 > 0x3ffffffu) return GP_EINVAL;  // whole 32-row units, row indices in an int
    if (b == 0) return GP_OK;
    const SAX9Args a{n, np, zstride, zoff, xyz, new_xyz, z, idx, wxyz, bias1, reinterpret_cast<const bf16x8 *>(w23_x9), bias2, bias3, out, cout_total, cout_off};
    return ns == 32 ? launch_bf16x9<32>(a, b, (hipStream_t)s) : launch_bf16x9<16>(a, b, (hipStream_t)s);
}

}  // extern "C"
