// OPT-IN, EXPLORATORY (round 5): one set-abstraction scale (hoisted first layer -> two dense layers -> max over the neighbourhood) with the
// dense layers on the BF16 matrix pipe as THREE-TERM SPLIT PRODUCTS, fp32 accumulate:
//       a . b  ~=  a_hi . b_hi  +  a_lo . b_hi  +  a_hi . b_lo ,      x_hi = bf16(x),  x_lo = bf16(x - x_hi)
// (relative error ~2^-17 per product - the dropped a_lo . b_lo term and the 8-bit lo parts - against 2^-24 for the fp32 pipe; the reference's own
// convolutions run at TF32 = 2^-11 on its stated RTX 3090 / PyTorch 1.12).  v_mfma_f32_16x16x32_bf16 issues 16x the FLOPs per cycle of
// v_mfma_f32_16x16x4_f32, so three of them per product are 5.3x the fp32 rate on paper.  NOT the default: the headline numbers and every parity
// claim are the fp32 kernels' (sa_mlp.hip); this file is reached only through gp_sa_pre_mlp_max_bf16x3 (encoder precision 'bf16x3').
// Furthest point sampling and the ball queries see coordinates only: centres and neighbourhoods are bit-identical either way.
//
// Form: sa_chain_ring_kernel's (sa_mlp.hip) - 8 waves per workgroup, activations register-resident from the gather to the pooled output,
// layer-2 weights LDS-resident, layer-3 weights through a 3-slot LDS ring shared by the waves, one barrier per ring step; the row front and
// back end (unit schedule, prefetch, layer 1, pooled store) is sa_rows.h's, shared with sa_bf16x9.hip - with
//   * 32 rows per wave and iteration (two 16-row sub-chunks: one neighbourhood of 32, or two of 16), so that every weight fragment read
//     from LDS feeds two rows' worth of matrix instructions (at 16 rows the kernel would be bound by the LDS reads: the matrix work shrinks
//     5x, the fragment bytes do not);
//   * the D fragment of a layer (lane = point, four consecutive channels of a 16-channel chunk) still IS the next layer's operand: two chunks
//     (2m, 2m+1) make the eight k-values a lane holds for k-block m of v_mfma_f32_16x16x32_bf16 - the host packs the weights in that k order
//     (weights.py: pack_bf16x3);
//   * layer 3 in halves of eight output chunks (64 accumulator registers for the two sub-chunks), ring slice = (half, k-block) = 16 KB;
//   * level 1 (64-64/96-128: all weights fit LDS) runs the same kernel without the ring and without a barrier in the loop.
#include "bf16x3.h"
#include "sa_rows.h"

namespace {

using namespace gp_bf16x3;

struct SABfArgs {
    int n, np, zstride, zoff;
    const float *xyz, *new_xyz, *z;
    const int32_t *idx;
    const float *wxyz, *b1;  // layer 1 stays on the fp32 VALU (three FMAs per channel on top of the hoisted feature half)
    const bf16x8 *w2;        // [KB1][NC2][2 = hi, lo][64 lanes]
    const float *b2;         // [32 * KB2] (zero padded)
    const bf16x8 *w3;        // [2 halves][KB2][8 chunks][2 = hi, lo][64 lanes]
    const float *b3;
    float *out;
    int cout_total, cout_off;
};

// RING: layer-3 weights through the 3-slot ring (level 2: 224 KB of them); !RING: they are LDS-resident too and the loop has no barrier
// (level 1: 64-64/96-128, 32-48 KB) - sa_chain_lds_kernel's form.
template <int C1, int C2, int C3, int NS, bool RING>
__global__ __launch_bounds__(512) void sa_chain_bf16x3_kernel(SABfArgs a, int nunits_total) {
    constexpr int KB1 = C1 / 32, NC2 = (C2 + 15) / 16, KB2 = (NC2 + 1) / 2, NC3H = 8, NHALF = C3 / 128, NWV = 8, NTH = 512;
    static_assert(C1 % 32 == 0 && C3 % 128 == 0 && (NS == 16 || NS == 32), "grouping levels 1 and 2 of the light / dense / lighter encoders");
    constexpr int SLICE = NC3H * 2 * 64;   // bf16x8 (16 B) per slice: one (half, k-block) of layer 3 = 16 KB
    constexpr int PER_T = SLICE / NTH;
    constexpr int NSL = NHALF * KB2;       // slices per iteration
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *w2l = reinterpret_cast<bf16x8 *>(lds);                 // [KB1][NC2][2][64] resident
    bf16x8 *ring = w2l + KB1 * NC2 * 2 * 64;                        // RING: [3][SLICE]; else all [NSL][SLICE] slices
    f32x4 *w1l = reinterpret_cast<f32x4 *>(ring + (RING ? 3 : NSL) * SLICE);  // [C1] rows (wx, wy, wz, b1)
    float *b2l = reinterpret_cast<float *>(w1l + C1);               // [32 KB2]
    float *b3l = b2l + 32 * KB2;                                    // [C3]
    const int tid = threadIdx.x, lane = tid & 63, pt = lane & 15, g = lane >> 4;
    for (int e = tid; e < KB1 * NC2 * 2 * 64; e += NTH) w2l[e] = a.w2[e];
    gp_sa_rows::stage_operands<C1, 32 * KB2, C3, NTH>(a, w1l, b2l, b3l, tid);
    // ring prologue: slices 0 and 1 into slots 0 and 1; slice 2 held in registers
    bf16x8 hold[PER_T];
    if constexpr (RING) {
#pragma unroll
        for (int u = 0; u < PER_T; ++u) {
            ring[0 * SLICE + tid + u * NTH] = a.w3[0 * SLICE + tid + u * NTH];
            ring[1 * SLICE + tid + u * NTH] = a.w3[1 * SLICE + tid + u * NTH];
            hold[u] = a.w3[2 * SLICE + tid + u * NTH];
        }
    } else {
        for (int e = tid; e < NSL * SLICE; e += NTH) ring[e] = a.w3[e];
    }
    __syncthreads();
    // RING: every wave runs the same number of iterations (idle ones compute on clamped rows and store nothing): barrier counts match
    const gp_sa_rows::Units<NS> un(nunits_total, NWV, tid);
    const int nits_wg = RING ? un.nits_all(nunits_total) : un.my_units;
    int jcur[2], jn[2];
    float dcur[2][3];
    un.load_idx(a, 0, pt, jcur);
    un.load_d(a, 0, jcur, dcur);
    un.load_idx(a, 1, pt, jn);
    int gstep = 0;  // global ring step: slice gstep % NSL sits in slot gstep % 3
#pragma unroll 1
    for (int it = 0; it < nits_wg; ++it) {
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));  // keep the LDS weight reads inside the loop (see sa_chain_lds_kernel)
        const int g4 = (lo_ >> 4) * 4;
        // ---- layers 1 + 2: k-block by k-block; the hoisted feature rows of k-block kb + 1 are requested while kb is multiplied
        const float *zrow[2];
        un.z_rows(a, it, jcur, g4, zrow);
        f32x4 zz[2][2][2];  // [buffer][sub][chunk of the k-block]
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int c = 0; c < 2; ++c) zz[0][s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 16 * c);
        f32x4 acc2[NC2][2];
#pragma unroll
        for (int n = 0; n < NC2; ++n) acc2[n][0] = acc2[n][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB1; ++kb) {
            if (kb + 1 < KB1) {
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int c = 0; c < 2; ++c) zz[(kb + 1) & 1][s][c] = *reinterpret_cast<const f32x4 *>(zrow[s] + 32 * (kb + 1) + 16 * c);
            }
            bf16x8 h1hi[2], h1lo[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                f32x4 h[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) h[c] = gp_sa_rows::layer1(w1l, 2 * kb + c, g4, zz[kb & 1][s][c], dcur[s][0], dcur[s][1], dcur[s][2]);  // chunks 2 kb, 2 kb + 1
                split8(h[0], h[1], h1hi[s], h1lo[s]);
            }
            // two output chunks at a time: four independent accumulators, the three terms in separate passes over them
#pragma unroll
            for (int n0 = 0; n0 < NC2; n0 += 2) {
                bf16x8 wh[2], wl[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int n = n0 + u < NC2 ? n0 + u : NC2 - 1;
                    wh[u] = w2l[((kb * NC2 + n) * 2 + 0) * 64 + lo_];
                    wl[u] = w2l[((kb * NC2 + n) * 2 + 1) * 64 + lo_];
                }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (n0 + u < NC2) {
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc2[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[u], h1hi[s], acc2[n0 + u][s], 0, 0, 0);
                    }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (n0 + u < NC2) {
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc2[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[u], h1hi[s], acc2[n0 + u][s], 0, 0, 0);
                    }
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    if (n0 + u < NC2) {
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc2[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[u], h1lo[s], acc2[n0 + u][s], 0, 0, 0);
                    }
            }
        }
        const bool cur_valid = it < un.my_units;
        const int unit = un.unit_of(it);
        un.advance(a, it, pt, jcur, jn, dcur);
        // ---- bias + ReLU + split of the hidden layer: k-block m of layer 3 = chunks 2m, 2m+1 (a missing odd chunk is zero)
        bf16x8 h2hi[KB2][2], h2lo[KB2][2];
#pragma unroll
        for (int m = 0; m < KB2; ++m)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const f32x4 v0 = relu4(acc2[2 * m][s] + *reinterpret_cast<const f32x4 *>(b2l + 16 * (2 * m) + g4));
                f32x4 v1 = {0.f, 0.f, 0.f, 0.f};
                if (2 * m + 1 < NC2) v1 = relu4(acc2[2 * m + 1][s] + *reinterpret_cast<const f32x4 *>(b2l + 16 * (2 * m + 1) + g4));
                split8(v0, v1, h2hi[m][s], h2lo[m][s]);
            }
        // ---- layer 3 (transposed: lane = channel, registers x lane groups = the 16 points of a sub-chunk), eight output chunks at a time
#pragma unroll 1
        for (int half = 0; half < NHALF; ++half) {
            f32x4 acc3[NC3H][2];
#pragma unroll
            for (int n = 0; n < NC3H; ++n) acc3[n][0] = acc3[n][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB2; ++kb) {
                // slice gstep + 2 (held in registers since the previous step) -> its slot, last read in step gstep - 1
                if constexpr (RING) {
                    bf16x8 *dst = ring + ((gstep + 2) % 3) * SLICE;
#pragma unroll
                    for (int u = 0; u < PER_T; ++u) dst[tid + u * NTH] = hold[u];
                    const bf16x8 *src = a.w3 + (size_t)((gstep + 3) % NSL) * SLICE;
#pragma unroll
                    for (int u = 0; u < PER_T; ++u) hold[u] = src[tid + u * NTH];
                }
                const bf16x8 *slot = RING ? ring + (gstep % 3) * SLICE : ring + (half * KB2 + kb) * SLICE;
#pragma unroll
                for (int n0 = 0; n0 < NC3H; n0 += 2) {
                    bf16x8 wh[2], wl[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        wh[u] = slot[((n0 + u) * 2 + 0) * 64 + lo_];
                        wl[u] = slot[((n0 + u) * 2 + 1) * 64 + lo_];
                    }
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc3[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2hi[kb][s], wh[u], acc3[n0 + u][s], 0, 0, 0);
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc3[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2lo[kb][s], wh[u], acc3[n0 + u][s], 0, 0, 0);
#pragma unroll
                    for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int s = 0; s < 2; ++s) acc3[n0 + u][s] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(h2hi[kb][s], wl[u], acc3[n0 + u][s], 0, 0, 0);
                }
                if constexpr (RING) {
                    ++gstep;
                    __syncthreads();
                }
            }
            // pooling over the points, bias + ReLU, store
#pragma unroll
            for (int n = 0; n < NC3H; ++n)
                gp_sa_rows::pooled_store<NS>(a, b3l, acc3[n][0], acc3[n][1], 16 * (half * NC3H + n) + (lo_ & 15), unit, cur_valid && g == 0);
        }
    }
}

template <int C1, int C2, int C3, int NS, bool RING>
int launch_bf16x3(const SABfArgs &a, int b, hipStream_t st) {
    constexpr int KB1 = C1 / 32, NC2 = (C2 + 15) / 16, KB2 = (NC2 + 1) / 2, NSL = (C3 / 128) * KB2;
    const size_t lds = ((size_t)KB1 * NC2 * 2 * 64 + (RING ? 3 : NSL) * 8 * 2 * 64 + C1) * 16 + (size_t)(32 * KB2 + C3) * sizeof(float);
    if (lds > 160 * 1024) return GP_EINVAL;
    const int nunits = (int)(((size_t)b * a.np * NS) / 32);
    int blocks = (nunits + 7) / 8;
    const int per_cu = RING ? 1 : 2;  // persistent; the resident form (<= 90 KB of LDS, <= 128 registers for the 64-wide hidden layer) fits twice
    if (blocks > gp_num_cus() * per_cu) blocks = gp_num_cus() * per_cu;
    return gp_launch<sa_chain_bf16x3_kernel<C1, C2, C3, NS, RING>>(dim3(blocks), dim3(512), lds, st, a, nunits);
}

}  // namespace

extern "C" {

int gp_sa_pre_mlp_max_bf16x3(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                             const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const void *w2_split, const float *bias2,
                             const void *w3_split, const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s) {
    if (!gp_sa_rows::units_args_ok(b, n, np, ns, c1, c3, zstride, zoff, cout_total, cout_off,
                                   {xyz, new_xyz, idx, z, wxyz, bias1, w2_split, bias2, w3_split, bias3, out}))
        return GP_EINVAL;
    if (b == 0) return GP_OK;
    SABfArgs a{n, np, zstride, zoff, xyz, new_xyz, z, idx, wxyz, bias1, reinterpret_cast<const bf16x8 *>(w2_split), bias2,
               reinterpret_cast<const bf16x8 *>(w3_split), bias3, out, cout_total, cout_off};
    if (c1 == 128 && c2 == 196 && c3 == 256 && ns == 32) return launch_bf16x3<128, 196, 256, 32, true>(a, b, (hipStream_t)s);
    if (c1 == 128 && c2 == 196 && c3 == 256 && ns == 16) return launch_bf16x3<128, 196, 256, 16, true>(a, b, (hipStream_t)s);
    if (c1 == 64 && c2 == 64 && c3 == 128 && ns == 16) return launch_bf16x3<64, 64, 128, 16, false>(a, b, (hipStream_t)s);
    if (c1 == 64 && c2 == 96 && c3 == 128 && ns == 32) return launch_bf16x3<64, 96, 128, 32, false>(a, b, (hipStream_t)s);
    if (c1 == 64 && c2 == 64 && c3 == 128 && ns == 32) return launch_bf16x3<64, 64, 128, 32, false>(a, b, (hipStream_t)s);
    return GP_EINVAL;  // grouping levels 1 and 2 of the light / dense / lighter encoders (exploratory)
}

}  // extern "C"
