// GroupAll level of the light encoder (128 points x [512 features + xyz] -> 256 -> 256 | 384 -> 512 -> max over the cloud, per scale) with ALL
// THREE dense layers as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h; SIX of the nine cross products are formed as the project builds it, NPROD =
// SA_NPROD = GP_SA_X9_PRODUCTS = 6 - all but lo.lo, lo.mid and mid.lo, at most (2^-23 + 2^-32) |a b| per multiply - each exact in fp32;
// with six the kernel keeps 156 B of scratch against 140 B with eight and is still 8 % faster, profiles/x6_products.txt), in ONE launch for both scales: the job of
// gp_point_linear (hoisted feature half of layer 1, both scales) + sa_groupall_ring_kernel<256, 256 | 384, 512> / the 32-row tile kernel
// (sa_mlp.hip), without the [B, 128, 512] hoisted rows in memory, without a zeroed output and without atomics.
//
// Work item = (cloud, scale) = 128 rows.  Form: the score trunk's (trunk_bf16x9.h) - 4 waves per workgroup, one wave per SIMD, two 16-row
// tiles per wave, so that every weight fragment read from LDS feeds 16 MFMAs and a wave has the 256 + 256 registers of its SIMD for the
// layer-2 accumulators (192 at C2 = 384) beside half of h1 (64); 8 waves x 16 rows would read each fragment for 8 MFMAs (94 B/clk of the
// LDS's 128) with 256 registers per wave for 160 + operands.  Persistent workgroups, one per CU: workgroup w serves the contiguous items
// [w I / G, (w + 1) I / G) in ascending order (item = cloud x scales + scale: a workgroup alternates between the scales, whose costs
// differ by 30 %), and the weight stream runs on from item to item through the 2-slot LDS ring (ring_step): slices of 24 KB = 8 output
// chunks x (hi, mid, lo) of one 32-wide k-block,
//   for half = 0, 1:  layer 1 (chunks 8 half .. + 7) x (k-block kb < 16)                     16 slices   feature half, feat rows split per k-block
//                     layer 2 (k-block 4 half + j, j < 4) x (8 chunks h < C2 / 128)          8 | 12
//   layer 3           (chunk group q < 4) x (k-block kb < C2 / 32)                           32 | 48     transposed (lane = channel)
// (layer 1 in two halves, each consumed at once as four k-blocks of layer 2: see ga_item)
// Every accumulator takes its k-blocks in ascending order, the products formed smallest first (mma9).  The xyz half of layer 1 and b1 are
// added on the VALU in sa_rows.h's order, z + (dot + b1), absolute coordinates (GroupAll: no centring); max over the rows before
// bias + ReLU (pooling of sa_groupall_ring_kernel: a wave pools its 32 rows in registers, the four waves meet in LDS once per item).
// A cloud's output depends on nothing but that cloud: an item's arithmetic is the same whichever workgroup serves it, and in whatever
// position.  With one wave per SIMD nothing hides VALU work, so the splits of the NEXT k-block ride beside the MFMAs of a step
// (ring_step's side).
// Per item: (256 + 128 | 192 + 256 | 384) chunk-k-blocks x 16 MFMAs x 16 cycles = 164 k | 213 k cycles per SIMD (all nine products:
// 18 MFMAs, 184 k | 240 k).
#include "bf16x9.h"
#include "sa_rows.h"

namespace {

using namespace gp_bf16x9;

struct GAScale {
    const bf16x8 *w;  // [80 | 104 slices][8 chunks][3 = hi, mid, lo][64 lanes] (weights.py: pack_groupall_bf16x9)
    const float *wxyz, *b1, *b2, *b3;
    int c2, off;
};

struct GAArgs {
    const float *xyz, *feat;
    float *out;
    int cout_total, nsc, nitems;
    GAScale sc0, sc1;
};

constexpr int GA_N = 128, GA_CIN = 512, GA_C1 = 256, GA_C2MAX = 384, GA_C3 = 512;
constexpr int GA_NWV = 4, GA_NTH = 64 * GA_NWV, GA_NCS = 8;
constexpr int GA_KB0 = GA_CIN / 32, GA_NC1 = GA_C1 / 16, GA_KB1 = GA_C1 / 32, GA_NG3 = GA_C3 / (16 * GA_NCS);
constexpr int GA_SLICE = GA_NCS * 3 * 64;  // bf16x8 (16 B) per slice = 24 KB
constexpr int GA_PER_T = GA_SLICE / GA_NTH;
constexpr size_t GA_LDS = (size_t)(2 * GA_SLICE + 2 * GA_C1) * 16 + (size_t)(2 * GA_C2MAX + 2 * GA_C3 + GA_NWV * GA_C3) * sizeof(float);
static_assert(GA_PER_T * GA_NTH == GA_SLICE && GA_PER_T <= GA_NCS && GA_NC1 == 2 * GA_NCS, "slice geometry");
static_assert(GA_LDS <= 160 * 1024, "LDS");

__host__ __device__ constexpr int ga_nslices(int c2) { return 2 * GA_KB0 + GA_KB1 * (c2 / 128) + GA_NG3 * (c2 / 32); }

// The ring's position and the weight stream's: the slices of the workgroup's items one after the other (past its last item: slices of
// scale 0 again, requested and never multiplied).
struct GARing {
    bf16x8 *ring;
    const bf16x8 *w0, *w1;
    int nsl0, nsl1, nsc, iend;
    const bf16x8 *rptr;
    int rleft, ritem, par;
    __device__ __forceinline__ void seek(int item) {
        const int s = item < iend ? item & (nsc - 1) : 0;
        rptr = s ? w1 : w0;
        rleft = s ? nsl1 : nsl0;
    }
    __device__ __forceinline__ const bf16x8 *next() {
        const bf16x8 *p = rptr;
        rptr += GA_SLICE;
        if (--rleft == 0) seek(++ritem);
        return p;
    }
};

// One ring step (bf16x9.h) over the current slot, chunks [N0, N0 + 8) of acc (the position advances before the call, as in the trunk).
template <bool TRANSPOSED, int N0, int NA, class Side>
__device__ __forceinline__ void ga_step(GARing &r, bf16x8 (&hold)[GA_PER_T], const Split8 (&xs)[2], f32x4 (&acc)[2][NA], int tid, int lane, bool first,
                                        Side side) {
    const bf16x8 *slot = r.ring + r.par * GA_SLICE;
    bf16x8 *dst = r.ring + (r.par ^ 1) * GA_SLICE;
    const bf16x8 *src = r.next();
    r.par ^= 1;
    ring_step<GA_NTH, GA_PER_T, TRANSPOSED, N0, GA_NCS, SA_NPROD>(slot, dst, src, hold, xs, acc, tid, lane, first, side);
}

// Piece q < 8 of the split of a k-block held as two fp32 D fragments per tile (v[p][0], v[p][1]): values 2 (q & 3), + 1 of tile q >> 2.
__device__ __forceinline__ void ga_split_piece(Split8 (&x)[2], const f32x4 (&v)[2][2], int q) {
    const int p = q >> 2, i = 2 * (q & 3);
    const f32x4 c = v[p][i >> 2];
    split8_pair(x[p], i, c[i & 3], c[(i & 3) + 1]);
}

// Piece q of a k-block of h1 (chunks c0, c0 + 1 of the half held in acc1; w1h = the staged layer-1 rows of that half): layer 1 =
// relu(feature half + (xyz half + b1)) in sa_rows.h's order (layer1()), then the split.
__device__ __forceinline__ void ga_h1_piece(Split8 (&x)[2], const f32x4 (&acc1)[2][GA_NCS], const f32x4 *w1h, const float (&d)[2][3], int g4, int c0, int q) {
    const int p = q >> 2, i = 2 * (q & 3), c = c0 + (i >> 2), j = i & 3;
    const f32x4 r0 = w1h[16 * c + g4 + j], r1 = w1h[16 * c + g4 + j + 1];
    const f32x4 z = acc1[p][c];
    const float v0 = fmaxf(z[j] + (gp_sa_rows::xyz_dot(r0, d[p][0], d[p][1], d[p][2]) + r0.w), 0.f);
    const float v1 = fmaxf(z[j + 1] + (gp_sa_rows::xyz_dot(r1, d[p][0], d[p][1], d[p][2]) + r1.w), 0.f);
    split8_pair(x[p], i, v0, v1);
}

// Piece q of k-block kb of h2 = relu(layer-2 accumulator + b2), and its split.
template <int NC2>
__device__ __forceinline__ void ga_h2_piece(Split8 (&x)[2], const f32x4 (&acc2)[2][NC2], const float *b2s, int g4, int kb, int q) {
    const int p = q >> 2, i = 2 * (q & 3), c = 2 * kb + (i >> 2), j = i & 3;
    const f32x4 z = acc2[p][c];
    const float b0 = b2s[16 * c + g4 + j], b1 = b2s[16 * c + g4 + j + 1];
    split8_pair(x[p], i, fmaxf(z[j] + b0, 0.f), fmaxf(z[j + 1] + b1, 0.f));
}

// One item: 128 rows of `cloud` through the three layers of a scale with C2 = 16 NC2, pooled per wave into `pool` ([wave][512] pre-bias
// maxima).  h1 (128 registers) beside the layer-2 accumulators (192) and the ring's operands does not fit the 256 + 256 registers of a
// wave, so layer 1 runs in two halves of eight output chunks, each consumed at once as four k-blocks of layer 2:
//   for half: layer 1 chunks 8 half .. + 7 over the 16 input k-blocks (the feat rows are read and split once per half);
//             layer 2 k-blocks 4 half .. + 3 into all NC2 chunks.
// frow[p]: the feat row of tile p at this lane group's four channels; d[p]: its coordinates.
template <int NC2>
__device__ __forceinline__ void ga_item(GARing &rg, bf16x8 (&hold)[GA_PER_T], const float *const (&frow)[2], const float (&d)[2][3], const f32x4 *w1s,
                                        const float *b2s, float *pool, int tid, int lane, int g4, int wave) {
    constexpr int NH2 = NC2 / GA_NCS, KB3 = NC2 / 2;
    static_assert(NH2 == 2 || NH2 == 3, "C2 = 256 | 384");
    Split8 xs2[2][2];  // the k-block being multiplied and the one being split beside it
    f32x4 zz[2][2][2];  // feat rows of two k-blocks in flight: [buffer][tile][chunk of the k-block]
    auto request = [&](f32x4(&z)[2][2], int kb) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int c = 0; c < 2; ++c) z[p][c] = *reinterpret_cast<const f32x4 *>(frow[p] + 32 * kb + 16 * c);
    };
    request(zz[0], 0);
    request(zz[1], 1);
    f32x4 acc2[2][NC2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int n = 0; n < NC2; ++n) acc2[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int half = 0; half < 2; ++half) {
        // ---- layer 1, feature half, chunks 8 half .. + 7: k-block kb + 2 is requested and kb + 1 split beside the MFMAs of kb (after the
        // last two k-blocks: 0 and 1 again, the other half's first)
        f32x4 acc1[2][GA_NCS];
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int n = 0; n < GA_NCS; ++n) acc1[p][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 8; ++q) ga_split_piece(xs2[0], zz[0], q);
        auto l1_block = [&](const Split8(&xc)[2], Split8(&xn)[2], f32x4(&zc)[2][2], const f32x4(&zn)[2][2], int kb) __attribute__((always_inline)) {
            request(zc, (kb + 2) & (GA_KB0 - 1));
            auto side = [&](int n) __attribute__((always_inline)) { ga_split_piece(xn, zn, n); };
            ga_step<false, 0>(rg, hold, xc, acc1, tid, lane, false, side);
        };
#pragma unroll 1
        for (int kb = 0; kb < GA_KB0; kb += 2) {
            l1_block(xs2[0], xs2[1], zz[0], zz[1], kb);
            l1_block(xs2[1], xs2[0], zz[1], zz[0], kb + 1);
        }
        // ---- layer 2, k-blocks 4 half .. + 3: k-block j + 1 of h1 is formed and split beside the last step of k-block j
        const f32x4 *w1h = w1s + 16 * GA_NCS * half;
#pragma unroll
        for (int q = 0; q < 8; ++q) ga_h1_piece(xs2[0], acc1, w1h, d, g4, 0, q);
#pragma unroll
        for (int j = 0; j < GA_KB1 / 2; ++j) {
            const Split8(&xc)[2] = xs2[j & 1];
            Split8(&xn)[2] = xs2[(j + 1) & 1];
            auto side = [&](int n) __attribute__((always_inline)) {
                if (j + 1 < GA_KB1 / 2) ga_h1_piece(xn, acc1, w1h, d, g4, 2 * (j + 1), n);
            };
            const bool first = false;
            ga_step<false, 0>(rg, hold, xc, acc2, tid, lane, first, RingNoSide());
            if constexpr (NH2 == 3) ga_step<false, GA_NCS>(rg, hold, xc, acc2, tid, lane, first, RingNoSide());
            ga_step<false, NC2 - GA_NCS>(rg, hold, xc, acc2, tid, lane, first, side);
        }
    }
    // ---- layer 3 (transposed: lane = channel, registers x lane groups = the 16 points of a tile), eight output chunks at a time; the
    // hidden layer stays in the layer-2 accumulators, bias + ReLU are applied as a k-block is split (once per group of output chunks)
#pragma unroll 1
    for (int grp = 0; grp < GA_NG3; ++grp) {
        f32x4 acc3[2][GA_NCS];
        // (pinned, in the accumulation registers: the splits do not depend on `grp` - hoisted out of that loop all of them would live in
        // registers - and the hidden layer, 128 | 192 values, stays where layer 2 left it; a piece reads the two values it splits)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
            for (int n = 0; n < NC2; ++n) asm volatile("" : "+a"(acc2[p][n]));
        const float *b2g = b2s;
#pragma unroll
        for (int q = 0; q < 8; ++q) ga_h2_piece(xs2[0], acc2, b2g, g4, 0, q);
#pragma unroll
        for (int kb = 0; kb < KB3; ++kb) {
            const Split8(&xc)[2] = xs2[kb & 1];
            Split8(&xn)[2] = xs2[(kb + 1) & 1];
            auto side = [&](int n) __attribute__((always_inline)) {
                if (kb + 1 < KB3) ga_h2_piece(xn, acc2, b2g, g4, kb + 1, n);
            };
            ga_step<true, 0>(rg, hold, xc, acc3, tid, lane, kb == 0, side);
        }
        // the wave's maxima over its 32 rows; the pool buffer was read (previous item) many barriers ago
#pragma unroll
        for (int n = 0; n < GA_NCS; ++n) {
            const float m = fmaxf(points16_max_t(acc3[0][n]), points16_max_t(acc3[1][n]));
            if (lane < 16) pool[wave * GA_C3 + 16 * (grp * GA_NCS + n) + lane] = m;
        }
    }
}

__global__ __launch_bounds__(GA_NTH) void sa_groupall_bf16x9_kernel(GAArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    bf16x8 *ring = reinterpret_cast<bf16x8 *>(lds);                // [2][SLICE]
    f32x4 *w1l = reinterpret_cast<f32x4 *>(ring + 2 * GA_SLICE);   // [scale][C1] rows (wx, wy, wz, b1)
    float *b2l = reinterpret_cast<float *>(w1l + 2 * GA_C1);       // [scale][384]
    float *b3l = b2l + 2 * GA_C2MAX;                               // [scale][C3]
    float *pool = b3l + 2 * GA_C3;                                 // [wave][C3] per-wave maxima of the pre-bias layer-3 output
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), pt = lane & 15;
    gp_sa_rows::stage_operands<GA_C1, 0, GA_C3, GA_NTH>(a.sc0, w1l, b2l, b3l, tid);
    for (int e = tid; e < a.sc0.c2; e += GA_NTH) b2l[e] = a.sc0.b2[e];
    if (a.nsc > 1) {
        gp_sa_rows::stage_operands<GA_C1, 0, GA_C3, GA_NTH>(a.sc1, w1l + GA_C1, b2l + GA_C2MAX, b3l + GA_C3, tid);
        for (int e = tid; e < a.sc1.c2; e += GA_NTH) b2l[GA_C2MAX + e] = a.sc1.b2[e];
    }
    // this workgroup's items, in ascending order
    const int i0 = (int)((long long)blockIdx.x * a.nitems / gridDim.x), i1 = (int)((long long)(blockIdx.x + 1) * a.nitems / gridDim.x);
    GARing rg;
    rg.ring = ring, rg.w0 = a.sc0.w, rg.w1 = a.sc1.w, rg.nsl0 = ga_nslices(a.sc0.c2), rg.nsl1 = ga_nslices(a.sc1.c2), rg.nsc = a.nsc, rg.iend = i1;
    rg.ritem = i0, rg.par = 0;
    rg.seek(i0);
    // ring prologue: slice 0 into slot 0; slice 1 held in registers (written during step 0)
    bf16x8 hold[GA_PER_T];
    {
        const bf16x8 *s0 = rg.next(), *s1 = rg.next();
#pragma unroll
        for (int u = 0; u < GA_PER_T; ++u) {
            ring[tid + u * GA_NTH] = s0[tid + u * GA_NTH];
            hold[u] = s1[tid + u * GA_NTH];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int item = i0; item < i1; ++item) {
        const int s = item & (a.nsc - 1), cloud = a.nsc > 1 ? item >> 1 : item;
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));  // keep the LDS operand reads inside the loop (see sa_chain_lds_kernel)
        const int g4 = (lo_ >> 4) * 4;
        const f32x4 *w1s = w1l + s * GA_C1;
        // rows of the wave's two tiles: points 32 wave + 16 p + pt of the cloud, absolute coordinates
        float d[2][3];
        const float *frow[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const size_t row = (size_t)cloud * GA_N + 32 * wave + 16 * p + pt;
            d[p][0] = a.xyz[row * 3 + 0], d[p][1] = a.xyz[row * 3 + 1], d[p][2] = a.xyz[row * 3 + 2];
            frow[p] = a.feat + row * GA_CIN + g4;
        }
        if (s == 0 ? a.sc0.c2 == 256 : a.sc1.c2 == 256) ga_item<16>(rg, hold, frow, d, w1s, b2l + s * GA_C2MAX, pool, tid, lo_, g4, wave);
        else ga_item<24>(rg, hold, frow, d, w1s, b2l + s * GA_C2MAX, pool, tid, lo_, g4, wave);
        __syncthreads();
        // max over the four waves, then bias and ReLU once per channel (max_i relu(x_i + b) = relu(max_i x_i + b))
        {
            float *o = a.out + (size_t)cloud * a.cout_total + (s ? a.sc1.off : a.sc0.off);
#pragma unroll
            for (int c = tid; c < GA_C3; c += GA_NTH) {
                float m = pool[c];
#pragma unroll
                for (int w = 1; w < GA_NWV; ++w) m = fmaxf(m, pool[w * GA_C3 + c]);
                o[c] = fmaxf(m + b3l[s * GA_C3 + c], 0.f);
            }
        }
        // (the next write to `pool` is two layers away: no barrier needed here)
    }
}

bool ga_scale_ok(int c2, const void *w, const float *wxyz, const float *b1, const float *b2, const float *b3, int off, int cout_total) {
    if (c2 != 256 && c2 != 384) return false;
    if (!w || !wxyz || !b1 || !b2 || !b3) return false;
    if (((uintptr_t)w & 15) || ((uintptr_t)wxyz & 15) || ((uintptr_t)b1 & 3) || ((uintptr_t)b2 & 3) || ((uintptr_t)b3 & 3)) return false;
    return off >= 0 && !(off & 3) && off + GA_C3 <= cout_total;
}

}  // namespace

extern "C" {

int gp_sa_groupall_bf16x9(int b, int n, int cin, int c1, int c3, const float *xyz, const float *feat, int c2_a, const void *w_a, const float *wxyz_a,
                          const float *bias1_a, const float *bias2_a, const float *bias3_a, int cout_off_a, int c2_b, const void *w_b,
                          const float *wxyz_b, const float *bias1_b, const float *bias2_b, const float *bias3_b, int cout_off_b, float *out,
                          int cout_total, gp_stream_t s) {
    if (b < 0 || !xyz || !feat || !out) return GP_EINVAL;
    if (n != GA_N || cin != GA_CIN || c1 != GA_C1 || c3 != GA_C3) return GP_EINVAL;  // the light encoder's GroupAll level
    if (((uintptr_t)xyz & 3) || ((uintptr_t)feat & 15) || ((uintptr_t)out & 3) || cout_total <= 0 || (cout_total & 3)) return GP_EINVAL;
    if (!ga_scale_ok(c2_a, w_a, wxyz_a, bias1_a, bias2_a, bias3_a, cout_off_a, cout_total)) return GP_EINVAL;
    const int nsc = c2_b ? 2 : 1;  // c2_b = 0: one scale
    if (nsc == 2 && !ga_scale_ok(c2_b, w_b, wxyz_b, bias1_b, bias2_b, bias3_b, cout_off_b, cout_total)) return GP_EINVAL;
    if (nsc == 2 && cout_off_a < cout_off_b + GA_C3 && cout_off_b < cout_off_a + GA_C3) return GP_EINVAL;  // overlapping output columns
    if ((long long)b * nsc > 0x3fffffff) return GP_EINVAL;
    if (b == 0) return GP_OK;
    GAArgs a;
    a.xyz = xyz, a.feat = feat, a.out = out, a.cout_total = cout_total, a.nsc = nsc, a.nitems = b * nsc;
    a.sc0 = GAScale{reinterpret_cast<const bf16x8 *>(w_a), wxyz_a, bias1_a, bias2_a, bias3_a, c2_a, cout_off_a};
    a.sc1 = nsc == 2 ? GAScale{reinterpret_cast<const bf16x8 *>(w_b), wxyz_b, bias1_b, bias2_b, bias3_b, c2_b, cout_off_b} : a.sc0;
    const int blocks = a.nitems < gp_num_cus() ? a.nitems : gp_num_cus();  // persistent: one 4-wave workgroup per CU
    return gp_launch<sa_groupall_bf16x9_kernel>(dim3(blocks), dim3(GA_NTH), GA_LDS, (hipStream_t)s, a);
}

}  // extern "C"
