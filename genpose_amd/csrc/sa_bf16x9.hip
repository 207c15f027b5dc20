// Grouping level 2 of the light / dense / lighter encoders (hoisted first layer -> 128 -> 196 -> 256 -> max over the neighbourhood) with the two
// dense layers as EXACT-PRODUCT split bf16 on the BF16 matrix pipe (bf16x9.h): every fp32 operand is hi + mid + lo, SIX of the nine cross
// products are formed as the project builds it (NPROD = SA_NPROD = GP_SA_X9_PRODUCTS = 6: all but lo.lo, lo.mid and mid.lo, together at
// most (2^-23 + 2^-32) |a b| per multiply, below the fp32 accumulation's own rounding; 8 and 9 are measurement builds), each exact in fp32, and only the fp32 accumulation rounds - the error class of sa_chain_ring_kernel<128, 196, 256, NS>
// (sa_mlp.hip), whose job, inputs and [B, 128, 256] output per scale this kernel takes over (encoder precision 'bf16x9'; the fp32 kernel
// stays selectable as 'f32').  The K tail below is fp32 and whole.
// Furthest point sampling and the ball queries see coordinates only: centres and neighbourhoods are bit-identical either way.
//
// Form: sa_bf16x3.hip's (the row front and back end is sa_rows.h's, shared with that kernel; the ring step is bf16x9.h's, shared with the
// score trunks) - 8 waves per workgroup, one persistent workgroup per CU, 32 rows per wave and iteration (one neighbourhood of 32 or two of
// 16: every weight fragment read from LDS feeds two B tiles), activations register-resident from the gather to the pooled output, layer 1
// on the fp32 VALU with the fp32 kernel's arithmetic, layer 3 transposed (activations as the A operand, lane = channel) in halves of eight
// output chunks, max over the points before bias + ReLU - except that three terms per weight do not leave layer 2 LDS-resident
// (128 x 208 x 3 x 2 B = 160 KB), so BOTH layers stream through a 2-slot LDS ring in slices of 24 KB = (one 32-wide k-block) x (8
// output chunks) x (hi, mid, lo): layer 2 as (k-block, chunk half) = 8 slices (13 chunks padded to 16 with zero weights; the MFMAs of the
// padding chunks are skipped), layer 3 as (half, k-block) = 12.  Slice s + 1 (held in registers since step s - 1) is written into the other
// slot while slot s is multiplied, slice s + 2 is requested, one barrier per slice; the slice in flight stays in flight across the barrier.
// Hidden activations stay in fp32 registers and are split one k-block at a time as the next layer consumes them.
// The 196-wide layer is padded to 208 outputs (zero weights, zero bias: ReLU(0) = 0).  Layer 3's K = 196 = 6 x 32 + 4: six k-blocks go
// through the ring, and the K TAIL OF FOUR (hidden channels 192-195 = chunk 12, lane group 0) is ONE v_mfma_f32_16x16x4_f32 per (output
// chunk, tile) on fp32 weights rebuilt exactly, (hi + mid) + lo, from the stream in the prologue (4 KB of LDS) - an exact-product fmaf chain,
// the fp32 kernels' arithmetic; it OPENS each layer-3 accumulator, before the first ring step, for every row alike.  The packed stream keeps
// its 22 slices (weights.py: pack_sa_bf16x9); the ring consumes 20: of slices 14 and 21 (layer 3's seventh k-block of either half) only the
// tail's 256 x 4 x 3 terms are read, once - nothing of layer-3 columns >= 196.
// Budget per workgroup iteration (256 rows; MI355X: v_mfma_f32_16x16x32_bf16 16 cycles, v_mfma_f32_16x16x4_f32 32, LDS 128 B/clk/CU):
//   MFMA                (4 x 13 + 6 x 16) chunks x 8 products x 2 tiles = 2 368 per wave x 16 cycles + 16 chunks x 2 tiles x 32 cycles
//                       = 38.9 k cycles per wave (43.6 k with all nine products) x 2 waves per SIMD = 78 k cycles
//   LDS fragment reads  (52 + 96) KB x 3 terms x 8 waves = 3.5 MB -> 28 k cycles;  ring writes 480 KB
// so the matrix pipe bounds it.
#include "bf16x9.h"
#include "sa_rows.h"

namespace {

using namespace gp_bf16x9;

struct SAX9Args {
    int n, np, zstride, zoff;
    const float *xyz, *new_xyz, *z;
    const int32_t *idx;
    const float *wxyz, *b1;  // layer 1 stays on the fp32 VALU (three FMAs per channel on top of the hoisted feature half)
    const bf16x8 *w;         // [22 slices][8 chunks][3 = hi, mid, lo][64 lanes] (weights.py: pack_sa_bf16x9); slices 14, 21: the K tail only
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
constexpr int SX_KB3 = SX_C2 / 32, SX_KT = SX_C2 - 32 * SX_KB3;  // layer 3's K: whole k-blocks through the ring + the tail (fp32 MFMA)
constexpr int SX_NSL = 2 * SX_KB1 + SX_NHALF * SX_KB2;            // slices of the packed stream: 8 + 14
constexpr int SX_NRING = 2 * SX_KB1 + SX_NHALF * SX_KB3;          // slices the ring consumes per iteration: 8 + 12
constexpr int SX_TAIL0 = 2 * SX_KB1 + SX_KB3;                     // the tail's slice of half h: SX_TAIL0 + h SX_KB2 (14, 21) - never in the ring
constexpr size_t SX_LDS = (size_t)(2 * SX_SLICE + SX_C1) * 16 + (size_t)(32 * SX_KB2 + SX_C3 + SX_KT * SX_C3) * sizeof(float);
static_assert(SX_NC2 > SX_NCS && SX_NC2 <= 2 * SX_NCS && SX_NC2 - SX_NCS >= SX_PER_T && SX_PER_T * SX_NTH == SX_SLICE, "slice geometry");
static_assert(SX_KT == 4 && SX_NC2 == 2 * SX_KB3 + 1 && SX_KB2 == SX_KB3 + 1 && SX_NHALF == 2, "layer 3: six k-blocks + a K tail of four = chunk 12, lane group 0");
static_assert(SX_NSL == 22 && SX_NRING == 20 && SX_TAIL0 + SX_KB2 == SX_NSL - 1, "the stream has 22 slices; the ring skips 14 and 21");
static_assert(SX_LDS <= 160 * 1024, "LDS");

// Keeps a value's uses behind this point (no instruction: the optimiser may not move what is computed from it further up).
__device__ __forceinline__ void sx_pin(f32x4 &v) { asm volatile("" : "+v"(v)); }

struct SXRing {
    bf16x8 *ring;
    const bf16x8 *w;
    int par, snext;  // slot of the slice being multiplied; slice to request next
};

// The slice the ring consumes after slice s: the stream's next, past a tail slice (13 -> 15), wrapping to the next iteration's first
// (20 -> 0).  Prologue (0 in the slot, 1 held, 2 to request), steady state and wrap all walk this one sequence of SX_NRING slices.
__device__ __forceinline__ int sx_next_slice(int s) {
    const int n = s + 1 + (s + 1 == SX_TAIL0 || s + 1 == SX_TAIL0 + SX_KB2);
    return n >= SX_NSL ? 0 : n;
}

// One step of the ring (bf16x9.h: ring_step) over the current slot, chunks [N0, N0 + NCH) of acc; the weight stream wraps over the
// iteration's SX_NRING slices (sx_next_slice).
template <bool TRANSPOSED, int N0, int NCH, int NA>
__device__ __forceinline__ void sx_step(SXRing &r, bf16x8 (&hold)[SX_PER_T], const Split8 (&xs)[2], f32x4 (&acc)[2][NA], int tid, int lane) {
    static_assert(NCH <= SX_NCS, "chunks of one slice");
    const bf16x8 *slot = r.ring + r.par * SX_SLICE;
    bf16x8 *dst = r.ring + (r.par ^ 1) * SX_SLICE;
    const bf16x8 *src = r.w + (size_t)r.snext * SX_SLICE;
    r.par ^= 1;
    r.snext = sx_next_slice(r.snext);
    ring_step<SX_NTH, SX_PER_T, TRANSPOSED, N0, NCH, SA_NPROD>(slot, dst, src, hold, xs, acc, tid, lane);
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
    float *wtl = b3l + C3;                                          // [KT][C3]: layer 3's K tail W3[c][32 KB3 + e] in fp32
    const int tid = threadIdx.x, lane = tid & 63, pt = lane & 15, g = lane >> 4;
    gp_sa_rows::stage_operands<C1, 32 * KB2, C3, NTH>(a, w1l, b2l, b3l, tid);
    // layer 3's K tail from the stream: output channel c = 16 (8 h + n) + l sits in slice (h, k-block KB3), chunk n, lane l < 16 (lane group
    // 0: k = 32 KB3 + e for elements e < 4).  Only those 8 bytes of each term are read; (hi + mid) + lo gives the fp32 weight back exactly.
    for (int c = tid; c < C3; c += NTH) {
        const bf16x8 *src = a.w + (size_t)(SX_TAIL0 + (c >> 7) * KB2) * SX_SLICE + ((c >> 4) & (NCS - 1)) * 3 * 64 + (c & 15);
        uint2 t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = *reinterpret_cast<const uint2 *>(src + k * 64);
#pragma unroll
        for (int e = 0; e < SX_KT; ++e) {
            float v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) v[k] = __uint_as_float(((e < 2 ? t[k].x : t[k].y) >> (16 * (e & 1))) << 16);
            wtl[e * C3 + c] = (v[0] + v[1]) + v[2];
        }
    }
    // ring prologue: slice 0 into slot 0; slice 1 held in registers (written during step 0)
    bf16x8 hold[SX_PER_T];
#pragma unroll
    for (int u = 0; u < SX_PER_T; ++u) {
        ring[tid + u * NTH] = a.w[tid + u * NTH];
        hold[u] = a.w[SX_SLICE + tid + u * NTH];
    }
    __syncthreads();
    SXRing rg = {ring, a.w, 0, 2};
    // every wave runs the same number of iterations (idle ones compute on clamped rows and store nothing): barrier counts match
    const gp_sa_rows::Units<NS> un(nunits_total, NWV, tid);
    const int nits_wg = un.nits_all(nunits_total);
    int jcur[2], jn[2];
    float dcur[2][3];
    un.load_idx(a, 0, pt, jcur);
    un.load_d(a, 0, jcur, dcur);
    un.load_idx(a, 1, pt, jn);
#pragma unroll 1
    for (int it = 0; it < nits_wg; ++it) {
        int lo_ = lane;
        asm volatile("" : "+v"(lo_));  // keep the LDS operand reads inside the loop (see sa_chain_lds_kernel)
        const int g4 = (lo_ >> 4) * 4;
        // ---- layers 1 + 2: k-block by k-block; the hoisted feature rows of k-block kb + 1 are requested while kb is multiplied
        const float *zrow[2];
        un.z_rows(a, it, jcur, g4, zrow);
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
                f32x4 h[2];
#pragma unroll
                for (int c = 0; c < 2; ++c) h[c] = gp_sa_rows::layer1(w1l, 2 * kb + c, g4, zz[s][c], dcur[s][0], dcur[s][1], dcur[s][2]);  // chunks 2 kb, 2 kb + 1
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
        const bool cur_valid = it < un.my_units;
        const int unit = un.unit_of(it);
        un.advance(a, it, pt, jcur, jn, dcur);
        // ---- bias + ReLU of the hidden layer, kept in fp32 (bias zero on the padding channels of chunk 12: they stay zero)
#pragma unroll
        for (int n = 0; n < NC2; ++n) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(b2l + 16 * n + g4);
#pragma unroll
            for (int s = 0; s < 2; ++s) acc2[s][n] = relu4(acc2[s][n] + bv);
        }
        // ---- layer 3's K tail as the A operand of v_mfma_f32_16x16x4_f32: lane (pt, g) holds h2[pt][32 KB3 + g] = register g of chunk
        // NC2 - 1 in lane pt (lane group 0); once per iteration, kept across the two halves
        float atail[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const f32x4 v = acc2[s][NC2 - 1];
            const int from = (lo_ & 15) * 4;
            const float t0 = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(v.x)));
            const float t1 = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(v.y)));
            const float t2 = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(v.z)));
            const float t3 = __int_as_float(__builtin_amdgcn_ds_bpermute(from, __float_as_int(v.w)));
            atail[s] = g4 == 0 ? t0 : g4 == 4 ? t1 : g4 == 8 ? t2 : t3;
        }
        // ---- layer 3 (transposed: lane = channel, registers x lane groups = the 16 points of a sub-chunk), eight output chunks at a time
#pragma unroll 1
        for (int half = 0; half < NHALF; ++half) {
            f32x4 acc3[2][NCS];
            // the tail opens the accumulators (a literal-zero C operand: no zero fill): B = Wtail[g][channel 16 chunk + pt].  (After the last
            // ring step instead it measured the same: 3 119 / 3 179 against 3 122 / 3 175 us for both scales at 640 clouds.)
#pragma unroll
            for (int n = 0; n < NCS; ++n) {
                const float bt = wtl[(g4 >> 2) * C3 + 16 * (half * NCS + n) + (lo_ & 15)];
#pragma unroll
                for (int s = 0; s < 2; ++s) acc3[s][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(atail[s], bt, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
            }
#pragma unroll
            for (int kb = 0; kb < SX_KB3; ++kb) {
                Split8 xs[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    // (pinned: the split does not depend on `half`, and hoisted out of that loop all 12 of them would live in registers)
                    sx_pin(acc2[s][2 * kb]);
                    sx_pin(acc2[s][2 * kb + 1]);
                    xs[s] = split8(acc2[s][2 * kb], acc2[s][2 * kb + 1]);
                }
                sx_step<true, 0, NCS>(rg, hold, xs, acc3, tid, lo_);
            }
            // pooling over the points, bias + ReLU, store
#pragma unroll
            for (int n = 0; n < NCS; ++n)
                gp_sa_rows::pooled_store<NS>(a, b3l, acc3[0][n], acc3[1][n], 16 * (half * NCS + n) + (lo_ & 15), unit, cur_valid && g == 0);
        }
    }
}

template <int NS>
int launch_bf16x9(const SAX9Args &a, int b, hipStream_t st) {
    const int nunits = (int)(((size_t)b * a.np * NS) / 32);
    int blocks = (nunits + SX_NWV - 1) / SX_NWV;
    if (blocks > gp_num_cus()) blocks = gp_num_cus();  // persistent: one 8-wave workgroup per CU
    return gp_launch<sa_chain_bf16x9_kernel<NS>>(dim3(blocks), dim3(SX_NTH), SX_LDS, st, a, nunits);
}

}  // namespace

extern "C" {

int gp_sa_pre_mlp_max_bf16x9(int b, int n, int np, int ns, int c1, int c2, int c3, const float *xyz, const float *new_xyz, const int32_t *idx,
                             const float *z, int zstride, int zoff, const float *wxyz, const float *bias1, const void *w23_x9, const float *bias2,
                             const float *bias3, float *out, int cout_total, int cout_off, gp_stream_t s) {
    if (!gp_sa_rows::units_args_ok(b, n, np, ns, c1, c3, zstride, zoff, cout_total, cout_off, {xyz, new_xyz, idx, z, wxyz, bias1, w23_x9, bias2, bias3, out}))
        return GP_EINVAL;
    if (c1 != SX_C1 || c2 != SX_C2 || c3 != SX_C3 || (ns != 16 && ns != 32)) return GP_EINVAL;  // grouping level 2
    if (b == 0) return GP_OK;
    const SAX9Args a{n, np, zstride, zoff, xyz, new_xyz, z, idx, wxyz, bias1, reinterpret_cast<const bf16x8 *>(w23_x9), bias2, bias3, out, cout_total, cout_off};
    return ns == 32 ? launch_bf16x9<32>(a, b, (hipStream_t)s) : launch_bf16x9<16>(a, b, (hipStream_t)s);
}

}  // extern "C"
